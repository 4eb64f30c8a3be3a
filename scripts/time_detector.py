#!/usr/bin/env python3
"""Time the fit and detect stages on the device (needs a GPU).

  fit     host clock around fit_detector(backend="hip") ending in a device
          synchronize, after a small warm-up fit has loaded the kernels;
  detect  device events around the two-kernel hot path (detect_encode +
          forest_proba) on resident inputs, after a warm-up call: median
          and min over --reps; plus the end-to-end detect() wall time,
          which includes reading the rows out of the tests dict.

Prints one JSON line.  Usage:
  python scripts/time_detector.py [--n 10000] [--config nod|od] [--reps 50]
"""

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000,
                    help="training tests and tests to classify")
    ap.add_argument("--config", choices=("nod", "od"), default="nod")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "time_detector needs a GPU"

    from flake16_framework_amd.configgrid import SHAP_CONFIGS
    from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
    from flake16_framework_amd.engine import detector as D
    from flake16_framework_amd.ops.backend import get_ops

    keys = SHAP_CONFIGS[("nod", "od").index(args.config)]
    train = make_synthetic_tests(n_tests=args.n, seed=0)
    other = make_synthetic_tests(n_tests=args.n, seed=1)

    D.fit_detector(keys, tests=train, backend="hip", n_trees=2)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    det = D.fit_detector(keys, tests=train, backend="hip")
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0

    ops = get_ops()
    X, _, _ = D.load_rows(det, other, None)
    inputs = D.device_inputs(det, X)
    D.device_acc(ops, inputs)                                     # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        D.device_acc(ops, inputs)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1000.0)
    t_dev = float(np.median(times))

    t0 = time.perf_counter()
    res = D.detect(det, tests=other, backend="hip")
    t_e2e = time.perf_counter() - t0

    print(json.dumps({
        "config": list(keys), "n_train": det.n_train, "m": len(X),
        "n_trees": det.n_trees, "n_nodes": int(len(det.feat)),
        "fit_s": round(t_fit, 4), "fit_rows_per_s": round(args.n / t_fit, 1),
        "detect_device_s_median": t_dev,
        "detect_device_s_min": float(min(times)),
        "detect_device_rows_per_s": round(len(X) / t_dev, 1),
        "detect_end_to_end_s": round(t_e2e, 4),
        "predicted_flaky": int(res["pred"].sum()),
    }))


if __name__ == "__main__":
    main()
