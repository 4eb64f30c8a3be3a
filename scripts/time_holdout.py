#!/usr/bin/env python3
"""Time the holdout stage on the device (needs a GPU).

For each of the study's two best configurations (nod, od) on the synthetic
tests.json:

  phases   host clock per phase of holdout(backend="hip"), each ending in
           a device synchronize, after a small warm-up run has loaded the
           kernels: host preprocessing, cuts + balancing, fused forest fit,
           grouped evaluation (upload, three launches, readback);
  eval     device events around (a) the three grouped launches
           holdout_encode + holdout_proba + threshold_counts on resident
           inputs, and (b) the loop they replace: detect_encode +
           forest_proba per project with that project's parameter upload.
           Median and min over --reps, both in this process, (a) and (b)
           alternating;
  fit      host clock around the fused fit phases of holdout against G
           separate fit_detector(backend="hip") calls on the same folds.

Prints one JSON line.  Usage:
  python scripts/time_holdout.py [--n 10000] [--projects 26] [--reps 30]
                                 [--n-trees N]
"""

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np


def _events(fn, reps):
    import torch
    times = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1000.0)
    return times


def time_config(keys, tests, reps, n_trees):
    import torch

    from flake16_framework_amd.engine import detector as D
    from flake16_framework_amd.engine import holdout as H
    from flake16_framework_amd.ops.backend import get_ops

    ops = get_ops()
    H.holdout(keys, tests=tests, backend="hip", n_trees=2)        # warm-up
    torch.cuda.synchronize()

    phases, last = {}, [time.perf_counter()]

    def timer(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        phases[name] = round(now - last[0], 4)
        last[0] = now

    t0 = time.perf_counter()
    last[0] = t0
    res = H.holdout(keys, tests=tests, backend="hip", n_trees=n_trees,
                    keep_detectors=True, timer=timer)
    torch.cuda.synchronize()
    t_stage = time.perf_counter() - t0
    dets = res["detectors"]
    names, seg_off = H._project_rows(tests)

    # (a) grouped launches and (b) the per-project loop, resident inputs
    first = dets[0]
    X, _, _ = D.load_rows(first, tests, None)
    labels = np.concatenate(
        [[row[1] == first.flaky_label for row in rows.values()]
         for rows in tests.values()]).astype(np.uint8)
    d = H.grouped_inputs(dets, X, seg_off)
    labels_dev = torch.from_numpy(labels).to(d["X64"].device)
    thresholds = torch.from_numpy(res["thresholds"])
    per_proj = [D.device_inputs(det, X[seg_off[g]:seg_off[g + 1]])
                for g, det in enumerate(dets)]

    def grouped():
        return H.grouped_eval(ops, d, labels_dev, thresholds)

    def loop():
        return [D.device_acc(ops, one) for one in per_proj]

    acc = grouped()[0]
    assert torch.equal(acc, torch.cat(loop()))                    # warm-up
    torch.cuda.synchronize()
    t_a, t_b = [], []
    for _ in range(reps):
        t_a += _events(grouped, 1)
        t_b += _events(loop, 1)

    # fused fit against G separate fits of the same folds
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for held in names:
        train = {p: rows for p, rows in tests.items() if p != held}
        D.fit_detector(keys, tests=train, backend="hip", n_trees=n_trees)
    torch.cuda.synchronize()
    t_separate = time.perf_counter() - t0

    best = H.best_f1_threshold(res["total"]["curve"], res["thresholds"])
    fused = sum(phases[k] for k in ("host_preprocessing", "cuts_balancing",
                                    "forest_fit", "assemble"))
    return {
        "config": list(keys), "n_tests": len(X), "n_projects": len(names),
        "n_trees": res["n_trees"],
        "n_nodes": int(sum(len(det.feat) for det in dets)),
        "stage_wall_s": round(t_stage, 4), "phase_wall_s": phases,
        "eval_grouped_s_median": float(np.median(t_a)),
        "eval_grouped_s_min": float(min(t_a)),
        "eval_loop_s_median": float(np.median(t_b)),
        "eval_loop_s_min": float(min(t_b)),
        "fit_fused_wall_s": round(fused, 4),
        "fit_separate_wall_s": round(t_separate, 4),
        "pooled_argmax": res["total"]["argmax"],
        "best_f1_threshold": best and list(best),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--projects", type=int, default=26)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--n-trees", type=int, default=None)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "time_holdout needs a GPU"

    from flake16_framework_amd.configgrid import SHAP_CONFIGS
    from flake16_framework_amd.dataset.synthetic import make_synthetic_tests

    tests = make_synthetic_tests(n_tests=args.n, n_projects=args.projects,
                                 seed=0)
    print(json.dumps({
        name: time_config(SHAP_CONFIGS[i], tests, args.reps, args.n_trees)
        for i, name in enumerate(("nod", "od"))}))


if __name__ == "__main__":
    main()
