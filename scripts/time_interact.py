#!/usr/bin/env python3
"""Time the interact stage's op against explain's (needs a GPU).

A detector is fitted on synthetic tests (seed 0) and the rows of a second
synthetic file (seed 1) are encoded once; on those resident codes, after a
warm-up of both, device events time alternately

  interact  detector_shap_interactions (ops/hip/detector_shap.hip), given phi
  shap      detector_shap (the same file and tree kernel) on the same rows

(median, min and max over --reps).  The op count predicts a ratio of about
the mean number of elements per leaf: every leaf is visited once per
element, on a path one shorter.  That mean is reported, and the inner-loop
iterations per row of both ops: a path of n elements takes n (n + 1) / 2
iterations of EXTEND and n^2 of the unwound sums, each with one or two
fp64 divisions; detector_shap runs every leaf's path, the new op n paths
of n - 1 elements per leaf.

Also reported: the end-to-end interact() wall time after a warm-up call,
which adds reading the rows, building the table, explain's ops and the
readback of the [M, F, F] array, and the invariants of the result at the
timed size.

Prints one JSON line.  Usage:
  python scripts/time_interact.py [--n 10000] [--config nod|od] [--reps 7]
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
                    help="training tests and tests to explain")
    ap.add_argument("--config", choices=("nod", "od"), default="nod")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n-trees", type=int, default=None)
    args = ap.parse_args()
    assert args.reps >= 5

    import torch
    assert torch.cuda.is_available(), "time_interact needs a GPU"

    from flake16_framework_amd.configgrid import SHAP_CONFIGS
    from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
    from flake16_framework_amd.engine import detector as D
    from flake16_framework_amd.engine import explain as E
    from flake16_framework_amd.engine import interact as I
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    from flake16_framework_amd.ops.backend import get_ops

    keys = SHAP_CONFIGS[("nod", "od").index(args.config)]
    train = make_synthetic_tests(n_tests=args.n, seed=0)
    other = make_synthetic_tests(n_tests=args.n, seed=1)
    det = D.fit_detector(keys, tests=train, backend="hip",
                         n_trees=args.n_trees)

    ops = get_ops()
    X, _, _ = D.load_rows(det, other, None)
    paths = build_merged_paths(det)
    codes, table, _, phi = E.explain_device(ops, det, paths, X)
    F = det.n_features

    def shap():
        return E.device_shap(ops, codes, table, det.n_trees, F)

    def inter():
        return I.device_interactions(ops, codes, table, phi, det.n_trees, F)

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / 1000.0, out

    shap(), inter()                                             # warm-up
    torch.cuda.synchronize()
    t_int, t_shap = [], []
    for _ in range(args.reps):
        t_int.append(timed(inter)[0])
        t_shap.append(timed(shap)[0])
        print(f"interact {t_int[-1]:.4f} s  shap {t_shap[-1]:.4f} s",
              file=sys.stderr, flush=True)

    I.interact(det, tests=other, backend="hip")                 # warm-up
    t0 = time.perf_counter()
    res = I.interact(det, tests=other, backend="hip")
    t_e2e = time.perf_counter() - t0
    phi_h, mat = res["phi"], res["interactions"]
    row_gap = float(np.abs(mat.sum(axis=2) - phi_h).max())
    gap = float(np.abs(res["base_value"] + mat.sum(axis=(1, 2))
                       - res["proba"]).max())
    asym = float(np.abs(mat - mat.transpose(0, 2, 1)).max())
    off = mat[:, ~np.eye(F, dtype=bool)]

    n_el = np.diff(paths.leaf_off).astype(np.int64)
    iters = lambda n: n * (n + 1) // 2 + n * n
    it_shap = int(iters(n_el).sum())
    it_int = int((n_el * iters(n_el - 1)).sum())
    med_int, med_shap = float(np.median(t_int)), float(np.median(t_shap))
    print(json.dumps({
        "config": list(keys), "n_train": det.n_train, "m": len(X),
        "n_trees": det.n_trees, "n_features": F,
        "n_leaves": paths.n_leaves, "n_elements": paths.n_elements,
        "max_elements_per_leaf": int(n_el.max()),
        "mean_elements_per_leaf": round(float(n_el.mean()), 2),
        "inner_iterations_per_row_shap": it_shap,
        "inner_iterations_per_row_interact": it_int,
        "inner_iterations_ratio": round(it_int / it_shap, 2),
        "reps": args.reps,
        "interact_s_median": med_int, "interact_s_min": float(min(t_int)),
        "interact_s_max": float(max(t_int)),
        "shap_s_median": med_shap, "shap_s_min": float(min(t_shap)),
        "shap_s_max": float(max(t_shap)),
        "ratio_median": round(med_int / med_shap, 2),
        "interact_end_to_end_s": round(t_e2e, 4),
        "max_row_sum_gap": row_gap, "max_additivity_gap": gap,
        "max_asymmetry": asym,
        "max_abs_off_diagonal": float(np.abs(off).max()),
    }))


if __name__ == "__main__":
    main()
