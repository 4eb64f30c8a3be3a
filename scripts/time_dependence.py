#!/usr/bin/env python3
"""Time the dependence stage on the device (needs a GPU).

The default nod detector is fitted on the synthetic tests.json of seed 0;
its partial dependence is then taken on the file of seed 1 with the
default grid (up to 20 values for each of the 16 features).

  fused   device events around ops.partial_dependence on resident inputs,
          with and without the ICE output: the two launches for the
          unmodified rows, the job upload, the one launch for all J jobs
          and the small reduction launch;
  loop    device events around the loop it replaces, on the same inputs:
          per job a column fill into a fresh [M, 16] matrix, detect_encode,
          forest_proba, a sum of acc1 and a count of the argmax rule.
          Median, min and max over --reps, fused and loop alternating in
          this process after a warm-up call of each; the two must return
          the same ICE bits and the same counts;
  stage   host clock around dependence(backend="hip") as a user calls it
          (load, grid, upload, launches, readback, the result dict).

Prints one JSON line.  Usage:
  python scripts/time_dependence.py [--n 10000] [--reps 10] [--grid 20]
                                    [--n-trees N]
"""

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np


def _events(fn):
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / 1000.0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--n-trees", type=int, default=None)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "time_dependence needs a GPU"

    from flake16_framework_amd.configgrid import SHAP_CONFIGS
    from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
    from flake16_framework_amd.engine import dependence as P
    from flake16_framework_amd.engine import detector as D
    from flake16_framework_amd.engine import holdout as H
    from flake16_framework_amd.ops.backend import get_ops

    ops = get_ops()
    det = D.fit_detector(
        SHAP_CONFIGS[0], tests=make_synthetic_tests(n_tests=args.n, seed=0),
        seed=0, backend="hip", n_trees=args.n_trees)
    tests = make_synthetic_tests(n_tests=args.n, seed=1)

    names, seg_off = H._project_rows(tests)
    X, _, _ = D.load_rows(det, tests, None)
    grids = P.make_grids(X, args.grid)
    job_col = np.array([f for f, v in enumerate(grids) for _ in v],
                       dtype=np.int32)
    job_val = np.concatenate(grids)
    G, M, J = len(names), len(X), len(job_col)

    d = H.grouped_inputs([det], X, seg_off)
    one = D.device_inputs(det, X)
    col_t, val_t = torch.from_numpy(job_col), torch.from_numpy(job_val)
    jobs = [(int(f), float(v)) for f, v in zip(job_col, job_val)]

    def fused(want_ice=True):
        return P.partial_dependence(ops, d, col_t, val_t, None, want_ice)

    def loop():
        ice, sums, counts = [], [], []
        for f, v in jobs:
            Xp = one["X64"].clone()
            Xp[:, f] = v
            codes = ops.detect_encode(
                Xp, one["mean"], one["scale"], one["pca_mean"], one["W"],
                one["has_pca"], one["cuts"], one["cut_off"], one["F"])
            acc = ops.forest_proba(codes, one["tree_off"], one["nodes"],
                                   one["n_trees"])
            ice.append(acc[:, 1])
            sums.append(acc[:, 1].sum())
            counts.append((acc[:, 1] > acc[:, 0]).sum())
        return torch.stack(ice), torch.stack(sums), torch.stack(counts)

    S, flagged, ice = fused()                                     # warm-up
    ice_loop, _, counts_loop = loop()
    assert torch.equal(ice, ice_loop)
    assert torch.equal(flagged[:J, G].long(), counts_loop)
    S_off, flagged_off, _ = fused(False)
    assert torch.equal(S, S_off) and torch.equal(flagged, flagged_off)
    torch.cuda.synchronize()
    t_fused, t_noice, t_loop = [], [], []
    for _ in range(args.reps):
        t_fused.append(_events(fused)[0])
        t_noice.append(_events(lambda: fused(False))[0])
        t_loop.append(_events(loop)[0])

    P.dependence(det, tests=tests, grid=2, backend="hip")        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = P.dependence(det, tests=tests, grid=args.grid, backend="hip")
    t_stage = time.perf_counter() - t0

    top = sorted(res["features"].items(), key=lambda kv: -kv[1]["range"])[:3]
    stats = lambda t: {"median": float(np.median(t)), "min": float(min(t)),
                       "max": float(max(t))}
    print(json.dumps({
        "n_tests": M, "n_projects": G, "n_trees": det.n_trees,
        "n_nodes": int(len(det.feat)), "jobs": J, "reps": args.reps,
        "fused_ice_s": stats(t_fused), "fused_s": stats(t_noice),
        "loop_s": stats(t_loop), "stage_wall_s": round(t_stage, 4),
        "baseline": [res["baseline"]["mean_proba"],
                     res["baseline"]["flagged"]],
        "largest_range": [[k, v["range"]] for k, v in top],
    }))


if __name__ == "__main__":
    main()
