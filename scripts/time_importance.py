#!/usr/bin/env python3
"""Time the importance stage on the device (needs a GPU).

The default nod detector is fitted on the synthetic tests.json of seed 0;
its permutation importance is then taken on the file of seed 1 with the
default groups (16 features + 3 families) and --repeats permutations.

  fused   device events around ops.permuted_counts on resident inputs:
          the two launches for the unpermuted rows, the permutation table's
          check and upload, and the one launch for all J * R jobs;
  loop    device events around the loop it replaces, on the same inputs
          with the table already resident: per job a torch gather of the
          permuted columns into a fresh [M, 16] matrix, then detect_encode
          + forest_proba + threshold_counts (K = 1).
          Median, min and max over --reps, fused and loop alternating in
          this process after a warm-up call of each; the two must return
          the same counts;
  stage   host clock around importance(backend="hip") as a user calls it
          (load, table, upload, launches, readback, metrics).

Prints one JSON line.  Usage:
  python scripts/time_importance.py [--n 10000] [--reps 10] [--repeats 5]
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-trees", type=int, default=None)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "time_importance needs a GPU"

    from flake16_framework_amd.configgrid import SHAP_CONFIGS
    from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
    from flake16_framework_amd.engine import detector as D
    from flake16_framework_amd.engine import holdout as H
    from flake16_framework_amd.engine import importance as I
    from flake16_framework_amd.ops.backend import get_ops

    ops = get_ops()
    det = D.fit_detector(
        SHAP_CONFIGS[0], tests=make_synthetic_tests(n_tests=args.n, seed=0),
        seed=0, backend="hip", n_trees=args.n_trees)
    tests = make_synthetic_tests(n_tests=args.n, seed=1)

    names, seg_off = H._project_rows(tests)
    X, _, _ = D.load_rows(det, tests, None)
    y = np.array([row[1] == det.flaky_label for rows in tests.values()
                  for row in rows.values()], dtype=np.uint8)
    _, _, masks = I._group_masks(det, I.default_groups(det))
    perm = I.make_permutations(seg_off, args.repeats, 0)
    G, M, F = len(names), len(X), det.n_features

    d = H.grouped_inputs([det], X, seg_off)
    one = D.device_inputs(det, X)
    dev = d["X64"].device
    labels_dev = torch.from_numpy(y).to(dev)
    det_of_group = torch.zeros(G, dtype=torch.int32)
    perm_t, masks_t = torch.from_numpy(perm), torch.from_numpy(masks)
    perm_dev = perm_t.to(dev).long()
    cols = [torch.tensor([f for f in range(F) if int(m) >> f & 1],
                         device=dev) for m in masks]
    half = torch.tensor([0.5], dtype=torch.float64)

    def fused():
        return I.permuted_counts(ops, d, labels_dev, det_of_group, perm_t,
                                 masks_t)[0]

    def loop():
        out = []
        for c in cols:
            for r in range(args.repeats):
                Xp = one["X64"].clone()
                Xp[:, c] = one["X64"][perm_dev[r][:, None], c[None, :]]
                codes = ops.detect_encode(
                    Xp, one["mean"], one["scale"], one["pca_mean"],
                    one["W"], one["has_pca"], one["cuts"], one["cut_off"],
                    one["F"])
                acc = ops.forest_proba(codes, one["tree_off"], one["nodes"],
                                       one["n_trees"])
                out.append(ops.threshold_counts(
                    acc, labels_dev, d["seg_off"], one["n_trees"], half)[1])
        return torch.stack(out).view(len(cols), args.repeats, G + 1, 3)

    assert torch.equal(fused(), loop())                           # warm-up
    torch.cuda.synchronize()
    t_fused, t_loop = [], []
    for _ in range(args.reps):
        t_fused.append(_events(fused)[0])
        t_loop.append(_events(loop)[0])

    I.importance(det, tests=tests, repeats=1, backend="hip")     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = I.importance(det, tests=tests, repeats=args.repeats, seed=0,
                       backend="hip")
    t_stage = time.perf_counter() - t0

    top = sorted(res["importance"].items(),
                 key=lambda kv: -(kv[1]["f1_drop_mean"] or 0.0))[:3]
    stats = lambda t: {"median": float(np.median(t)), "min": float(min(t)),
                       "max": float(max(t))}
    print(json.dumps({
        "n_tests": M, "n_projects": G, "n_trees": det.n_trees,
        "n_nodes": int(len(det.feat)), "groups": len(masks),
        "repeats": args.repeats, "reps": args.reps,
        "fused_s": stats(t_fused), "loop_s": stats(t_loop),
        "stage_wall_s": round(t_stage, 4),
        "baseline": res["baseline"]["total"],
        "largest_f1_drop_mean": [[k, v["f1_drop_mean"]] for k, v in top],
    }))


if __name__ == "__main__":
    main()
