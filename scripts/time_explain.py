#!/usr/bin/env python3
"""Time the explain stage's kernel against the shap stage's (needs a GPU).

A detector is fitted on synthetic tests (seed 0) and the rows of a second
synthetic file (seed 1) are encoded once; on those resident codes, after a
warm-up of both, device events time alternately

  merged   detector_shap (ops/hip/detector_shap.hip) over the merged-path table
  paths    treeshap_paths (ops/hip/treeshap.hip) over the same trees'
           root->leaf node paths

(median and min over --reps), and the two results are compared (they are
negations of each other up to rounding).  Also reported: the end-to-end
explain() wall time, which adds reading the rows, building the table and the
transfers, and the forest's leaf / element counts.

Prints one JSON line.  Usage:
  python scripts/time_explain.py [--n 10000] [--config nod|od] [--reps 7]
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
    assert torch.cuda.is_available(), "time_explain needs a GPU"

    from flake16_framework_amd.configgrid import SHAP_CONFIGS
    from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
    from flake16_framework_amd.engine import detector as D
    from flake16_framework_amd.engine import explain as E
    from flake16_framework_amd.models.leafpaths import build_leaf_paths
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    from flake16_framework_amd.ops.backend import get_ops

    keys = SHAP_CONFIGS[("nod", "od").index(args.config)]
    train = make_synthetic_tests(n_tests=args.n, seed=0)
    other = make_synthetic_tests(n_tests=args.n, seed=1)
    det = D.fit_detector(keys, tests=train, backend="hip",
                         n_trees=args.n_trees)

    ops = get_ops()
    X, _, _ = D.load_rows(det, other, None)
    d = D.device_inputs(det, X)
    dev = d["X64"].device
    codes = ops.detect_encode(d["X64"], d["mean"], d["scale"], d["pca_mean"],
                              d["W"], d["has_pca"], d["cuts"], d["cut_off"],
                              d["F"])

    t0 = time.perf_counter()
    paths = build_merged_paths(det)
    t_table = time.perf_counter() - t0
    table = E.device_table(paths, dev)

    node_alloc = np.diff(det.tree_off)
    leaf_tree, leaf_off, path_nodes, max_depth = build_leaf_paths(
        det.feat, det.left, det.tree_off[:-1], node_alloc)
    assert max_depth <= 128, "treeshap_paths holds paths up to 128 nodes"
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    old_args = (codes, put(leaf_tree), put(leaf_off), put(path_nodes),
                put(det.tree_off[:-1]), put(det.feat), put(det.split),
                put(det.left), put(det.cnt0), put(det.cnt1))

    def merged():
        return E.device_shap(ops, codes, table, det.n_trees, det.n_features)

    def node_paths():
        return ops.treeshap_paths(*old_args)

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / 1000.0, out

    phi_new, phi_old = merged(), node_paths()                    # warm-up
    torch.cuda.synchronize()
    diff = float((phi_new + phi_old / det.n_trees).abs().max())
    t_new, t_old = [], []
    for _ in range(args.reps):
        t_new.append(timed(merged)[0])
        t_old.append(timed(node_paths)[0])
        print(f"merged {t_new[-1]:.4f} s  paths {t_old[-1]:.4f} s",
              file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    res = E.explain(det, tests=other, backend="hip")
    t_e2e = time.perf_counter() - t0
    gap = float(np.abs(res["base_value"] + res["phi"].sum(axis=1)
                       - res["proba"]).max())

    n_el = np.diff(paths.leaf_off)
    med_new, med_old = float(np.median(t_new)), float(np.median(t_old))
    print(json.dumps({
        "config": list(keys), "n_train": det.n_train, "m": len(X),
        "n_trees": det.n_trees, "n_nodes": int(len(det.feat)),
        "n_leaves": paths.n_leaves, "n_elements": paths.n_elements,
        "max_elements_per_leaf": int(n_el.max()),
        "mean_elements_per_leaf": round(float(n_el.mean()), 2),
        "path_nodes": int(len(path_nodes)), "max_depth": max_depth,
        "reps": args.reps,
        "merged_s_median": med_new, "merged_s_min": float(min(t_new)),
        "paths_s_median": med_old, "paths_s_min": float(min(t_old)),
        "speedup_median": round(med_old / med_new, 2),
        "max_abs_diff_merged_vs_paths": diff,
        "build_table_s": round(t_table, 4),
        "explain_end_to_end_s": round(t_e2e, 4),
        "max_additivity_gap": gap,
    }))


if __name__ == "__main__":
    main()
