#!/usr/bin/env python3
"""Time the similar stage on the device (needs a GPU).

The default nod detector is fitted on the synthetic tests.json of seed 0;
the file of seed 1 is then queried against the seed-0 corpus with k = 5.

  leaves  device events around ops.forest_leaves on the resident codes of
          both files (the walk alone);
  fused   device events around ops.proximity_topk on the resident leaf
          matrices: the 16-bit check, the repack and the top-k launches;
  torch   device events around the same result from torch ops on the same
          matrices: (lq[:, t, None] == lc[None, :, t]) accumulated per
          tree in query chunks of --chunk rows, then torch.topk of the
          int64 key shared * N + (N - 1 - idx), which is exact.
          Median, min and max over --reps, fused and torch alternating in
          this process after a warm-up call of each; the two must return
          the same idx and shared, or the script fails;
  stage   host clock around similar(backend="hip") as a user calls it
          (load, encode, upload, launches, readback).

Comparisons per second are M * N * T over the fused median.  Prints one
JSON line.  Usage:
  python scripts/time_similar.py [--n 10000] [--reps 10] [--k 5]
                                 [--n-trees N] [--chunk 2048]
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
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--n-trees", type=int, default=None)
    ap.add_argument("--chunk", type=int, default=2048)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "time_similar needs a GPU"

    from flake16_framework_amd.configgrid import SHAP_CONFIGS
    from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
    from flake16_framework_amd.engine import detector as D
    from flake16_framework_amd.engine import similar as S
    from flake16_framework_amd.ops.backend import get_ops

    ops = get_ops()
    corpus = make_synthetic_tests(n_tests=args.n, seed=0)
    det = D.fit_detector(SHAP_CONFIGS[0], tests=corpus, seed=0,
                         backend="hip", n_trees=args.n_trees)
    tests = make_synthetic_tests(n_tests=args.n, seed=1)

    dq = D.device_inputs(det, D.load_rows(det, tests, None)[0])
    dc = D.device_inputs(det, D.load_rows(det, corpus, None)[0])
    codes_q, lq = S.device_leaves(ops, dq)
    codes_c, lc = S.device_leaves(ops, dc)
    M, N, T, k = len(lq), len(lc), det.n_trees, args.k
    dev = lq.device
    none = torch.full((M,), -1, dtype=torch.int32)
    col = torch.arange(N, device=dev, dtype=torch.int64)

    def leaves():
        return [ops.forest_leaves(c, dq["tree_off"], dq["nodes"], T)
                for c in (codes_q, codes_c)]

    def fused():
        return ops.proximity_topk(lq, lc, none, k)

    def composed():
        idx, shared = [], []
        for a in range(0, M, args.chunk):
            s = torch.zeros((min(M, a + args.chunk) - a, N),
                            dtype=torch.int32, device=dev)
            for t in range(T):
                s += lq[a:a + args.chunk, t, None] == lc[None, :, t]
            key = torch.topk(s.long() * N + (N - 1 - col), k, dim=1).values
            shared.append((key // N).int())
            idx.append((N - 1 - key % N).int())
        return torch.cat(idx), torch.cat(shared)

    got, want = fused(), composed()                               # warm-up
    equal = bool(torch.equal(got[0], want[0])
                 and torch.equal(got[1], want[1]))
    assert equal, "the fused op and the torch composition differ"
    leaves()
    torch.cuda.synchronize()
    t_fused, t_torch, t_leaves = [], [], []
    for _ in range(args.reps):
        t_fused.append(_events(fused)[0])
        t_torch.append(_events(composed)[0])
        t_leaves.append(_events(leaves)[0])

    S.similar(det, tests=tests, corpus=corpus, k=k, backend="hip")  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = S.similar(det, tests=tests, corpus=corpus, k=k, backend="hip")
    t_stage = time.perf_counter() - t0

    flagged = res["pred"] == 1
    first = res["idx"][flagged, 0]
    stats = lambda t: {"median": float(np.median(t)), "min": float(min(t)),
                       "max": float(max(t))}
    print(json.dumps({
        "n_queries": M, "n_corpus": N, "n_trees": T, "k": k,
        "n_nodes": int(len(det.feat)),
        "largest_tree": int(np.diff(det.tree_off).max()),
        "reps": args.reps, "torch_chunk": args.chunk,
        "leaves_s": stats(t_leaves), "fused_s": stats(t_fused),
        "torch_s": stats(t_torch), "equal": equal,
        "comparisons": M * N * T,
        "comparisons_per_s": M * N * T / float(np.median(t_fused)),
        "stage_wall_s": round(t_stage, 4),
        "predicted_flaky": int(flagged.sum()),
        "first_neighbour_flaky": int(
            res["corpus_labels"][first[first >= 0]].sum()),
    }))


if __name__ == "__main__":
    main()
