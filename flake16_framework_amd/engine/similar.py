"""similar: the labelled tests a detector treats most like a new test.

`detect` says how flaky a test looks and `explain` which inputs said so;
neither says which KNOWN tests it looks like.  A forest answers that with
its proximity: two tests are alike to the degree that the trees send them
to the same leaves.  This stage ranks a labelled corpus (typically the
training file) by that measure for every test of a query file.

Definition.  Given a detector with T trees, M query rows and N corpus
rows, both encoded exactly as `detect` encodes them:

  leaf         leaf[i, t] is the tree-local canonical node id (Detector
               numbering, root 0) of the leaf that row i reaches in tree
               t; int32 [rows, T]
  shared       shared(q, c) = #{t : leafQ[q, t] == leafC[c, t]}, an
               integer in 0..T
  neighbours   for query q the first k corpus rows in the order (larger
               shared, then lower corpus index), after leaving out
               self_idx[q]; self_idx is int32 [M], -1 leaves nothing out
  output       idx int32 [M, k] and shared int32 [M, k]; where fewer than
               k candidates exist the remaining slots hold idx = -1,
               shared = 0
  limits       1 <= k <= MAX_K and T >= 1; N = 0 and M = 0 are legal

The order is total, so the result does not depend on tiling, on how the
corpus is split over workgroups, or on merge order: any partial top-k
merged under the same comparison gives the same answer.  Every output is
an integer, so the two backends agree exactly.  `backend="ref"` is numpy
(models.forest_ref._tree_leaves per tree, a chunked == and sum, a stable
argsort of -shared); `backend="hip"` runs detect_encode, forest_leaves on
both sides and the fused proximity_topk (ops/hip/similar.hip), which needs
no M x N memory.
"""

import json

import numpy as np

from ..constants import SIMILAR_FILE, TESTS_FILE
from ..dataset.tests_io import load_tests
from ..models.binning import bin_codes
from ..models.forest_ref import _tree_leaves, accumulate_proba
from ..preprocess import transform_preprocessing
from .detector import _resolve_backend, device_inputs, load_rows

MAX_K = 16
# the kernel's tiling (ops/hip/similar.hip), for tests that straddle it
PROX_TILE = 32       # corpus rows staged per LDS tile
PROX_CHUNK = 512     # corpus rows per workgroup (a multiple on huge grids)

_REF_CHUNK = 256     # query rows per block of the numpy comparison


def _rows(detector, tests):
    """load_rows that also shapes an empty file."""
    if any(len(tests_proj) for tests_proj in tests.values()):
        return load_rows(detector, tests, None)
    empty = np.array([], dtype=str)
    return np.zeros((0, detector.n_features)), empty, empty


def _codes_ref(detector, X):
    T = transform_preprocessing(X, detector.preprocessing_params())
    return bin_codes(T.astype(np.float32), detector.cut_list())


def leaves_ref(detector, codes):
    """int32 [rows, T] leaf ids of bin-code rows, numpy."""
    codes = np.asarray(codes, dtype=np.uint8)
    out = np.zeros((codes.shape[0], detector.n_trees), dtype=np.int32)
    if codes.shape[0]:
        for t, tree in enumerate(detector.trees()):
            out[:, t] = _tree_leaves(tree, codes)
    return out


def proximity_topk_ref(leaf_q, leaf_c, self_idx, k):
    """(idx, shared) int32 [M, k] by the module's definition, numpy."""
    leaf_q, leaf_c = np.asarray(leaf_q), np.asarray(leaf_c)
    M, N = len(leaf_q), len(leaf_c)
    idx = np.full((M, k), -1, dtype=np.int32)
    shared = np.zeros((M, k), dtype=np.int32)
    if N == 0:
        return idx, shared
    for a in range(0, M, _REF_CHUNK):
        b = min(M, a + _REF_CHUNK)
        s = np.zeros((b - a, N), dtype=np.int32)
        for t in range(leaf_q.shape[1]):
            s += leaf_q[a:b, t, None] == leaf_c[None, :, t]
        for q in range(a, b):
            row = s[q - a]
            if self_idx[q] >= 0:
                row[self_idx[q]] = -1
            order = np.argsort(-row, kind="stable")
            order = order[row[order] >= 0][:k]
            idx[q, :len(order)] = order
            shared[q, :len(order)] = row[order]
    return idx, shared


def _similar_ref(detector, Xq, Xc, self_idx, k):
    codes_q = _codes_ref(detector, Xq)
    if len(Xq):
        acc0, acc1 = accumulate_proba(detector.trees(), codes_q)
    else:
        acc0 = acc1 = np.zeros(0)
    idx, shared = proximity_topk_ref(
        leaves_ref(detector, codes_q),
        leaves_ref(detector, _codes_ref(detector, Xc)), self_idx, k)
    return acc0, acc1, idx, shared


def device_leaves(ops, d):
    """The tensors of detector.device_inputs -> (codes, leaf ids int32
    [rows, T]), both device-resident."""
    codes = ops.detect_encode(d["X64"], d["mean"], d["scale"], d["pca_mean"],
                              d["W"], d["has_pca"], d["cuts"], d["cut_off"],
                              d["F"])
    return codes, ops.forest_leaves(codes, d["tree_off"], d["nodes"],
                                    d["n_trees"])


def _similar_hip(detector, Xq, Xc, self_idx, k):
    import torch

    from ..ops.backend import get_ops

    ops = get_ops()
    dq = device_inputs(detector, Xq)
    X64c = np.zeros((Xc.shape[0], dq["X64"].shape[1]), dtype=np.float64)
    X64c[:, :detector.n_features] = Xc
    dc = dict(dq, X64=torch.from_numpy(X64c).to(dq["X64"].device))
    codes_q, leaf_q = device_leaves(ops, dq)
    _, leaf_c = device_leaves(ops, dc)
    acc = ops.forest_proba(codes_q, dq["tree_off"], dq["nodes"],
                           dq["n_trees"]).cpu().numpy()
    idx, shared = ops.proximity_topk(leaf_q, leaf_c,
                                     torch.from_numpy(self_idx), k)
    return acc[:, 0], acc[:, 1], idx.cpu().numpy(), shared.cpu().numpy()


def similar(detector, tests=None, tests_file=None, corpus=None, k=5,
            flaky_only=False, skip_self=True, backend="auto"):
    """The k nearest corpus tests, by forest proximity, of every test of a
    tests.json (file iteration order).

    corpus is a labelled tests.json-shaped dict or a file name (default:
    tests.json), typically the detector's training file; a corpus row is
    flaky when row[1] == detector.flaky_label.  flaky_only keeps only the
    flaky corpus rows as candidates; skip_self leaves out the corpus row
    with the query's own (project, nodeid), so a test queried against its
    own training file does not return itself.

    Returns detect's "proba", "pred", "projects", "nodeids", and "idx",
    "shared" int32 [M, k] (idx into the WHOLE corpus in file order, -1 / 0
    in unused slots), "corpus_projects", "corpus_nodeids", "corpus_labels"
    (bool) of the whole corpus, "n_candidates" (corpus rows compared),
    "k" and "n_trees"."""
    backend = _resolve_backend(backend)
    detector.validate()
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in 1..{MAX_K}")
    if tests is None:
        tests = load_tests(tests_file)
    if corpus is None or isinstance(corpus, str):
        corpus = load_tests(corpus or TESTS_FILE)

    Xq, projects, nodeids = _rows(detector, tests)
    Xc, c_projects, c_nodeids = _rows(detector, corpus)
    c_labels = np.array(
        [row[1] == detector.flaky_label for rows in corpus.values()
         for row in rows.values()], dtype=bool)

    keep = np.flatnonzero(c_labels) if flaky_only else np.arange(len(Xc))
    keep = keep.astype(np.int32)
    self_idx = np.full(len(Xq), -1, dtype=np.int32)
    if skip_self:
        where = {(str(c_projects[i]), str(c_nodeids[i])): j
                 for j, i in enumerate(keep)}
        for q, key in enumerate(zip(projects, nodeids)):
            self_idx[q] = where.get((str(key[0]), str(key[1])), -1)

    run = _similar_hip if backend == "hip" else _similar_ref
    acc0, acc1, idx, shared = run(detector, Xq, Xc[keep], self_idx, k)
    if len(keep):       # candidate positions -> rows of the whole corpus
        idx = np.where(idx >= 0, keep[np.maximum(idx, 0)], -1)
    return {"proba": acc1 / detector.n_trees,
            "pred": (acc1 > acc0).astype(np.uint8),
            "projects": projects, "nodeids": nodeids,
            "idx": np.ascontiguousarray(idx, dtype=np.int32),
            "shared": np.ascontiguousarray(shared, dtype=np.int32),
            "corpus_projects": c_projects, "corpus_nodeids": c_nodeids,
            "corpus_labels": c_labels, "n_candidates": int(len(keep)),
            "k": k, "n_trees": int(detector.n_trees)}


def write_similar(detector, tests=None, tests_file=None, corpus=None,
                  out_file=SIMILAR_FILE, **kwargs):
    """similar() written as {"k", "n_trees", "corpus_tests" (corpus rows
    compared), "tests": {proj: {nodeid: [proba, pred, [[corpus_proj,
    corpus_nodeid, label, shared], ...]]}}}.  Neighbours with shared == 0
    and unused slots are not written: their order carries no
    information."""
    res = similar(detector, tests=tests, tests_file=tests_file,
                  corpus=corpus, **kwargs)
    out = {}
    for q, (proj, nid) in enumerate(zip(res["projects"], res["nodeids"])):
        near = [[str(res["corpus_projects"][i]),
                 str(res["corpus_nodeids"][i]),
                 int(res["corpus_labels"][i]), int(s)]
                for i, s in zip(res["idx"][q], res["shared"][q])
                if i >= 0 and s > 0]
        out.setdefault(str(proj), {})[str(nid)] = [
            float(res["proba"][q]), int(res["pred"][q]), near]
    with open(out_file, "w") as fd:
        json.dump({"k": res["k"], "n_trees": res["n_trees"],
                   "corpus_tests": res["n_candidates"], "tests": out},
                  fd, indent=4)
    return res
