"""interact: SHAP interaction values for a saved detector.

`explain` gives every test one number per model input; a pair effect
("covered lines matter only when the run time is also high") is folded
into the two inputs' own numbers.  `interact` splits it back out: an
[F, F] matrix per test, the Shapley interaction index of Lundberg et al.
(`shap_interaction_values`), with explain's conventions (class 1, leaf
value cnt1 / cover, path-dependent expectation).  For g != f

    Phi[g, f] = sum over S subset of N \\ {g, f} of
                |S|! (F - |S| - 2)! / (2 (F - 1)!)
                * (v(S+g+f) - v(S+g) - v(S+f) + v(S))
    Phi[g, g] = phi[g] - sum_{f != g} Phi[g, f]

so every row of the matrix sums to explain's phi[g] and
base_value + sum_{g, f} Phi[g, f] == proba up to rounding.

A feature appears at most once in a merged leaf path
(models/mergedpaths.py), so conditioning on g is dropping its element.

Pinned arithmetic (the contract ops/hip/detector_shap.hip reproduces bit
for bit; fp64, no fused multiply-add, every expression left to right):
  per leaf with elements e_0..e_{n-1} and value v, per element c with
  feature g
    the reduced path is the same elements in table order without c; on it
    explain's per-element terms (explain._leaf_terms: EXTEND from the
    sentinel, then unwound_sum(k) * (o_k - z_k) * v); every remaining
    element k with feature f adds term_k * (o_c - z_c) to the tree's sum
    for (g, f);
  a tree's (g, f) sum starts at 0.0 and adds contributions with leaves
  ascending (within a leaf, remaining elements in table order); a leaf
  with one element contributes nothing;
  Phi[g, f], g != f
    tree sums combined in blocks of PREDICT_TREE_BLOCK as explain's phi,
    divided by n_trees, then multiplied by 0.5;
  Phi[g, g] = phi[g] - s
    phi[g] is explain's value and s adds Phi[g, f] for f ascending,
    skipping f = g, from 0.0.
The two triangles come from different reduced paths: Phi[g, f] and
Phi[f, g] agree to rounding, not bit for bit.
"""

import json

import numpy as np

from ..constants import INTERACTIONS_FILE
from .explain import _blocked_tree_sum, _leaf_terms, explain_more


def interactions_ref(detector, paths, codes, phi):
    """float64 [M, F, F] class-1 interaction values, numpy: vectorised
    over rows, one _leaf_terms call per (leaf, element).  phi is
    explain's [M, F]; the arithmetic is pinned in the module docstring."""
    codes = np.asarray(codes).astype(np.int16)
    m, F = codes.shape[0], detector.n_features
    value = paths.leaf_value.tolist()
    tree_sums = []
    with np.errstate(all="ignore"):     # the unselected form may overflow
        for t in range(detector.n_trees):
            s = np.zeros((m, F, F))
            for leaf in range(paths.tree_leaf_off[t],
                              paths.tree_leaf_off[t + 1]):
                elems = paths.elements(leaf)
                for c, (g, lo, hi, zc) in enumerate(elems):
                    oc = ((codes[:, g] > lo)
                          & (codes[:, g] <= hi)).astype(np.float64)
                    cond = oc - zc
                    for f, term in _leaf_terms(
                            codes, elems[:c] + elems[c + 1:], value[leaf]):
                        s[:, g, f] += term * cond
            tree_sums.append(s)
    out = _blocked_tree_sum(tree_sums) / detector.n_trees * 0.5
    for g in range(F):
        s = np.zeros(m)
        for f in range(F):
            if f != g:
                s = s + out[:, g, f]
        out[:, g, g] = phi[:, g] - s
    return out


def device_interactions(ops, codes, table, phi, n_trees, F):
    """The device hot path on resident codes and phi: float64
    [M, 16, 16]."""
    return ops.detector_shap_interactions(
        codes, table["tree_leaf_off"], table["leaf_off"], table["leaf_val"],
        table["elem_code"], table["elem_z"], phi, n_trees, F)


def interact(detector, tests=None, tests_file=None, backend="auto"):
    """explain() plus interaction values for every test of a tests.json.

    Returns explain's fields unchanged ("proba", "pred", "projects",
    "nodeids", "phi", "base_value", "feature_names") and "interactions",
    float64 [M, F, F]."""
    ex = explain_more(detector, tests, tests_file, backend)
    F = detector.n_features
    if len(ex.res["proba"]) == 0:
        inter = np.zeros((0, F, F))
    elif ex.backend == "hip":
        from ..ops.backend import get_ops

        inter = device_interactions(get_ops(), ex.codes, ex.table, ex.phi,
                                    detector.n_trees, F)
        inter = inter.cpu().numpy()[:, :F, :F]
    else:
        inter = interactions_ref(detector, ex.paths, ex.codes, ex.phi)
    return dict(ex.res,
                interactions=np.ascontiguousarray(inter, dtype=np.float64))


def pair_index(F):
    """The pairs g < f in ascending (g, f) order, int [P, 2]."""
    g, f = np.triu_indices(F, k=1)
    return np.stack([g, f], axis=1)


def pair_values(inter):
    """float64 [M, P]: Phi[g, f] + Phi[f, g] for the pairs of
    pair_index."""
    inter = np.asarray(inter, dtype=np.float64)
    pairs = pair_index(inter.shape[1])
    return inter[:, pairs[:, 0], pairs[:, 1]] \
        + inter[:, pairs[:, 1], pairs[:, 0]]


def rank_pairs(values):
    """Order of the last axis by larger |value|, then lower (g, f):
    indices into pair_index, same shape as `values`."""
    return np.argsort(-np.abs(values), axis=-1, kind="stable")


def top_pairs(inter, top):
    """Per test of an [M, F, F] array the first `top` pairs g < f as
    [g, f, Phi[g, f] + Phi[f, g]], by larger |value|, then lower (g, f)."""
    inter = np.asarray(inter, dtype=np.float64)
    pairs = pair_index(inter.shape[1]).tolist()
    values = pair_values(inter)
    return [[[*pairs[p], float(row[p])] for p in order]
            for row, order in zip(values, rank_pairs(values)[:, :top])]


def summarize(inter):
    """(mean_abs [F, F], pair_mean [P]) over the tests of an [M, F, F]
    array; zeros when there is no test."""
    inter = np.asarray(inter, dtype=np.float64)
    m, F = inter.shape[0], inter.shape[1]
    if m == 0:
        return np.zeros((F, F)), np.zeros(F * (F - 1) // 2)
    return np.abs(inter).mean(axis=0), np.abs(pair_values(inter)).mean(axis=0)


def write_interactions(detector, tests=None, tests_file=None,
                       out_file=INTERACTIONS_FILE, top=3, matrix_out=None,
                       backend="auto"):
    """interact() written as
        {"feature_names": [...], "base_value": b,
         "mean_abs": [[F x F]],      mean over tests of |Phi|
         "pairs": [[name_g, name_f, mean |Phi[g,f] + Phi[f,g]|], ...],
                                     all g < f, descending
         "tests": {proj: {nodeid: [proba, pred, [Phi[0,0], ...,
                   Phi[F-1,F-1]], [[g, f, Phi[g,f] + Phi[f,g]], ...]]}}}
    with the first `top` pairs of every test by larger |value|, then lower
    (g, f); "pairs" breaks ties the same way.  matrix_out saves the full
    [M, F, F] array as .npy."""
    F = detector.n_features
    n_pairs = F * (F - 1) // 2
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) \
            or not 0 <= top <= n_pairs:
        raise ValueError(f"interact: top takes 0..{n_pairs}")
    res = interact(detector, tests=tests, tests_file=tests_file,
                   backend=backend)
    inter, names = res["interactions"], res["feature_names"]
    pairs = pair_index(F).tolist()
    diag = np.diagonal(inter, axis1=1, axis2=2)
    out = {}
    for proj, nid, p, y, d, best in zip(
            res["projects"], res["nodeids"], res["proba"], res["pred"],
            diag, top_pairs(inter, top)):
        out.setdefault(str(proj), {})[str(nid)] = [
            float(p), int(y), [float(x) for x in d], best]
    mean_abs, pair_mean = summarize(inter)
    with open(out_file, "w") as fd:
        json.dump({"feature_names": list(names),
                   "base_value": res["base_value"],
                   "mean_abs": mean_abs.tolist(),
                   "pairs": [[names[pairs[p][0]], names[pairs[p][1]],
                              float(pair_mean[p])]
                             for p in rank_pairs(pair_mean)],
                   "tests": out}, fd, indent=4)
    if matrix_out is not None:
        with open(matrix_out, "wb") as fd:
            np.save(fd, inter)
    return res
