"""explain: per-test TreeSHAP attributions for a saved detector.

`detect` says how likely a test is flaky; `explain` splits that probability
into one additive contribution per model input plus the detector's base
value (its expected output under the training covers):

    proba[i] == base_value + sum_f phi[i, f]        (up to rounding)

Conventions
  - Values are for the FLAKY class, class 1, with leaf value
    cnt1 / (cnt0 + cnt1): the quantity `detect` reports.  shap.pkl (the
    `shap` stage, reference experiment.py:504-530) stores class-0 values,
    i.e. the negation.
  - For a scale+pca detector the model's inputs are principal components;
    attributions are for those inputs, named pc0..pc{F-1}.  Otherwise the
    names are constants.FEATURE_NAMES[feature_cols].

The algorithm is path-dependent TreeSHAP over MERGED leaf paths
(models/mergedpaths.py): at most 16 elements per path, no UNWIND along it.

Pinned arithmetic (the contract ops/hip/detector_shap.hip reproduces bit
for bit; fp64, no fused multiply-add, every expression left to right):
  per (leaf, row)
    start from the sentinel (w[0] = 1), EXTEND with each element in table
    order, o in {0.0, 1.0} from the interval test, as treeshap_ref._extend:
        w[i+1] += po * w[i] * (i+1) / (l+1)
        w[i]    = pz * w[i] * (l-i) / (l+1)
    then per element i >= 1 the term
        unwound_sum(i) * (o_i - z_i) * v
    with unwound_sum as treeshap_ref._unwound_sum;
  phi[row, f]
    a tree's sum starts at 0.0 and adds terms leaf by leaf (ascending),
    element by element; tree sums are added sequentially within blocks of
    PREDICT_TREE_BLOCK trees from 0.0, blocks in ascending order, and the
    total is divided by n_trees — forest_ref.accumulate_proba's association;
  base_value
    per leaf (product of z in table order, from 1.0) * v, summed in the
    same leaf / tree / block association, divided by n_trees; computed on
    the host for both backends.
"""

import json
from typing import NamedTuple

import numpy as np

from ..constants import EXPLANATIONS_FILE, FEATURE_NAMES
from ..dataset.tests_io import load_tests
from ..models.binning import bin_codes
from ..models.forest_ref import PREDICT_TREE_BLOCK, accumulate_proba
from ..models.mergedpaths import build_merged_paths
from ..preprocess import transform_preprocessing
from .detector import _resolve_backend, device_inputs, load_rows


def feature_names(detector):
    if detector.preproc == "scale+pca":
        return tuple(f"pc{k}" for k in range(detector.n_features))
    return tuple(FEATURE_NAMES[int(c)] for c in detector.feature_cols)


def _blocked_tree_sum(tree_sums):
    """Per-tree values (scalars or row vectors) summed in the
    PREDICT_TREE_BLOCK association."""
    total = 0.0 * tree_sums[0]
    for b in range(0, len(tree_sums), PREDICT_TREE_BLOCK):
        blk = 0.0 * tree_sums[0]
        for s in tree_sums[b:b + PREDICT_TREE_BLOCK]:
            blk = blk + s
        total = total + blk
    return total


def base_value(detector, paths):
    """The detector's expected class-1 output: every leaf's value weighted
    by the cover fraction that reaches it."""
    z, off = paths.z.tolist(), paths.leaf_off.tolist()
    value = paths.leaf_value.tolist()
    tree_sums = []
    for t in range(detector.n_trees):
        s = 0.0
        for leaf in range(paths.tree_leaf_off[t], paths.tree_leaf_off[t + 1]):
            p = 1.0
            for e in range(off[leaf], off[leaf + 1]):
                p = p * z[e]
            s = s + p * value[leaf]
        tree_sums.append(s)
    return float(_blocked_tree_sum(tree_sums) / detector.n_trees)


def _leaf_terms(codes, elems, v):
    """One leaf's terms for all rows: [(feature, float64[M])] in element
    order.  codes: int16 [M, F]."""
    m, n = codes.shape[0], len(elems)
    o = [((codes[:, f] > lo) & (codes[:, f] <= hi)).astype(np.float64)
         for f, lo, hi, _ in elems]
    w = np.zeros((n + 1, m))
    w[0] = 1.0
    for k, (_, _, _, pz) in enumerate(elems):
        l, po = k + 1, o[k]
        for i in range(l - 1, -1, -1):
            w[i + 1] += po * w[i] * (i + 1) / (l + 1)
            w[i] = pz * w[i] * (l - i) / (l + 1)

    l, lm = n + 1, n
    out = []
    for k, (f, _, _, z) in enumerate(elems):
        # hot form; (j + 1) * o[i] is j + 1 where it is selected
        total_hot = np.zeros(m)
        nx = w[lm].copy()
        for j in range(lm - 1, -1, -1):
            t = nx * l / (j + 1)
            total_hot += t
            nx = w[j] - t * z * (lm - j) / l
        total_cold = np.zeros(m)
        for j in range(lm - 1, -1, -1):
            total_cold += w[j] * l / (z * (lm - j))
        total = np.where(o[k] != 0.0, total_hot, total_cold)
        out.append((f, total * (o[k] - z) * v))
    return out


def shap_ref(detector, paths, codes):
    """float64 [M, F] class-1 attributions, numpy: vectorised over rows,
    one Python iteration per leaf."""
    codes = np.asarray(codes).astype(np.int16)
    m, F = codes.shape[0], detector.n_features
    value = paths.leaf_value.tolist()
    tree_sums = []
    with np.errstate(all="ignore"):     # the unselected form may overflow
        for t in range(detector.n_trees):
            s = np.zeros((m, F))
            for leaf in range(paths.tree_leaf_off[t],
                              paths.tree_leaf_off[t + 1]):
                for f, term in _leaf_terms(codes, paths.elements(leaf),
                                           value[leaf]):
                    s[:, f] += term
            tree_sums.append(s)
    return _blocked_tree_sum(tree_sums) / detector.n_trees


def pack_elements(paths):
    """int32 [E] element records (layout: ops/hip/detector_shap.hip)."""
    return (paths.feature.astype(np.int32)
            | ((paths.lo.astype(np.int32) + 1) << 8)
            | (paths.hi.astype(np.int32) << 20))


def device_table(paths, device=None):
    """The merged-path table as detector_shap's device tensors."""
    import torch

    device = device or torch.device("cuda")
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return {"tree_leaf_off": put(paths.tree_leaf_off),
            "leaf_off": put(paths.leaf_off),
            "leaf_val": put(paths.leaf_value),
            "elem_code": put(pack_elements(paths)),
            "elem_z": put(paths.z)}


def device_shap(ops, codes, table, n_trees, F):
    """The device hot path on resident codes: float64 [M, 16]."""
    return ops.detector_shap(codes, table["tree_leaf_off"],
                             table["leaf_off"], table["leaf_val"],
                             table["elem_code"], table["elem_z"], n_trees, F)


def explain_device(ops, detector, paths, X):
    """The device part of explain: (codes, path table, acc [M, 2],
    phi [M, 16]), all resident."""
    d = device_inputs(detector, X)
    codes = ops.detect_encode(d["X64"], d["mean"], d["scale"], d["pca_mean"],
                              d["W"], d["has_pca"], d["cuts"], d["cut_off"],
                              d["F"])
    acc = ops.forest_proba(codes, d["tree_off"], d["nodes"], d["n_trees"])
    table = device_table(paths, codes.device)
    phi = device_shap(ops, codes, table, detector.n_trees,
                      detector.n_features)
    return codes, table, acc, phi


class Explained(NamedTuple):
    """explain()'s result and what interact goes on from.  codes and phi
    are what the backend computed with: device tensors (phi [M, 16]) with
    the device path table for hip, host arrays (phi [M, F]) and no table
    for ref.  Without a test all three are None."""
    res: dict
    backend: str
    paths: object
    codes: object = None
    table: object = None
    phi: object = None


def _explain_hip(detector, paths, X):
    """(acc0, acc1, phi [M, F]) on the host, then the resident codes,
    table and phi [M, 16]."""
    from ..ops.backend import get_ops

    codes, table, acc, phi = explain_device(get_ops(), detector, paths, X)
    acc, phi_host = acc.cpu().numpy(), phi.cpu().numpy()
    return (acc[:, 0], acc[:, 1], phi_host[:, :detector.n_features],
            codes, table, phi)


def _explain_ref(detector, paths, X):
    """(acc0, acc1, phi [M, F]), then the codes, no table and phi again."""
    T = transform_preprocessing(X, detector.preprocessing_params())
    codes = bin_codes(T.astype(np.float32), detector.cut_list())
    acc0, acc1 = accumulate_proba(detector.trees(), codes)
    phi = shap_ref(detector, paths, codes)
    return acc0, acc1, phi, codes, None, phi


def input_rows(detector, tests=None, tests_file=None):
    """(X, projects, nodeids) of a tests.json, which may hold no test."""
    if tests is None:
        tests = load_tests(tests_file)
    if any(len(tests_proj) for tests_proj in tests.values()):
        return load_rows(detector, tests, None)
    # load_rows cannot shape an empty matrix
    none = np.array([], dtype=str)
    return np.zeros((0, detector.n_features)), none, none


def explain_more(detector, tests, tests_file, backend):
    """explain() as an Explained."""
    backend = _resolve_backend(backend)
    detector.validate()
    paths = build_merged_paths(detector)
    X, projects, nodeids = input_rows(detector, tests, tests_file)
    if len(X) == 0:
        acc0 = acc1 = np.zeros(0)
        phi, used = np.zeros((0, detector.n_features)), ()
    elif backend == "hip":
        acc0, acc1, phi, *used = _explain_hip(detector, paths, X)
    else:
        acc0, acc1, phi, *used = _explain_ref(detector, paths, X)
    res = {"proba": acc1 / detector.n_trees,
           "pred": (acc1 > acc0).astype(np.uint8),
           "projects": projects, "nodeids": nodeids,
           "phi": np.ascontiguousarray(phi, dtype=np.float64),
           "base_value": base_value(detector, paths),
           "feature_names": feature_names(detector)}
    return Explained(res, backend, paths, *used)


def explain(detector, tests=None, tests_file=None, backend="auto"):
    """detect() plus attributions for every test of a tests.json.

    Returns detect's "proba", "pred", "projects", "nodeids" and
    "phi" float64 [M, F], "base_value" float, "feature_names" tuple."""
    return explain_more(detector, tests, tests_file, backend).res


def write_explanations(detector, tests=None, tests_file=None,
                       out_file=EXPLANATIONS_FILE, backend="auto"):
    """explain() written as {"feature_names": [...], "base_value": b,
    "tests": {proj: {nodeid: [proba, pred, phi_0, ..., phi_{F-1}]}}}."""
    res = explain(detector, tests=tests, tests_file=tests_file,
                  backend=backend)
    out = {}
    for proj, nid, p, y, row in zip(res["projects"], res["nodeids"],
                                    res["proba"], res["pred"], res["phi"]):
        out.setdefault(str(proj), {})[str(nid)] = [
            float(p), int(y), *(float(x) for x in row)]
    with open(out_file, "w") as fd:
        json.dump({"feature_names": list(res["feature_names"]),
                   "base_value": res["base_value"], "tests": out},
                  fd, indent=4)
    return res
