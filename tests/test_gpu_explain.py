"""GPU tests for explain: the detector_shap.hip kernels against the numpy
reference bit for bit on hand-built detectors (consistent counts, 16-element
paths, interval edges), and on hip-fitted detectors."""

import numpy as np
import pytest
import torch

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.constants import FLAKEFLAGGER_COLUMNS
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
from flake16_framework_amd.models.binning import bin_codes
from flake16_framework_amd.models.forest_ref import Tree, canonicalize_tree
from flake16_framework_amd.preprocess import transform_preprocessing

pytestmark = pytest.mark.gpu

M_POOL = 257          # > one 256-thread block; 63 and 1 are prefixes
CHAIN_DEPTH = 24
ONE_CUT, MANY_CUTS, CONST_COL = 0, 1, 2   # feature roles
SPINE_ROW = 0         # the pool row that reaches the end of the long path


# -- detector builder (local to this file) -----------------------------------
def _params(F, spec, rng):
    p = {"spec": spec, "mean": np.zeros(F), "scale": np.ones(F),
         "pca_mean": np.zeros(F), "W": np.eye(F)}
    if spec is not None:
        p["mean"] = rng.uniform(-20.0, 20.0, size=F)
        p["scale"] = rng.uniform(0.05, 30.0, size=F)
        p["scale"][CONST_COL] = 1.0
    if spec == "scale+pca":
        p["pca_mean"] = rng.randn(F) * 1e-3
        q, _ = np.linalg.qr(rng.randn(F, F))
        p["W"] = q
    return p


def _pool(F, params, rng):
    X = rng.randn(M_POOL, F) * rng.uniform(0.5, 40.0, size=F)
    X[:, CONST_COL] = 3.5 if params["spec"] is None \
        else params["mean"][CONST_COL]
    return X


def _cuts_from(T32, rng):
    """Cuts taken from the transformed inputs; each column's extremes stay
    outside the cuts, the 255-cut column reaches code 255."""
    cuts = []
    for f in range(T32.shape[1]):
        vals = np.unique(T32[:, f])
        inner = vals[1:-1] if len(vals) >= 3 else vals[:1]
        if f == ONE_CUT:
            c = inner[len(inner) // 2:len(inner) // 2 + 1]
        elif f == MANY_CUTS:
            c = inner[:255]
        else:
            k = min(len(inner), int(rng.randint(1, 40)))
            c = np.sort(rng.choice(inner, size=k, replace=False))
        cuts.append(np.ascontiguousarray(c, dtype=np.float32))
    return cuts


# A tree is ("leaf", cnt0, cnt1) or (feature, split, left, right); internal
# counts are summed bottom-up from the leaves.
def _tree(desc):
    rows = []

    def add(d):
        i = len(rows)
        rows.append(None)
        if d[0] == "leaf":
            rows[i] = [-1, 0, -1, -1, float(d[1]), float(d[2])]
            return i
        rt, lt = add(d[3]), add(d[2])       # right subtree first
        rows[i] = [d[0], d[1], lt, rt, rows[lt][4] + rows[rt][4],
                   rows[lt][5] + rows[rt][5]]
        return i

    add(desc)
    a = np.array(rows, dtype=np.float64)
    return canonicalize_tree(Tree(
        a[:, 0].astype(np.int32), a[:, 1].astype(np.int32),
        np.zeros(len(a), dtype=np.float32), a[:, 2].astype(np.int32),
        a[:, 3].astype(np.int32), a[:, 4].copy(), a[:, 5].copy()))


def _leaf(rng):
    c0, c1 = (int(v) for v in rng.randint(0, 50, size=2))
    return ("leaf", c0, c1 if c0 + c1 else 3)


def _pool_split(codes, f, rng):
    """A split some pool row's code equals."""
    return int(codes[rng.randint(len(codes)), f])


def _random_desc(codes, rng, depth=0, max_depth=6):
    if depth == max_depth or (depth > 0 and rng.rand() < 0.25):
        return _leaf(rng)
    f = int(rng.randint(codes.shape[1])) if depth else MANY_CUTS
    s = _pool_split(codes, f, rng) if depth else 127
    return (f, s, _random_desc(codes, rng, depth + 1, max_depth),
            _random_desc(codes, rng, depth + 1, max_depth))


def _chain_desc(rng):
    desc = _leaf(rng)
    for d in range(CHAIN_DEPTH - 1, -1, -1):
        desc = (MANY_CUTS, 10 * d, _leaf(rng), desc)
    return desc


def _spine_desc(codes, rng):
    """One long path through every feature and then some of them again,
    taking at every split the side pool row SPINE_ROW takes; the other
    child is a leaf."""
    F = codes.shape[1]
    perm = [int(f) for f in rng.permutation(F)]
    feats = perm + [perm[1], perm[F - 1], perm[1], MANY_CUTS]
    steps = []
    for f in feats:
        s = _pool_split(codes, f, rng)
        steps.append((f, s, int(codes[SPINE_ROW, f]) > s))
    desc = _leaf(rng)
    for f, s, right in reversed(steps):
        desc = (f, s, _leaf(rng), desc) if right else (f, s, desc, _leaf(rng))
    return desc


def _hand_built(F, spec, n_trees, seed):
    from flake16_framework_amd.engine.detector import assemble_detector
    rng = np.random.RandomState(seed)
    params = _params(F, spec, rng)
    X = _pool(F, params, rng)
    T32 = transform_preprocessing(X, params).astype(np.float32)
    cuts = _cuts_from(T32, rng)
    codes = bin_codes(T32, cuts)
    trees = []
    for t in range(n_trees):
        if n_trees == 1 or (t % 3 == 2 and (t // 3) % 2 == 1):
            trees.append(_tree(_spine_desc(codes, rng)))
        elif t % 3 == 0:
            trees.append(_tree(_random_desc(codes, rng)))
        elif t % 3 == 1:
            trees.append(_tree(_leaf(rng)))
        else:
            trees.append(_tree(_chain_desc(rng)))
    cols = tuple(range(16)) if F == 16 else FLAKEFLAGGER_COLUMNS
    det = assemble_detector(
        ("NOD", "Flake16" if F == 16 else "FlakeFlagger", "None", "None",
         "Random Forest"), 2, cols, params, cuts, trees, n_trees, 0, M_POOL)
    return det, X, codes


def _as_tests(X, cols, m):
    rows = {}
    for i in range(m):
        full = [float(-1000 - i)] * 16
        for j, c in enumerate(cols):
            full[c] = float(X[i, j])
        rows[f"t{i:04d}"] = [0, 0, *full]
    return {"proj": rows}


def _check_edges(det, paths, codes, F, n_trees):
    """The inputs do hit the edges this test is about."""
    n_el = np.diff(paths.leaf_off)
    leaf_of = np.repeat(np.arange(paths.n_leaves), n_el)
    c = codes[:, paths.feature].astype(np.int64)            # [M, E]
    lo, hi = paths.lo.astype(np.int64), paths.hi.astype(np.int64)
    assert (c == hi).any() and (c == lo).any()
    assert (c == 0).any() and (c == 255).any()
    hot = (c > lo) & (c <= hi)
    n_hot = np.zeros((len(codes), paths.n_leaves), dtype=np.int64)
    np.add.at(n_hot.T, leaf_of, hot.T)
    longest = n_el.max()
    assert (n_hot[:, n_el == longest] == longest).any()     # all-hot
    assert (n_hot[:, n_el >= 1] == 0).any()                 # all-cold
    assert ((n_hot > 0) & (n_hot < n_el)).any()             # and mixed
    assert longest == F                 # a leaf with F elements: 16 registers
    # consistent counts: children sum to their parent, every cover > 0
    internal = np.flatnonzero(det.feat >= 0)
    base = np.repeat(det.tree_off[:-1], np.diff(det.tree_off))
    lt = det.left[internal] + base[internal]
    for cnt in (det.cnt0, det.cnt1):
        np.testing.assert_array_equal(cnt[internal], cnt[lt] + cnt[lt + 1])
    assert (det.cnt0 + det.cnt1 > 0).all()
    if n_trees >= 7:
        assert (np.diff(det.tree_off) == 1).any()           # a root leaf
        assert (np.diff(det.tree_off) == 2 * CHAIN_DEPTH + 1).any()
        assert len(np.unique(n_el)) > 3


@pytest.mark.parametrize("n_trees", [1, 7, 23])
@pytest.mark.parametrize("spec", [None, "scale+pca"])
@pytest.mark.parametrize("F", [16, 7])
def test_kernel_bitwise_on_hand_built(F, spec, n_trees):
    from flake16_framework_amd.engine.detector import FPAD, device_inputs
    from flake16_framework_amd.engine.explain import (
        device_shap, device_table, explain,
    )
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    det, X, codes = _hand_built(F, spec, n_trees, seed=100 * F + n_trees)
    paths = build_merged_paths(det)
    _check_edges(det, paths, codes, F, n_trees)

    want = explain(det, tests=_as_tests(X, det.feature_cols, M_POOL),
                   backend="ref")          # rows are independent: prefixes
    assert np.ptp(want["phi"], axis=0).max() > 1e-3     # not constant
    gap = want["base_value"] + want["phi"].sum(axis=1) - want["proba"]
    assert np.abs(gap).max() <= 1e-9

    for m in (1, 63, M_POOL):
        got = explain(det, tests=_as_tests(X, det.feature_cols, m),
                      backend="hip")
        assert got["phi"].dtype == np.float64 and got["phi"].shape == (m, F)
        np.testing.assert_array_equal(got["phi"], want["phi"][:m])
        assert got["base_value"] == want["base_value"]
        np.testing.assert_array_equal(got["proba"], want["proba"][:m])
        np.testing.assert_array_equal(got["pred"], want["pred"][:m])
        assert got["feature_names"] == want["feature_names"]

        d = device_inputs(det, X[:m])
        dev_codes = ops.detect_encode(
            d["X64"], d["mean"], d["scale"], d["pca_mean"], d["W"],
            d["has_pca"], d["cuts"], d["cut_off"], d["F"])
        raw = device_shap(ops, dev_codes,
                          device_table(paths, dev_codes.device), n_trees, F)
        assert raw.dtype == torch.float64 and tuple(raw.shape) == (m, FPAD)
        raw = raw.cpu().numpy()
        np.testing.assert_array_equal(raw[:, :F], want["phi"][:m])
        assert (raw[:, F:] == 0.0).all()


def test_forest_of_root_leaves():
    """No path elements at all: an empty element table reaches the op."""
    from flake16_framework_amd.engine.detector import assemble_detector
    from flake16_framework_amd.engine.explain import explain
    det, X, _ = _hand_built(7, "scale+pca", 1, seed=3)
    rng = np.random.RandomState(4)
    flat = assemble_detector(
        det.config_keys, 2, tuple(det.feature_cols),
        det.preprocessing_params(), det.cut_list(),
        [_tree(_leaf(rng)) for _ in range(3)], 3, 0, M_POOL)
    tests = _as_tests(X, flat.feature_cols, 63)
    want = explain(flat, tests=tests, backend="ref")
    got = explain(flat, tests=tests, backend="hip")
    assert got["phi"].shape == (63, 7) and (got["phi"] == 0.0).all()
    np.testing.assert_array_equal(got["proba"], want["proba"])
    assert got["base_value"] == want["base_value"] == want["proba"][0]


def test_rows_in_two_chunks():
    """The op bounds its [T, 16, rows] workspace at 256 MiB; with 8192
    trees that is 256 rows per chunk, so 257 rows take two chunks.  Most
    of the trees are root leaves to keep the forest small."""
    from flake16_framework_amd.engine.detector import assemble_detector
    from flake16_framework_amd.engine.explain import explain
    n_trees = 8192
    det, X, _ = _hand_built(16, None, 23, seed=77)
    rng = np.random.RandomState(78)
    trees = det.trees() + [_tree(_leaf(rng)) for _ in range(n_trees - 23)]
    big = assemble_detector(
        det.config_keys, 2, tuple(det.feature_cols),
        det.preprocessing_params(), det.cut_list(), trees, n_trees, 0,
        M_POOL)
    tests = _as_tests(X, big.feature_cols, M_POOL)
    want = explain(big, tests=tests, backend="ref")
    got = explain(big, tests=tests, backend="hip")
    np.testing.assert_array_equal(got["phi"], want["phi"])
    np.testing.assert_array_equal(got["proba"], want["proba"])
    assert got["base_value"] == want["base_value"]
    assert np.ptp(want["phi"][255:], axis=0).max() > 0   # rows 255, 256 differ


def test_op_refuses_malformed_table():
    from flake16_framework_amd.engine.explain import device_shap, device_table
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    det, X, codes = _hand_built(16, None, 7, seed=5)
    paths = build_merged_paths(det)
    dev = torch.device("cuda:0")
    pad = np.zeros((4, 16), dtype=np.uint8)
    dev_codes = torch.from_numpy(pad).to(dev)
    table = device_table(paths, dev)
    device_shap(ops, dev_codes, table, 7, 16)
    with pytest.raises(RuntimeError):       # an element names feature >= F
        device_shap(ops, dev_codes, table, 7, 7)
    bad = dict(table, leaf_off=table["leaf_off"].clone())
    bad["leaf_off"][1] = paths.n_elements + 5
    with pytest.raises(RuntimeError):       # offsets step back / too far
        device_shap(ops, dev_codes, bad, 7, 16)
    with pytest.raises(RuntimeError):       # tree count against the ranges
        device_shap(ops, dev_codes, table, 6, 16)
    with pytest.raises(RuntimeError):       # dtype
        device_shap(ops, dev_codes,
                    dict(table, elem_z=table["elem_z"].float()), 7, 16)


@pytest.fixture(scope="module")
def train_tests():
    return make_synthetic_tests(n_tests=300, seed=2)


@pytest.fixture(scope="module")
def other_tests():
    return make_synthetic_tests(n_tests=257, seed=5)


@pytest.mark.parametrize("keys", [
    SHAP_CONFIGS[0], SHAP_CONFIGS[1],
    ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN", "Random Forest"),
], ids=["nod", "od", "pca-flakeflagger"])
def test_fitted_equal_across_backends(keys, train_tests, other_tests):
    from flake16_framework_amd.engine.detector import fit_detector
    from flake16_framework_amd.engine.explain import explain
    det = fit_detector(keys, tests=train_tests, backend="hip", n_trees=12)
    want = explain(det, tests=other_tests, backend="ref")
    got = explain(det, tests=other_tests, backend="hip")
    assert got["phi"].shape == (257, det.n_features)
    np.testing.assert_array_equal(got["phi"], want["phi"])
    assert got["base_value"] == want["base_value"]
    np.testing.assert_array_equal(got["proba"], want["proba"])
    np.testing.assert_array_equal(got["pred"], want["pred"])
    gap = got["base_value"] + got["phi"].sum(axis=1) - got["proba"]
    assert np.abs(gap).max() <= 1e-9
    assert np.ptp(got["phi"], axis=0).max() > 1e-3
