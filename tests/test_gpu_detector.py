"""GPU tests for fit / detect: the detect.hip kernels against the numpy
reference bit for bit on hand-built detectors, and hip-fitted against
ref-fitted detectors array for array."""

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


def _params(F, spec, rng):
    p = {"spec": spec, "mean": np.zeros(F), "scale": np.ones(F),
         "pca_mean": np.zeros(F), "W": np.eye(F)}
    if spec is not None:
        p["mean"] = rng.uniform(-20.0, 20.0, size=F)
        p["scale"] = rng.uniform(0.05, 30.0, size=F)
        p["scale"][CONST_COL] = 1.0          # zero-variance column
    if spec == "scale+pca":
        p["pca_mean"] = rng.randn(F) * 1e-3
        q, _ = np.linalg.qr(rng.randn(F, F))
        p["W"] = q
    return p


def _pool(F, params, rng):
    X = rng.randn(M_POOL, F) * rng.uniform(0.5, 40.0, size=F)
    X[:, CONST_COL] = 3.5
    if params["spec"] is not None:
        X[:, CONST_COL] = params["mean"][CONST_COL]
    return X


def _cuts_from(T32, rng):
    """Cuts taken FROM the transformed inputs, so inputs equal cut values
    exactly; each column's extremes stay outside the cuts."""
    cuts = []
    for f in range(T32.shape[1]):
        vals = np.unique(T32[:, f])
        inner = vals[1:-1] if len(vals) >= 3 else vals[:1]
        if f == ONE_CUT:
            c = inner[len(inner) // 2:len(inner) // 2 + 1]
        elif f == MANY_CUTS:
            assert len(inner) >= 255
            c = inner[:255]
        else:
            k = min(len(inner), int(rng.randint(1, 40)))
            c = np.sort(rng.choice(inner, size=k, replace=False))
        cuts.append(np.ascontiguousarray(c, dtype=np.float32))
    return cuts


class _Builder:
    """Collects nodes in creation order (NOT canonical: children are
    allocated depth-first and far from their siblings)."""

    def __init__(self):
        self.rows = []

    def node(self):
        self.rows.append([-1, 0, -1, -1, 0.0, 0.0])
        return len(self.rows) - 1

    def tree(self):
        a = np.array(self.rows, dtype=np.float64)
        return canonicalize_tree(Tree(
            a[:, 0].astype(np.int32), a[:, 1].astype(np.int32),
            np.zeros(len(a), dtype=np.float32), a[:, 2].astype(np.int32),
            a[:, 3].astype(np.int32), a[:, 4].copy(), a[:, 5].copy()))


def _leaf_counts(rng):
    c0, c1 = (float(v) for v in rng.randint(0, 50, size=2))
    if c0 + c1 == 0:
        c1 = 3.0
    return c0, c1


def _random_tree(n_cut, rng, max_depth=6):
    b = _Builder()

    def grow(depth):
        i = b.node()
        if depth == max_depth or (depth > 0 and rng.rand() < 0.25):
            b.rows[i][4:6] = _leaf_counts(rng)
            return i
        f = int(rng.randint(len(n_cut))) if depth else MANY_CUTS
        b.rows[i][0] = f
        b.rows[i][1] = int(rng.randint(0, n_cut[f] + 1)) if depth else 127
        b.rows[i][3] = grow(depth + 1)       # right subtree first
        b.rows[i][2] = grow(depth + 1)
        b.rows[i][4:6] = (1.0, 1.0)
        return i

    grow(0)
    return b.tree()


def _root_leaf_tree(rng):
    b = _Builder()
    b.rows[b.node()][4:6] = (4.0, 3.0)
    return b.tree()


def _chain_tree(n_cut, rng):
    """Degenerate chain on the 255-cut feature: level d sends
    code <= 10 d to a leaf and everything else one level down."""
    b = _Builder()
    node = b.node()
    for d in range(CHAIN_DEPTH):
        leaf, nxt = b.node(), b.node()
        b.rows[leaf][4:6] = _leaf_counts(rng)
        b.rows[node][:4] = [MANY_CUTS, 10 * d, leaf, nxt]
        b.rows[node][4:6] = (1.0, 1.0)
        node = nxt
    b.rows[node][4:6] = _leaf_counts(rng)
    return b.tree()


def _hand_built(F, spec, n_trees, seed):
    from flake16_framework_amd.engine.detector import assemble_detector
    rng = np.random.RandomState(seed)
    params = _params(F, spec, rng)
    X = _pool(F, params, rng)
    T32 = transform_preprocessing(X, params).astype(np.float32)
    cuts = _cuts_from(T32, rng)
    n_cut = [len(c) for c in cuts]
    trees = []
    for t in range(n_trees):
        kind = t % 3
        if kind == 0:
            trees.append(_random_tree(n_cut, rng))
        elif kind == 1:
            trees.append(_root_leaf_tree(rng))
        else:
            trees.append(_chain_tree(n_cut, rng))
    cols = tuple(range(16)) if F == 16 else FLAKEFLAGGER_COLUMNS
    det = assemble_detector(
        ("NOD", "Flake16" if F == 16 else "FlakeFlagger", "None", "None",
         "Random Forest"), 2, cols, params, cuts, trees, n_trees, 0, M_POOL)
    return det, X, T32


def _as_tests(X, cols, m):
    """tests.json rows; unselected columns hold junk that must be ignored."""
    rows = {}
    for i in range(m):
        full = [float(-1000 - i)] * 16
        for j, c in enumerate(cols):
            full[c] = float(X[i, j])
        rows[f"t{i:04d}"] = [0, 0, *full]
    return {"proj": rows}


@pytest.mark.parametrize("n_trees", [1, 7, 23])
@pytest.mark.parametrize("spec", [None, "scale", "scale+pca"])
@pytest.mark.parametrize("F", [16, 7])
def test_kernels_bitwise_on_hand_built(F, spec, n_trees):
    from flake16_framework_amd.engine.detector import (
        FPAD, detect, encode_inputs,
    )
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    dev = torch.device("cuda:0")
    det, X, T32 = _hand_built(F, spec, n_trees, seed=100 * F + n_trees)

    # the inputs do hit the edges this test is about
    ref_codes = bin_codes(T32, det.cut_list())
    n_cut = np.diff(det.cut_off)[:F]
    assert n_cut[ONE_CUT] == 1 and n_cut[MANY_CUTS] == 255
    assert det.scale[CONST_COL] == 1.0
    for f in range(F):
        cf = det.cut_list()[f]
        assert np.isin(T32[:, f], cf).any(), f          # equal to a cut
        if len(np.unique(T32[:, f])) >= 3:
            assert (T32[:, f] < cf[0]).any(), f         # below the smallest
            assert (T32[:, f] > cf[-1]).any(), f        # above the largest
    assert ref_codes[:, MANY_CUTS].max() == 255
    if n_trees >= 3:
        depth_reached = (ref_codes[:, MANY_CUTS].astype(int) - 1) // 10
        assert depth_reached.max() >= 20
        assert (np.diff(det.tree_off) == 1).any()       # a root that is a leaf

    for m in (1, 63, M_POOL):
        X64 = np.zeros((m, FPAD))
        X64[:, :F] = X[:m]
        mean, scale, pca_mean, W = (torch.from_numpy(a)
                                    for a in encode_inputs(det))
        codes = ops.detect_encode(
            torch.from_numpy(X64).to(dev), mean, scale, pca_mean, W,
            spec == "scale+pca", torch.from_numpy(det.cuts),
            torch.from_numpy(det.cut_off), F).cpu().numpy()
        np.testing.assert_array_equal(codes[:, :F], ref_codes[:m])
        assert (codes[:, F:] == 0).all()

        tests = _as_tests(X, det.feature_cols, m)
        want = detect(det, tests=tests, backend="ref")
        got = detect(det, tests=tests, backend="hip")
        np.testing.assert_array_equal(got["proba"], want["proba"])
        np.testing.assert_array_equal(got["pred"], want["pred"])
        assert got["proba"].dtype == np.float64
        assert list(got["nodeids"]) == list(want["nodeids"])
    if n_trees >= 3:
        assert len(np.unique(want["proba"])) > 10       # not a constant forest


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
def test_fit_equal_across_backends(keys, train_tests, other_tests):
    from flake16_framework_amd.engine.detector import detect, fit_detector
    ref = fit_detector(keys, tests=train_tests, backend="ref", n_trees=12)
    hip = fit_detector(keys, tests=train_tests, backend="hip", n_trees=12)
    a, b = hip.arrays(), ref.arrays()
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].dtype == b[name].dtype, name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)

    want = detect(ref, tests=other_tests, backend="ref")
    got = detect(hip, tests=other_tests, backend="hip")
    assert len(got["proba"]) == 257
    np.testing.assert_array_equal(got["proba"], want["proba"])
    np.testing.assert_array_equal(got["pred"], want["pred"])


@pytest.mark.parametrize("spec", [None, "scale+pca"])
def test_ops_agree_on_one_input(spec):
    """The ops that share the encode, tree-walk and rule steps, pinned to
    each other on one input: 130 rows (two 64-row blocks and a tail of 2)
    in three groups of 64, 0 and 66 rows, F = 7, 11 trees (two tree blocks,
    the second short).  Every group is served by a copy of one detector;
    a different detector stands in front of the three copies in the stacked
    arrays, so every row that matters is reached through non-zero
    parameter, cut and root offsets.  The grouped encode and sums take one
    group per stacked detector, so there the dummy owns a leading group
    without rows."""
    from flake16_framework_amd.engine.dependence import partial_dependence
    from flake16_framework_amd.engine.detector import device_inputs
    from flake16_framework_amd.engine.holdout import (
        grouped_acc, grouped_inputs,
    )
    from flake16_framework_amd.engine.importance import permuted_counts
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    F, n_trees, M = 7, 11, 130
    det, X, _ = _hand_built(F, spec, n_trees, seed=31)
    dummy, _, _ = _hand_built(F, spec, n_trees, seed=32)
    assert not np.array_equal(dummy.cuts[:8], det.cuts[:8])
    X = X[:M]
    i32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int32))
    seg3, seg4 = [0, 64, 64, M], [0, 0, 64, 64, M]

    one = device_inputs(det, X)
    stacked = grouped_inputs([dummy, det, det, det], X, seg4)
    dev = one["X64"].device

    # encode and sums: single detector against the grouped kernels
    codes = ops.detect_encode(one["X64"], one["mean"], one["scale"],
                              one["pca_mean"], one["W"], one["has_pca"],
                              one["cuts"], one["cut_off"], F)
    g_codes = ops.holdout_encode(
        stacked["X64"], stacked["seg_off"], stacked["mean"],
        stacked["scale"], stacked["pca_mean"], stacked["W"],
        stacked["has_pca"], stacked["cuts"], stacked["cut_off"], F)
    assert torch.equal(codes, g_codes)
    assert len(torch.unique(codes, dim=0)) > M // 2
    acc = ops.forest_proba(codes, one["tree_off"], one["nodes"], n_trees)
    assert torch.equal(acc, grouped_acc(ops, stacked))
    acc_np = acc.cpu().numpy()
    assert len(np.unique(acc_np[:, 1])) > 10

    # ICE: a job that writes row 0's own value back leaves its acc1 alone
    grouped_one = grouped_inputs([det], X, seg3)
    _, _, ice = partial_dependence(
        ops, grouped_one, i32(range(F)),
        torch.from_numpy(np.ascontiguousarray(X[0], dtype=np.float64)),
        want_ice=True)
    np.testing.assert_array_equal(ice[:, 0].cpu().numpy(),
                                  np.full(F, acc_np[0, 1]))

    # ICE of a job that does change codes: another row's value in the
    # 255-cut column, against encode + sums of the explicitly edited rows
    X_edit = X.copy()
    X_edit[:, MANY_CUTS] = X[77, MANY_CUTS]
    edited = device_inputs(det, X_edit)
    codes_edit = ops.detect_encode(
        edited["X64"], one["mean"], one["scale"], one["pca_mean"], one["W"],
        one["has_pca"], one["cuts"], one["cut_off"], F)
    assert int((codes_edit != codes).any(dim=1).sum()) > M // 2
    acc_edit = ops.forest_proba(codes_edit, one["tree_off"], one["nodes"],
                                n_trees)
    assert not torch.equal(acc_edit, acc)
    _, _, ice = partial_dependence(
        ops, grouped_one, i32([MANY_CUTS]),
        torch.tensor([X[77, MANY_CUTS]], dtype=torch.float64),
        want_ice=True)
    assert torch.equal(ice[0], acc_edit[:, 1])

    # the identity permutation changes nothing, whatever the mask
    labels = torch.from_numpy(
        np.random.RandomState(5).randint(0, 2, size=M).astype(np.uint8)
    ).to(dev)
    assert 0 < int(labels.sum()) < M
    threshold = 0.5
    curve, argmax = ops.threshold_counts(
        acc, labels, i32(seg3), n_trees, torch.tensor([threshold],
                                                      dtype=torch.float64))
    three = dict(stacked, seg_off=i32(seg3))
    for thr, want in ((None, argmax), (threshold, curve[:, 0])):
        counts, baseline = permuted_counts(
            ops, three, labels, i32([1, 2, 3]), i32(np.arange(M)[None]),
            i32([1, 1 << (F - 1), (1 << F) - 1]), thr)
        assert int(want.sum()) > 0
        assert torch.equal(baseline, want)
        for j in range(3):
            assert torch.equal(counts[j, 0], baseline)

    # leaves: each tree's leaf record gives the term forest_proba sums
    leaves = ops.forest_leaves(codes, one["tree_off"], one["nodes"],
                               n_trees).cpu().numpy()
    nodes = one["nodes"].cpu().numpy()
    for t in range(n_trees):
        rec = nodes[det.tree_off[t] + leaves[:, t]]
        assert (rec[:, 0] >= 0).all()                   # leaves, not splits
        c = rec.view(np.float32).astype(np.float64)
        term = ops.forest_proba(codes, one["tree_off"][t:t + 2],
                                one["nodes"], 1).cpu().numpy()
        np.testing.assert_array_equal(term, c / c.sum(axis=1, keepdims=True))
