"""GPU tests for dependence: the fused partial_dependence op of
ops/hip/dependence.hip against the numpy definition, bit for bit in the
sums, the counts and the ICE values, on hand-built detectors; against the
existing ops on an explicitly overwritten matrix; the device backend of
dependence() against the ref backend; the op's host checks.  One test
needs no GPU: it shows from the numpy side alone that the pinned pairwise
block sum differs from a left-to-right sum on the very inputs the GPU
tests use, so a wrong reduction order cannot pass unnoticed."""

import functools
import json

import numpy as np
import pytest
import torch

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.constants import FLAKEFLAGGER_COLUMNS
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
from flake16_framework_amd.models.binning import bin_codes
from flake16_framework_amd.models.forest_ref import (
    Tree, accumulate_proba, canonicalize_tree,
)
from flake16_framework_amd.preprocess import transform_preprocessing

M_POOL = 257          # > one 256-thread block and > four 64-row blocks
CHAIN_DEPTH = 24
ONE_CUT, MANY_CUTS, CONST_COL = 0, 1, 2   # feature roles
# rows per group: the empty group first, in the middle, last
GROUP_ORDERS = [(0, 1, 63, 257), (63, 0, 257, 1), (257, 63, 1, 0)]
G = 4
N_BLOCKS64 = 7        # 1 + 1 + 5 blocks of 64 rows in every order
# the op splits the jobs over ceil(1024 / n_blocks64) = 147 shares of four
# waves: one job more than 4 * 147 makes a wave stride to a second job
J_BIG = 4 * 147 + 1
JOB_COUNTS = (1, 4, 5, J_BIG)

CASES = [(F, spec, n_trees) for F in (16, 7)
         for spec in (None, "scale", "scale+pca")
         for n_trees in (1, 10, 11, 23)]


# -- hand-built detectors (the construction of tests/test_gpu_importance.py)
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
    """Cuts taken FROM the transformed inputs, so a row's own value (and,
    without a projection, every grid value taken from a row) lies exactly
    on a cut; each column's extremes stay outside the cuts."""
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
    """Collects nodes in creation order (NOT canonical)."""

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
    if rng.rand() < 0.25:
        c0 = c1 = max(c0, 1.0)               # an argmax tie, proba 0.5
    if c0 + c1 == 0:
        c1 = 3.0
    return c0, c1


def _random_tree(n_cut, rng, max_depth):
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
    b.rows[b.node()][4:6] = _leaf_counts(rng)
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
    """Tree kinds rotate: a random tree, a single leaf, a chain."""
    from flake16_framework_amd.engine.detector import assemble_detector
    rng = np.random.RandomState(seed)
    params = _params(F, spec, rng)
    X = _pool(F, params, rng)
    T32 = transform_preprocessing(X, params).astype(np.float32)
    cuts = _cuts_from(T32, rng)
    n_cut = [len(c) for c in cuts]
    trees = []
    for t in range(n_trees):
        if t % 3 == 0:
            trees.append(_random_tree(n_cut, rng, max_depth=6))
        elif t % 3 == 1:
            trees.append(_root_leaf_tree(rng))
        else:
            trees.append(_chain_tree(n_cut, rng))
    cols = tuple(range(16)) if F == 16 else FLAKEFLAGGER_COLUMNS
    det = assemble_detector(
        ("NOD", "Flake16" if F == 16 else "FlakeFlagger", "None", "None",
         "Random Forest"), 2, cols, params, cuts, trees, n_trees, 0, M_POOL)
    return det, X, cuts


# -- the numpy side ---------------------------------------------------------
def _acc_numpy(det, X):
    T = transform_preprocessing(X, det.preprocessing_params())
    codes = bin_codes(T.astype(np.float32), det.cut_list())
    return np.stack(accumulate_proba(det.trees(), codes), axis=1)


def _job_list(F, spec, X, cuts, rng):
    """Feature-major (column, value) pairs: per column a value far below
    and far above every row's (so below the first and above the last cut
    without a projection), three rows' own values (on a cut wherever the
    row's value was taken as one; under a projection the only way to put
    a component exactly on a cut), and without preprocessing the first,
    middle and last cut itself with both float64 neighbours: the lower
    one rounds to the cut in fp32 and must be coded like it."""
    col, val = [], []
    for f in range(F):
        v = {X[:, f].min() - 1e3, X[:, f].max() + 1e3,
             *X[rng.choice(M_POOL, size=3, replace=False), f]}
        if spec is None and len(cuts[f]):
            for c in cuts[f][[0, len(cuts[f]) // 2, -1]]:
                c64 = np.float64(c)
                below = np.nextafter(c64, -np.inf)
                assert np.float32(below) == c and below < c64
                v |= {c64, below, np.nextafter(c64, np.inf)}
        v = sorted(float(x) for x in v)
        col += [f] * len(v)
        val += v
    return np.array(col, dtype=np.int32), np.array(val, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _case(F, spec, n_trees):
    """One hand-built detector, its pool of rows, the distinct jobs and
    the numpy (acc0, acc1) of every (job, pool row): computed once and
    shared by the tests, which only index into it."""
    seed = 1000 * F + 10 * n_trees + len(spec or "") + 3
    det, X, cuts = _hand_built(F, spec, n_trees, seed)
    rng = np.random.RandomState(seed + 7)
    col, val = _job_list(F, spec, X, cuts, rng)
    Xj = np.tile(X, (len(col), 1, 1))
    Xj[np.arange(len(col)), :, col] = val[:, None]
    acc = _acc_numpy(det, Xj.reshape(-1, F)).reshape(len(col), M_POOL, 2)
    base = _acc_numpy(det, X)
    for a in (X, col, val, acc, base):
        a.setflags(write=False)
    # which pool rows each group takes, in a group's own order
    take = [rng.permutation(M_POOL) for _ in range(G)]
    return {"det": det, "X": X, "col": col, "val": val, "acc": acc,
            "base": base, "take": take, "seed": seed,
            # a threshold that probabilities of the reference hit exactly
            "threshold": float(np.median(base[:, 1] / n_trees))}


def _layout(case, sizes):
    idx = np.concatenate([case["take"][g][:m] for g, m in enumerate(sizes)])
    seg_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    return idx.astype(np.int64), seg_off


def _job_sets(case, order):
    """Indices into the distinct jobs for J = 1, 4, 5 and J_BIG (with
    repeats: the op takes any job list)."""
    rng = np.random.RandomState(case["seed"] + 100 + order)
    n = len(case["col"])
    return [rng.choice(n, size=J, replace=J > n) for J in JOB_COUNTS]


def _block_sums(a):
    """The definition's numpy lines for the rows of one group."""
    v = np.zeros((-(-len(a) // 64), 64))
    v.reshape(-1)[:len(a)] = a
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def _want(acc, seg_off, n_trees, threshold):
    """(S [G + 1], flagged [G + 1]) of one job from its rows' sums."""
    S = np.zeros(G + 1)
    flagged = np.zeros(G + 1, dtype=np.int32)
    pred = (acc[:, 1] > acc[:, 0] if threshold is None
            else acc[:, 1] / n_trees >= threshold)
    for g in range(G):
        s = 0.0
        for B in _block_sums(acc[seg_off[g]:seg_off[g + 1], 1]):
            s = s + B
        S[g] = s
        flagged[g] = pred[seg_off[g]:seg_off[g + 1]].sum()
    for g in range(G):
        S[G] = S[G] + S[g]
    flagged[G] = pred.sum()
    return S, flagged


@pytest.mark.parametrize("F,spec,n_trees", CASES)
def test_reduction_order_is_observable(F, spec, n_trees):
    """No GPU: on the inputs of test_op_equals_the_definition the pinned
    pairwise block sum and the left-to-right sum differ for some (job,
    block), and the job list holds what it is meant to hold."""
    case = _case(F, spec, n_trees)
    differ = blocks = 0
    for order, sizes in enumerate(GROUP_ORDERS):
        idx, seg_off = _layout(case, sizes)
        assert -(-np.diff(seg_off) // 64).sum() == N_BLOCKS64
        for j in np.unique(np.concatenate(_job_sets(case, order))):
            acc1 = case["acc"][j, idx, 1]
            for g in range(G):
                a = acc1[seg_off[g]:seg_off[g + 1]]
                for k, B in enumerate(_block_sums(a)):
                    seq = np.cumsum(a[64 * k:64 * k + 64])[-1]
                    differ += int(B != seq)
                    blocks += 1
    assert differ > 0, blocks
    # the jobs move sums, probabilities lie on the threshold, rows tie
    assert (case["acc"] != case["base"]).any()
    assert (case["base"][:, 1] / n_trees == case["threshold"]).any()
    if n_trees == 1:
        assert (case["acc"][..., 0] == case["acc"][..., 1]).any()


# -- the op against the definition ------------------------------------------
def _run_op(ops, d, col, val, threshold, want_ice):
    from flake16_framework_amd.engine.dependence import partial_dependence
    S, flagged, ice = partial_dependence(
        ops, d, torch.from_numpy(np.array(col)),
        torch.from_numpy(np.array(val)), threshold, want_ice)
    J, n_groups = len(col), len(d["seg_off"]) - 1
    assert S.dtype == ice.dtype == torch.float64
    assert flagged.dtype == torch.int32
    assert S.shape == flagged.shape == (J + 1, n_groups + 1)
    assert ice.shape == ((J, d["X64"].shape[0]) if want_ice else (0, 0))
    return S.cpu().numpy(), flagged.cpu().numpy(), ice.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("F,spec,n_trees", CASES)
def test_op_equals_the_definition(F, spec, n_trees):
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    case = _case(F, spec, n_trees)
    det, threshold = case["det"], case["threshold"]
    for order, sizes in enumerate(GROUP_ORDERS):
        idx, seg_off = _layout(case, sizes)
        d = grouped_inputs([det], case["X"][idx], seg_off)
        base = {t: _want(case["base"][idx], seg_off, n_trees, t)
                for t in (None, threshold)}
        for js in _job_sets(case, order):
            col, val = case["col"][js], case["val"][js]
            acc = case["acc"][js][:, idx]
            for t in (None, threshold):
                S, flagged, ice = _run_op(ops, d, col, val, t, True)
                np.testing.assert_array_equal(ice, acc[:, :, 1])
                want = [_want(a, seg_off, n_trees, t) for a in acc]
                want.append(base[t])
                np.testing.assert_array_equal(
                    flagged, np.stack([w[1] for w in want]))
                np.testing.assert_array_equal(
                    S, np.stack([w[0] for w in want]))


# -- the other oracles ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("F,spec", [(16, None), (7, "scale+pca")])
def test_ice_equals_the_existing_ops(F, spec):
    """detect_encode + forest_proba on an explicitly overwritten matrix."""
    from flake16_framework_amd.engine.detector import device_inputs
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    case = _case(F, spec, 11)
    idx, seg_off = _layout(case, GROUP_ORDERS[1])
    X = case["X"][idx]
    d = grouped_inputs([case["det"]], X, seg_off)
    one = device_inputs(case["det"], X)
    _, _, ice = _run_op(ops, d, case["col"], case["val"], None, True)
    for j, (f, v) in enumerate(zip(case["col"], case["val"])):
        Xp = one["X64"].clone()
        Xp[:, int(f)] = float(v)
        codes = ops.detect_encode(Xp, one["mean"], one["scale"],
                                  one["pca_mean"], one["W"], one["has_pca"],
                                  one["cuts"], one["cut_off"], one["F"])
        acc = ops.forest_proba(codes, one["tree_off"], one["nodes"],
                               one["n_trees"])
        np.testing.assert_array_equal(ice[j], acc[:, 1].cpu().numpy())


@pytest.mark.gpu
def test_ice_on_and_off_give_the_same_sums():
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    for F, spec in ((16, "scale"), (7, "scale+pca")):
        case = _case(F, spec, 10)
        idx, seg_off = _layout(case, GROUP_ORDERS[2])
        d = grouped_inputs([case["det"]], case["X"][idx], seg_off)
        for t in (None, case["threshold"]):
            on = _run_op(ops, d, case["col"], case["val"], t, True)
            off = _run_op(ops, d, case["col"], case["val"], t, False)
            np.testing.assert_array_equal(on[0], off[0])
            np.testing.assert_array_equal(on[1], off[1])
            assert on[1][:, G].max() > 0 and (on[0] > 0).any()


@pytest.mark.gpu
def test_no_rows():
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    case = _case(7, "scale+pca", 10)
    d = grouped_inputs([case["det"]], case["X"][:0], [0, 0, 0])
    col, val = case["col"][:5], case["val"][:5]
    for want_ice in (False, True):
        S, flagged, ice = _run_op(ops, d, col, val, None, want_ice)
        assert S.shape == (6, 3) and not S.any() and not flagged.any()
        assert ice.size == 0


# -- end to end -------------------------------------------------------------
@pytest.fixture(scope="module")
def tests600():
    return make_synthetic_tests(n_tests=600, seed=0)


@pytest.mark.gpu
@pytest.mark.parametrize("keys", [
    SHAP_CONFIGS[0],
    ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN", "Random Forest"),
], ids=["nod", "pca-flakeflagger"])
def test_dependence_equal_across_backends(keys, tests600, tmp_path):
    from flake16_framework_amd.engine.dependence import write_dependence
    from flake16_framework_amd.engine.detector import fit_detector
    det = fit_detector(keys, tests=tests600, seed=0, backend="ref",
                       n_trees=12)
    for threshold in (None, 0.3):
        res = {}
        for backend in ("ref", "hip"):
            res[backend] = write_dependence(
                det, tests=tests600, out_file=str(tmp_path / backend),
                grid=8, threshold=threshold, ice=True, backend=backend)
        want, got = dict(res["ref"]), dict(res["hip"])
        np.testing.assert_array_equal(got.pop("ice"), want.pop("ice"))
        assert got == want
        assert (tmp_path / "hip").read_bytes() == \
            (tmp_path / "ref").read_bytes()
        doc = json.loads((tmp_path / "hip").read_text())
        assert doc["features"] == want["features"]
        assert len(want["features"]) == len(det.feature_cols)
        assert any(e["range"] > 0 for e in want["features"].values())
        assert want["baseline"]["flagged"] > 0


# -- host checks ------------------------------------------------------------
@pytest.mark.gpu
def test_op_refuses_bad_arguments():
    """Every refusal is a host check: nothing is launched."""
    from flake16_framework_amd.engine.dependence import partial_dependence
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    F = 7
    case = _case(F, "scale", 10)
    d = grouped_inputs([case["det"]], case["X"][:10], [0, 5, 10])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)

    def run(col, val, inputs=d, threshold=None):
        return partial_dependence(ops, inputs, col, val, threshold, True)

    S, flagged, ice = run(i32([0, F - 1]), f64([1.0, -2.0]))
    assert S.shape == (3, 3) and ice.shape == (2, 10)
    S, _, _ = run(i32([1] * 1024), f64([0.5] * 1024))
    assert S.shape == (1025, 3)
    for val in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(RuntimeError):
            run(i32([0, 1]), f64([1.0, val]))
    for col in ([F], [0, 16], [-1]):
        with pytest.raises(RuntimeError):
            run(i32(col), f64([1.0] * len(col)))
    with pytest.raises(RuntimeError):                    # J = 0
        run(i32([]), f64([]))
    with pytest.raises(RuntimeError):                    # J > 1024
        run(i32([0] * 1025), f64([1.0] * 1025))
    with pytest.raises(RuntimeError):                    # lengths differ
        run(i32([0, 1]), f64([1.0]))
    with pytest.raises(RuntimeError):                    # wrong dtypes
        run(torch.tensor([0, 1]), f64([1.0, 2.0]))
    with pytest.raises(RuntimeError):
        run(i32([0, 1]), torch.tensor([1.0, 2.0], dtype=torch.float32))
    with pytest.raises(RuntimeError):                    # jobs on the device
        run(i32([0, 1]).cuda(), f64([1.0, 2.0]))
    with pytest.raises(RuntimeError):
        run(i32([0, 1]), f64([1.0, 2.0]).cuda())
    with pytest.raises(RuntimeError):
        run(i32([0]), f64([1.0]), inputs=dict(d, X64=d["X64"].float()))
    with pytest.raises(RuntimeError):
        run(i32([0]), f64([1.0]), threshold=float("nan"))
    for seg in ([0, 5, 9], [0, 5, 11], [1, 5, 10], [0, 7, 5, 10]):
        with pytest.raises(RuntimeError):
            run(i32([0]), f64([1.0]), inputs=dict(d, seg_off=i32(seg)))
    bad = d["cut_off"].clone()
    bad[0, 16] += 1                        # past the end of the cut array
    with pytest.raises(RuntimeError):
        run(i32([0]), f64([1.0]), inputs=dict(d, cut_off=bad))
    with pytest.raises(RuntimeError):      # one root id short
        run(i32([0]), f64([1.0]),
            inputs=dict(d, tree_off=d["tree_off"][:-1]))
