"""GPU tests for holdout: the grouped kernels of ops/hip/holdout.hip against
the numpy reference and against the single-detector ops bit for bit on
hand-built groups, threshold_counts against numpy counts, and the device
backend of holdout() against the ref backend."""

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

pytestmark = pytest.mark.gpu

M_POOL = 257          # > one 256-thread block and > four 64-row blocks
CHAIN_DEPTH = 24
ONE_CUT, MANY_CUTS, CONST_COL = 0, 1, 2   # feature roles
# rows per group: the empty group first, in the middle, last
GROUP_ORDERS = [(0, 1, 63, 257), (63, 0, 257, 1), (257, 63, 1, 0)]


# -- hand-built detectors (the construction of tests/test_gpu_detector.py,
# -- one per group, each with its own parameters, cuts and forest) ---------
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


def _hand_built(F, spec, n_trees, g, seed):
    """Group g's detector: tree kinds rotate with t + g, so with one tree
    per forest the groups still hold a random tree, a single leaf and a
    chain, and forests of different groups differ in node count."""
    from flake16_framework_amd.engine.detector import assemble_detector
    rng = np.random.RandomState(seed)
    params = _params(F, spec, rng)
    X = _pool(F, params, rng)
    T32 = transform_preprocessing(X, params).astype(np.float32)
    cuts = _cuts_from(T32, rng)
    n_cut = [len(c) for c in cuts]
    trees = []
    for t in range(n_trees):
        kind = (t + g) % 3
        if kind == 0:
            trees.append(_random_tree(n_cut, rng, max_depth=4 + g))
        elif kind == 1:
            trees.append(_root_leaf_tree(rng))
        else:
            trees.append(_chain_tree(n_cut, rng))
    cols = tuple(range(16)) if F == 16 else FLAKEFLAGGER_COLUMNS
    det = assemble_detector(
        ("NOD", "Flake16" if F == 16 else "FlakeFlagger", "None", "None",
         "Random Forest"), 2, cols, params, cuts, trees, n_trees, 0, M_POOL)
    return det, X, T32


@pytest.mark.parametrize("n_trees", [1, 10, 11, 23])
@pytest.mark.parametrize("spec", [None, "scale", "scale+pca"])
@pytest.mark.parametrize("F", [16, 7])
def test_grouped_kernels_bitwise_on_hand_built(F, spec, n_trees):
    from flake16_framework_amd.engine.detector import (
        FPAD, device_inputs,
    )
    from flake16_framework_amd.engine.holdout import (
        grouped_acc, grouped_inputs,
    )
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    G = 4
    built = [_hand_built(F, spec, n_trees, g,
                         seed=1000 * F + 10 * n_trees + g) for g in range(G)]
    dets = [b[0] for b in built]

    # the groups differ where the kernels index per group
    assert len({len(d.feat) for d in dets}) > 1
    assert len({len(d.cuts) for d in dets}) > 1
    kinds = [np.diff(d.tree_off) for d in dets]
    assert any((k == 1).any() for k in kinds)                  # single leaf
    assert any((k == 2 * CHAIN_DEPTH + 1).any() for k in kinds)     # chain
    for det, _, T32 in built:
        n_cut = np.diff(det.cut_off)[:F]
        assert n_cut[ONE_CUT] == 1 and n_cut[MANY_CUTS] == 255
        assert det.scale[CONST_COL] == 1.0
        for f in range(F):
            assert np.isin(T32[:, f], det.cut_list()[f]).any(), f

    for sizes in GROUP_ORDERS:
        seg_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
        X = np.concatenate([b[1][:m] for b, m in zip(built, sizes)])
        d = grouped_inputs(dets, X, seg_off)
        codes = ops.holdout_encode(
            d["X64"], d["seg_off"], d["mean"], d["scale"], d["pca_mean"],
            d["W"], d["has_pca"], d["cuts"], d["cut_off"], d["F"])
        acc = grouped_acc(ops, d)
        assert codes.shape == (len(X), FPAD) and codes.dtype == torch.uint8
        assert acc.shape == (len(X), 2) and acc.dtype == torch.float64
        codes, acc = codes.cpu().numpy(), acc.cpu().numpy()
        assert (codes[:, F:] == 0).all()

        for g, ((det, Xg, T32), m) in enumerate(zip(built, sizes)):
            s = slice(seg_off[g], seg_off[g + 1])
            ref_codes = bin_codes(T32[:m], det.cut_list())
            np.testing.assert_array_equal(codes[s, :F], ref_codes,
                                          err_msg=f"{sizes} group {g}")
            if m == 0:
                continue
            if m == M_POOL:
                assert ref_codes[:, MANY_CUTS].max() == 255
            acc0, acc1 = accumulate_proba(det.trees(), ref_codes)
            np.testing.assert_array_equal(acc[s, 0], acc0)
            np.testing.assert_array_equal(acc[s, 1], acc1)

            # the single-detector ops on the slice alone
            one = device_inputs(det, Xg[:m])
            codes_one = ops.detect_encode(
                one["X64"], one["mean"], one["scale"], one["pca_mean"],
                one["W"], one["has_pca"], one["cuts"], one["cut_off"],
                one["F"])
            acc_one = ops.forest_proba(codes_one, one["tree_off"],
                                       one["nodes"], one["n_trees"])
            np.testing.assert_array_equal(codes[s], codes_one.cpu().numpy())
            np.testing.assert_array_equal(acc[s], acc_one.cpu().numpy())
        if n_trees >= 3:
            big = sizes.index(M_POOL)
            s = slice(seg_off[big], seg_off[big + 1])
            assert len(np.unique(acc[s, 1])) > 10    # not a constant forest


def test_grouped_ops_reject_bad_offsets():
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    built = [_hand_built(7, "scale", 2, g, seed=g) for g in range(2)]
    X = np.concatenate([b[1][:5] for b in built])
    d = grouped_inputs([b[0] for b in built], X, [0, 5, 10])

    def encode(**kw):
        a = dict(d, **kw)
        return ops.holdout_encode(
            a["X64"], a["seg_off"], a["mean"], a["scale"], a["pca_mean"],
            a["W"], a["has_pca"], a["cuts"], a["cut_off"], a["F"])

    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    encode()
    for seg in ([0, 5, 9], [0, 5, 11], [1, 5, 10], [0, 7, 5, 10]):
        with pytest.raises(RuntimeError):
            encode(seg_off=i32(seg))
    bad = d["cut_off"].clone()
    bad[1, 16] += 1                        # past the end of the cut array
    with pytest.raises(RuntimeError):
        encode(cut_off=bad)
    bad = d["cut_off"].clone()
    bad[1, 3], bad[1, 4] = bad[1, 4].item() + 1, bad[1, 3].item()
    with pytest.raises(RuntimeError):      # offsets step back
        encode(cut_off=bad)
    codes = encode()
    with pytest.raises(RuntimeError):      # one root id short
        ops.holdout_proba(codes, d["seg_off"], d["tree_off"][:-1],
                          d["nodes"], d["n_trees"])
    with pytest.raises(RuntimeError):
        ops.holdout_proba(codes, i32([0, 5, 11]), d["tree_off"],
                          d["nodes"], d["n_trees"])


# -- threshold_counts -------------------------------------------------------
def _counts_dev(acc0, acc1, labels, seg_off, n_trees, thresholds):
    from flake16_framework_amd.ops.backend import get_ops
    dev = torch.device("cuda:0")
    acc = torch.from_numpy(np.stack([acc0, acc1], axis=1)).to(dev)
    curve, argmax = get_ops().threshold_counts(
        acc.contiguous(), torch.from_numpy(labels).to(dev),
        torch.tensor(list(seg_off), dtype=torch.int32), n_trees,
        torch.from_numpy(np.asarray(thresholds, dtype=np.float64)))
    assert curve.dtype == argmax.dtype == torch.int32
    return curve.cpu().numpy(), argmax.cpu().numpy()


def test_threshold_counts_hand_written_table():
    import test_holdout as cpu
    from flake16_framework_amd.engine.holdout import make_thresholds
    acc0, acc1, labels = cpu.table_arrays()
    curve, argmax = _counts_dev(acc0, acc1, labels, cpu.TABLE_SEG,
                                cpu.TABLE_TREES,
                                make_thresholds(cpu.TABLE_K))
    assert argmax.tolist() == cpu.TABLE_ARGMAX
    assert curve.tolist() == cpu.TABLE_CURVE


@pytest.mark.parametrize("K", [1, 2, 101, 256])
@pytest.mark.parametrize("M", [1, 63, 257, 1000])
def test_threshold_counts_against_numpy(M, K):
    from flake16_framework_amd.engine.holdout import (
        counts_ref, make_thresholds,
    )
    thresholds = make_thresholds(K)
    for n_trees in (4, 100):
        rng = np.random.RandomState(1000 * M + 10 * K + n_trees)
        # whole votes: proba = j / n_trees lands on thresholds exactly
        # (every j for K = 101, n_trees = 100); a quarter of the rows
        # carry fractional sums instead
        acc1 = rng.randint(0, n_trees + 1, size=M).astype(np.float64)
        frac = rng.rand(M) < 0.25
        acc1[frac] = rng.uniform(0, n_trees, size=int(frac.sum()))
        acc0 = n_trees - acc1
        if M > 4:
            acc0[:2] = acc1[:2] = n_trees / 2          # argmax ties
            acc0[2:4], acc1[2:4] = (0, n_trees), (n_trees, 0)
        labels = (rng.rand(M) < 0.3).astype(np.uint8)
        G = 5                                  # group 2 is always empty
        inner = np.sort(rng.randint(0, M + 1, size=G - 2))
        seg_off = np.array([0, inner[0], inner[1], inner[1], inner[2], M])
        proba = acc1 / n_trees
        if M > 4 and K >= 2:
            assert np.isin(proba[2:4], thresholds).all()   # t = 1 and t = 0
        want_curve, want_argmax = counts_ref(proba, acc1 > acc0, labels,
                                             seg_off, thresholds)
        curve, argmax = _counts_dev(acc0, acc1, labels, seg_off, n_trees,
                                    thresholds)
        assert curve.shape == (G + 1, K, 3) and argmax.shape == (G + 1, 3)
        np.testing.assert_array_equal(curve, want_curve)
        np.testing.assert_array_equal(argmax, want_argmax)


def test_threshold_counts_rejects_bad_thresholds():
    acc0, acc1 = np.array([1.0, 3.0]), np.array([3.0, 1.0])
    labels = np.array([1, 0], dtype=np.uint8)
    _counts_dev(acc0, acc1, labels, [0, 1, 2], 4, [0.0, 0.5, 1.0])
    for bad in ([0.0, 0.5, 0.5], [0.5, 0.25], [0.0, np.nan], [0.0, np.inf],
                [-np.inf, 0.0], [], np.arange(257) / 256):
        with pytest.raises(RuntimeError):
            _counts_dev(acc0, acc1, labels, [0, 1, 2], 4, bad)
    with pytest.raises(RuntimeError):      # rows outside the groups
        _counts_dev(acc0, acc1, labels, [0, 1, 1], 4, [0.5])


# -- end to end -------------------------------------------------------------
CONFIGS = {
    "nod": SHAP_CONFIGS[0],
    "od": SHAP_CONFIGS[1],
    "pca-flakeflagger": ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN",
                         "Random Forest"),
}


@pytest.fixture(scope="module")
def tests5():
    return make_synthetic_tests(n_tests=300, n_projects=5, seed=2)


def _assert_same_result(got, want):
    assert got.keys() == want.keys()
    for name in ("config_keys", "seed", "n_trees", "projects", "total"):
        assert got[name] == want[name], name
    np.testing.assert_array_equal(got["thresholds"], want["thresholds"])
    for name in ("proba", "pred", "projects", "nodeids"):
        assert got["oof"][name].dtype == want["oof"][name].dtype, name
        np.testing.assert_array_equal(got["oof"][name], want["oof"][name],
                                      err_msg=name)
    assert len(got["detectors"]) == len(want["detectors"])
    for g, (a, b) in enumerate(zip(got["detectors"], want["detectors"])):
        a, b = a.arrays(), b.arrays()
        assert a.keys() == b.keys()
        for name in a:
            assert a[name].dtype == b[name].dtype, name
            np.testing.assert_array_equal(a[name], b[name],
                                          err_msg=f"fold {g} {name}")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_holdout_equal_across_backends(name, tests5, monkeypatch):
    from flake16_framework_amd.engine import holdout as H
    kw = dict(tests=tests5, n_trees=12, keep_detectors=True)
    want = H.holdout(CONFIGS[name], backend="ref", **kw)
    got = H.holdout(CONFIGS[name], backend="hip", **kw)
    _assert_same_result(got, want)
    assert want["total"]["curve"][0][2] == want["total"]["n_flaky"] > 0

    # the same folds fitted in at least three forest_fit calls
    chunkings = []
    fold_chunks = H._fold_chunks

    def spy(*args):
        chunkings.append(fold_chunks(*args))
        return chunkings[-1]

    monkeypatch.setenv("FLAKE16_FUSE_MAX_S", "7000")
    monkeypatch.setattr(H, "_fold_chunks", spy)
    chunked = H.holdout(CONFIGS[name], backend="hip", **kw)
    assert len(chunkings) == 1 and len(chunkings[0]) >= 3
    assert sum(chunkings[0], []) == list(range(5))
    _assert_same_result(chunked, want)
