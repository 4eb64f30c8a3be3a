"""GPU tests for similar: forest_leaves against the numpy walk on
hand-built forests (and on a complete tree whose leaf ids pass 16 bits),
proximity_topk against numpy on leaf matrices given directly, integer for
integer, over the sizes at which the kernel changes path; the op's host
checks; the device backend of similar() against the ref backend."""

import numpy as np
import pytest
import torch

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.constants import FLAKEFLAGGER_COLUMNS
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
from flake16_framework_amd.models.binning import bin_codes
from flake16_framework_amd.models.forest_ref import (
    Tree, _tree_leaves, canonicalize_tree,
)
from flake16_framework_amd.preprocess import transform_preprocessing

pytestmark = pytest.mark.gpu

M_POOL = 257          # > one 256-thread block
CHAIN_DEPTH = 24
ONE_CUT, MANY_CUTS, CONST_COL = 0, 1, 2   # feature roles


@pytest.fixture(scope="module")
def ops():
    from flake16_framework_amd.ops.backend import get_ops
    return get_ops()


# -- hand-built detectors (the construction of tests/test_gpu_holdout.py and
# -- tests/test_gpu_importance.py) -------------------------------------------
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
    """Cuts taken FROM the transformed inputs, so rows lie on cut values
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
        kind = (t + seed) % 3
        if kind == 0:
            trees.append(_random_tree(n_cut, rng, max_depth=5))
        elif kind == 1:
            trees.append(_root_leaf_tree(rng))
        else:
            trees.append(_chain_tree(n_cut, rng))
    cols = tuple(range(16)) if F == 16 else FLAKEFLAGGER_COLUMNS
    det = assemble_detector(
        ("NOD", "Flake16" if F == 16 else "FlakeFlagger", "None", "None",
         "Random Forest"), 2, cols, params, cuts, trees, n_trees, 0, M_POOL)
    return det, X


def _leaves_numpy(det, X):
    T = transform_preprocessing(X, det.preprocessing_params())
    codes = bin_codes(T.astype(np.float32), det.cut_list())
    return np.stack([_tree_leaves(tree, codes) for tree in det.trees()],
                    axis=1)


def _leaves_device(ops, det, X):
    from flake16_framework_amd.engine.detector import device_inputs
    from flake16_framework_amd.engine.similar import device_leaves
    leaf = device_leaves(ops, device_inputs(det, X))[1]
    assert leaf.dtype == torch.int32 and leaf.is_contiguous()
    assert leaf.shape == (len(X), det.n_trees)
    return leaf.cpu().numpy()


# -- forest_leaves -----------------------------------------------------------
@pytest.mark.parametrize("n_trees", [1, 10, 11, 101])
@pytest.mark.parametrize("spec", [None, "scale", "scale+pca"])
@pytest.mark.parametrize("F", [16, 7])
def test_forest_leaves_on_hand_built(F, spec, n_trees, ops):
    seed = n_trees + F
    det, X = _hand_built(F, spec, n_trees, seed=seed)
    want = _leaves_numpy(det, X)
    got = _leaves_device(ops, det, X)
    assert np.array_equal(got, want)
    for t in range(n_trees):
        if (t + seed) % 3 == 2:     # a chain, walked to its end
            assert want[:, t].max() == 2 * CHAIN_DEPTH
        elif (t + seed) % 3 == 1:
            assert (want[:, t] == 0).all()
    one = _leaves_device(ops, det, X[:1])
    assert np.array_equal(one, want[:1])
    none = _leaves_device(ops, det, X[:0])
    assert none.shape == (0, n_trees)


def _complete_tree_detector(levels=16):
    """One complete tree: level d splits on feature d at bin 0, so a row of
    {0, 1} codes reaches leaf 2^levels - 1 + (its codes read as a binary
    number, feature 0 the highest bit).  Already canonical: the children of
    node i are 2 i + 1 and 2 i + 2."""
    from flake16_framework_amd.engine.detector import assemble_detector
    F = 16
    n_int = 2 ** levels - 1
    n = 2 ** (levels + 1) - 1
    i = np.arange(n)
    internal = i < n_int
    level = np.floor(np.log2(i + 1)).astype(np.int32)
    feat = np.where(internal, level, -1).astype(np.int32)
    left = np.where(internal, 2 * i + 1, -1).astype(np.int32)
    right = np.where(internal, 2 * i + 2, -1).astype(np.int32)
    tree = Tree(feat, np.zeros(n, dtype=np.int32),
                np.zeros(n, dtype=np.float32), left, right,
                np.ones(n), (i % 3).astype(np.float64))
    params = {"spec": None, "mean": np.zeros(F), "scale": np.ones(F),
              "pca_mean": np.zeros(F), "W": np.eye(F)}
    cuts = [np.array([0.0], dtype=np.float32)] * F
    return assemble_detector(
        ("NOD", "Flake16", "None", "None", "Decision Tree"), 2,
        tuple(range(16)), params, cuts, [tree], 1, 0, 1)


def test_forest_leaves_pass_16_bits(ops):
    det = _complete_tree_detector()
    assert len(det.feat) == 131071
    rng = np.random.RandomState(0)
    bits = rng.randint(0, 2, size=(300, 16))
    bits[0], bits[1] = 0, 1
    X = np.where(bits == 1, 1.0, -1.0)       # the cut is 0.0: code = bit
    want = 65535 + (bits << np.arange(15, -1, -1)).sum(axis=1)
    assert want.min() == 65535 and want.max() == 131070
    assert np.array_equal(_leaves_numpy(det, X)[:, 0], want)
    got = _leaves_device(ops, det, X)
    assert np.array_equal(got[:, 0], want)

    # and such ids compare at full width: 65536 + x is not x
    _check(ops, got[:40], np.concatenate([got - 65536, got]), None, 5)


# -- proximity_topk on given leaf matrices -----------------------------------
def _topk_numpy(lq, lc, self_idx, k):
    M, N = len(lq), len(lc)
    idx = np.full((M, k), -1, dtype=np.int32)
    shared = np.zeros((M, k), dtype=np.int32)
    if N == 0 or M == 0:
        return idx, shared
    s = np.zeros((M, N), dtype=np.int64)
    for t in range(lq.shape[1]):
        s += lq[:, t, None] == lc[None, :, t]
    if self_idx is not None:
        rows = np.flatnonzero(self_idx >= 0)
        s[rows, self_idx[rows]] = -1
    cols = np.arange(N)
    for q in range(M):
        order = np.lexsort((cols, -s[q]))
        order = order[s[q][order] >= 0][:k]
        idx[q, :len(order)] = order
        shared[q, :len(order)] = s[q][order]
    return idx, shared


def _run(ops, lq, lc, self_idx, k):
    dev = torch.device("cuda")
    if self_idx is None:
        self_idx = np.full(len(lq), -1, dtype=np.int32)
    idx, shared = ops.proximity_topk(
        torch.from_numpy(np.ascontiguousarray(lq)).to(dev),
        torch.from_numpy(np.ascontiguousarray(lc)).to(dev),
        torch.from_numpy(self_idx), k)
    assert idx.dtype == shared.dtype == torch.int32
    assert idx.shape == shared.shape == (len(lq), k)
    return idx.cpu().numpy(), shared.cpu().numpy()


def _check(ops, lq, lc, self_idx, k, what=""):
    got_idx, got_sh = _run(ops, lq, lc, self_idx, k)
    idx, shared = _topk_numpy(lq, lc, self_idx, k)
    assert np.array_equal(got_sh, shared), what
    assert np.array_equal(got_idx, idx), what


def _ids(kind, rows, T, rng):
    """int32 [rows, T] of one kind of content."""
    if kind == "identical":
        return np.tile(rng.randint(0, 1000, size=T), (rows, 1)).astype(
            np.int32)
    if kind == "low":            # massive ties at every count
        return rng.randint(0, 2, size=(rows, T)).astype(np.int32)
    if kind == "wide":
        # ids that differ by exactly 65,536 (equal low halves), and ids at
        # the top of int32 that differ in the high or the low half only
        pool = np.array([7, 7 + 65536, 7 + 2 * 65536, 2 ** 31 - 1,
                         2 ** 31 - 2, 2 ** 31 - 1 - 65536, 0, 65535],
                        dtype=np.int64)
        return pool[rng.randint(0, len(pool), size=(rows, T))].astype(
            np.int32)
    raise ValueError(kind)


def _sizes(k):
    from flake16_framework_amd.engine.similar import PROX_CHUNK, PROX_TILE
    assert (PROX_TILE, PROX_CHUNK) == (32, 512)    # ops/hip/similar.hip
    ns = {0, 1, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, PROX_TILE + 1,
          PROX_CHUNK + 1}
    return sorted(ns), [0, 1, 63, 64, 65, 257]


@pytest.mark.parametrize("kind", ["identical", "low", "wide"])
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("T", [1, 2, 3, 101])
def test_proximity_topk_sizes(T, k, kind, ops):
    """Every N x M of the list; the rows are drawn once per case and cut
    to size, so a shorter corpus is a prefix of a longer one."""
    rng = np.random.RandomState(1000 * T + 10 * k + len(kind))
    ns, ms = _sizes(k)
    pool_q = _ids(kind, max(ms), T, rng)
    pool_c = _ids(kind, max(ns), T, rng)
    if kind == "identical":
        pool_c = np.tile(pool_q[:1], (max(ns), 1))
    for N in ns:
        for M in ms:
            lq, lc = pool_q[:M], pool_c[:N]
            got_idx, got_sh = _run(ops, lq, lc, None, k)
            what = f"N={N} M={M}"
            if kind == "identical":
                # every count equals T: the answer is rows 0 .. k-1
                fill = min(N, k)
                want = np.full((M, k), -1)
                want[:, :fill] = np.arange(fill)
                assert np.array_equal(got_idx, want), what
                assert np.array_equal(got_sh, np.where(want >= 0, T, 0)), \
                    what
            else:
                idx, shared = _topk_numpy(lq, lc, None, k)
                assert np.array_equal(got_sh, shared), what
                assert np.array_equal(got_idx, idx), what


@pytest.mark.parametrize("kind", ["low", "wide"])
@pytest.mark.parametrize("T", [52, 53, 104, 105, 209])
def test_proximity_topk_row_pieces(T, kind, ops):
    """T on both sides of one register piece of a row (52 dwords: 104
    packed ids, 52 at full width), and a row of several pieces."""
    rng = np.random.RandomState(T)
    lq, lc = _ids(kind, 70, T, rng), _ids(kind, 600, T, rng)
    lc[17], lc[590] = lq[3], lq[3]           # full counts, far apart
    _check(ops, lq, lc, None, 5)


def test_proximity_topk_ties_across_chunks(ops):
    """Equal counts on the two sides of both chunk boundaries come out in
    index order, after a higher count from the last chunk."""
    from flake16_framework_amd.engine.similar import PROX_CHUNK as C
    T, N, M = 3, 2 * C + 5, 3
    lq = np.tile(np.array([[5, 6, 7]], dtype=np.int32), (M, 1))
    lc = np.full((N, T), 9, dtype=np.int32)          # shares nothing
    ties = [C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 4]
    lc[ties] = [5, 6, 0]                             # two trees
    lc[2 * C + 2] = [5, 6, 7]                        # all three
    for k in (1, 5, 16):
        got_idx, got_sh = _run(ops, lq, lc, None, k)
        want = ([2 * C + 2] + ties + list(range(9)))[:k]
        assert got_idx.tolist() == [want] * M, k
        assert got_sh.tolist() == [([3] + [2] * 6 + [0] * 9)[:k]] * M, k
    _check(ops, lq, lc, None, 16)


def test_proximity_topk_self_idx(ops):
    from flake16_framework_amd.engine.similar import PROX_CHUNK as C
    from flake16_framework_amd.engine.similar import PROX_TILE as TILE
    rng = np.random.RandomState(5)
    T, N = 4, C + 40
    lc = _ids("low", N, T, rng)
    edges = [-1, 0, N - 1, TILE - 1, TILE, C - 1, C, 7]
    lq = lc[[max(e, 0) for e in edges]].copy()   # query = the skipped row
    self_idx = np.array(edges, dtype=np.int32)
    for k in (1, 5):
        got_idx, got_sh = _run(ops, lq, lc, self_idx, k)
        idx, shared = _topk_numpy(lq, lc, self_idx, k)
        assert np.array_equal(got_idx, idx) and np.array_equal(got_sh,
                                                               shared)
        for q, e in enumerate(edges):
            assert e < 0 or e not in got_idx[q]
    # a skipped row that would otherwise win alone
    lc2 = np.full((N, T), 9, dtype=np.int32)
    lc2[C] = lq[6]
    won = _run(ops, lq[6:7], lc2, np.array([-1], dtype=np.int32), 2)
    assert won[0].tolist() == [[C, 0]] and won[1].tolist() == [[T, 0]]
    lost = _run(ops, lq[6:7], lc2, np.array([C], dtype=np.int32), 2)
    assert lost[0].tolist() == [[0, 1]] and lost[1].tolist() == [[0, 0]]

    # padding when N - 1 < k, with and without a skipped row
    for N_small in (1, 2, 5):
        sub = lc[:N_small]
        _check(ops, lq[:3], sub, np.array([0, -1, N_small - 1],
                                          dtype=np.int32), 5)
        got_idx, _ = _run(ops, lq[:1], sub, np.array([0], dtype=np.int32),
                          5)
        assert (got_idx[0] >= 0).sum() == N_small - 1


def test_proximity_topk_long_chunks(ops):
    """More query blocks than 2048 / chunks: the corpus chunks grow to a
    multiple of PROX_CHUNK.  The reference is torch.topk of the int64 key
    shared * N + (N - 1 - idx), which is exact."""
    from flake16_framework_amd.engine.similar import PROX_CHUNK as C
    dev = torch.device("cuda")
    M, N, T, k = 33 * 256 - 7, 63 * C + 1, 3, 5      # 33 blocks x 64 chunks
    gen = torch.Generator().manual_seed(3)
    lq = torch.randint(0, 2, (M, T), generator=gen, dtype=torch.int32).to(dev)
    lc = torch.randint(0, 2, (N, T), generator=gen, dtype=torch.int32).to(dev)
    self_idx = torch.full((M,), -1, dtype=torch.int32)
    idx, shared = ops.proximity_topk(lq, lc, self_idx, k)
    col = torch.arange(N, device=dev, dtype=torch.int64)
    for a in range(0, M, 1024):
        s = torch.zeros((min(M, a + 1024) - a, N), dtype=torch.int64,
                        device=dev)
        for t in range(T):
            s += lq[a:a + 1024, t, None] == lc[None, :, t]
        key = torch.topk(s * N + (N - 1 - col), k, dim=1).values
        assert torch.equal(shared[a:a + 1024].long(), key // N)
        assert torch.equal(idx[a:a + 1024].long(), N - 1 - key % N)


def test_ops_refuse_bad_arguments(ops):
    dev = torch.device("cuda")
    lq = torch.zeros((4, 3), dtype=torch.int32, device=dev)
    lc = torch.zeros((6, 3), dtype=torch.int32, device=dev)
    none = torch.full((4,), -1, dtype=torch.int32)
    ops.proximity_topk(lq, lc, none, 16)
    ops.proximity_topk(lq, lc, none.to(dev), 1)      # either side
    bad = [
        (lq.long(), lc, none, 5),                    # dtype
        (lq, lc.float(), none, 5),
        (lq.cpu(), lc, none, 5),                     # device
        (lq, lc[:, :2].contiguous(), none, 5),       # T differs
        (lq.t().contiguous().t(), lc, none, 5),      # not contiguous
        (lq[:, :0], lc[:, :0], none, 5),             # T = 0
        (lq, lc, none, 0), (lq, lc, none, 17),       # k
        (lq, lc, none[:3], 5),                       # self_idx length
        (lq, lc, none.long(), 5),
        (lq, lc, torch.tensor([-1, 6, 0, 0], dtype=torch.int32), 5),
        (lq, lc, torch.tensor([-2, 0, 0, 0], dtype=torch.int32), 5),
        (lq, lc[:0], torch.tensor([0, -1, -1, -1], dtype=torch.int32), 5),
    ]
    for args in bad:
        with pytest.raises((RuntimeError, TypeError)):
            ops.proximity_topk(*args)

    from flake16_framework_amd.engine.detector import device_inputs
    det, X = _hand_built(16, None, 3, seed=0)
    d = device_inputs(det, X)
    codes = ops.detect_encode(d["X64"], d["mean"], d["scale"],
                              d["pca_mean"], d["W"], d["has_pca"],
                              d["cuts"], d["cut_off"], d["F"])
    ops.forest_leaves(codes, d["tree_off"], d["nodes"], 3)
    for args in [
        (codes.int(), d["tree_off"], d["nodes"], 3),
        (codes, d["tree_off"], d["nodes"], 2),       # offsets do not match
        (codes, d["tree_off"].int(), d["nodes"], 3),
        (codes, d["tree_off"], d["nodes"].cpu(), 3),
        (codes, d["tree_off"], d["nodes"], 0),
    ]:
        with pytest.raises((RuntimeError, TypeError)):
            ops.forest_leaves(*args)


# -- the stage ---------------------------------------------------------------
@pytest.fixture(scope="module")
def tests600():
    return make_synthetic_tests(n_tests=600, seed=0)


@pytest.fixture(scope="module")
def fitted600(tests600):
    from flake16_framework_amd.engine.detector import fit_detector
    return {keys: fit_detector(keys, tests=tests600, seed=0, backend="ref",
                               n_trees=6)
            for keys in (SHAP_CONFIGS[0],
                         ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN",
                          "Random Forest"))}


@pytest.mark.parametrize("own_file", [True, False])
@pytest.mark.parametrize("flaky_only", [False, True])
@pytest.mark.parametrize("keys", [
    SHAP_CONFIGS[0],
    ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN", "Random Forest")])
def test_similar_equal_across_backends(keys, flaky_only, own_file, tests600,
                                       fitted600):
    from flake16_framework_amd.engine.similar import similar
    det = fitted600[keys]
    tests = tests600 if own_file else make_synthetic_tests(n_tests=150,
                                                           seed=4)
    kw = dict(tests=tests, corpus=tests600, k=5, flaky_only=flaky_only)
    ref = similar(det, backend="ref", **kw)
    hip = similar(det, backend="hip", **kw)
    assert set(ref) == set(hip)
    for name, value in ref.items():
        assert np.array_equal(hip[name], value), name
        if isinstance(value, np.ndarray):
            assert hip[name].dtype == value.dtype, name
    if own_file and not flaky_only:
        assert not (hip["idx"] == np.arange(600)[:, None]).any()
    kept = similar(det, backend="hip", skip_self=False, **kw)
    want = similar(det, backend="ref", skip_self=False, **kw)
    assert np.array_equal(kept["idx"], want["idx"])
    assert np.array_equal(kept["shared"], want["shared"])


def test_similar_hip_on_empty_files(tests600, fitted600):
    from flake16_framework_amd.engine.similar import similar
    det = fitted600[SHAP_CONFIGS[0]]
    for kw in (dict(tests={}, corpus=tests600),
               dict(tests=tests600, corpus={})):
        ref = similar(det, backend="ref", k=3, **kw)
        hip = similar(det, backend="hip", k=3, **kw)
        for name, value in ref.items():
            assert np.array_equal(hip[name], value), name
