"""GPU tests for the per-node path of the mid and small subtree builders.

mid_subtree_kernel (65..2048 samples, LDS-staged, wave-parallel or
block-wide nodes) and small_subtree_kernel (<= 64 samples, one wave per
subtree) keep the feature permutation in a register, reduce with DPP and
carry the label in bit 15 of the staged sample index.  Every case fits
trees with ops.forest_fit_multi and compares them node by node with
models/forest_ref.py: the trees must be bit-identical.

The test_band_* cases do the same for the level band (> 2048 samples):
hist_split_kernel (RF, DT) and et_split_kernel (ET) build those nodes with
the node steps they share with the subtree builders, one 256-thread block
per node, partition the samples in 256-wide tiles and hand children of
65..2048 samples a precomputed histogram from the subtraction pools.  The
cases cover sizes either side of a partition-tile edge and with several
band levels, F below the pad, constant columns, ties, degenerate labels,
and the same trees with the pools switched off.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

JOB_BASE = 40
# (kind, random splitter, bootstrap): ET and RF take max_features =
# int(sqrt(F)) (4 at F = 16: the wave-parallel mid path), DT takes all F
# features (the block-wide mid path).
MODELS = [
    ("extra_trees", 1, 0),
    ("random_forest", 0, 1),
    ("decision_tree", 0, 0),
]
# small (<= 64), mid (65..2048) and the level band (> 2048), each side of
# both thresholds; 2048 puts label bits on staged indices above 1023.
TIER_SIZES = [2, 63, 64, 65, 66, 128, 129, 1024, 2047, 2048, 2049]
N_ROWS = 2049


@pytest.fixture(scope="module")
def ops():
    from flake16_framework_amd.ops.backend import get_ops
    return get_ops()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rand_data():
    """Random 0..255 codes in all 16 columns, about 30 % positives."""
    rng = np.random.RandomState(11)
    codes = rng.randint(0, 256, (N_ROWS, 16)).astype(np.uint8)
    y = (rng.rand(N_ROWS) < 0.3).astype(np.uint8)
    return codes, y


def _ref_params(kind):
    from flake16_framework_amd.models.forest_ref import params_for_model
    params = params_for_model({"kind": kind, "n_estimators": 1}, seed=0)
    params.n_trees = 1
    return params


def _jobs(sizes, F):
    """One single-tree job per (size, model): (n, key, kind, mf, boot, rnd)."""
    jobs = []
    for i, m in enumerate(sizes):
        for kind, rnd, boot in MODELS:
            mf = _ref_params(kind).resolve_max_features(F)
            jobs.append((m, JOB_BASE + 8 * i, kind, mf, boot, rnd))
    return jobs


def _reference(codes, y, sizes, F):
    """Reference trees of _jobs(sizes, F) on the row prefixes, columns < F."""
    from flake16_framework_amd.models.forest_ref import fit_forest
    return [fit_forest(np.ascontiguousarray(codes[:m, :F]), y[:m],
                       _ref_params(kind), job_base=key).trees[0]
            for m, key, kind, _, _, _ in _jobs(sizes, F)]


def _fit_multi(ops, dev, codes, y, jobs, F):
    codes_d = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
    y_d = torch.from_numpy(y).to(dev)
    col = lambda i, dt: torch.tensor([j[i] for j in jobs], dtype=dt)
    j_row_off = torch.zeros(len(jobs), dtype=torch.int32, device=dev)
    out = ops.forest_fit_multi(
        codes_d, y_d, j_row_off, col(0, torch.int32),
        col(1, torch.int32).to(dev), col(3, torch.int32),
        col(5, torch.uint8), col(4, torch.uint8), F, 0)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _assert_trees_equal(out, ref_trees):
    nfeat, nsplit, nleft, c0, c1, j_node_off, node_alloc = out
    for t, tree in enumerate(ref_trees):
        assert node_alloc[t] == tree.n_nodes, (t, node_alloc[t],
                                               tree.n_nodes)
    # node numbering may differ (device allocation order): compare
    # structurally by walking both trees from the root.
    for t, tree in enumerate(ref_trees):
        base = int(j_node_off[t])
        stack = [(0, 0)]   # (ref node, dev node)
        while stack:
            r, d = stack.pop()
            assert c0[base + d] == tree.count0[r], (t, r)
            assert c1[base + d] == tree.count1[r], (t, r)
            if tree.feature[r] == -1:
                assert nfeat[base + d] == -1, (t, r)
                continue
            assert nfeat[base + d] == tree.feature[r], (t, r)
            assert nsplit[base + d] == tree.split_bin[r], (t, r)
            dl = nleft[base + d]
            stack.append((tree.left[r], dl))
            stack.append((tree.right[r], dl + 1))


def _check(ops, dev, codes, y, sizes, F=16, refs=None):
    """Fit one ragged batch and compare every tree with the reference."""
    assert codes.shape[1] == 16 and len(y) == len(codes) >= max(sizes)
    if refs is None:
        refs = _reference(codes, y, sizes, F)
    out = _fit_multi(ops, dev, codes, y, _jobs(sizes, F), F)
    _assert_trees_equal(out, refs)


@pytest.fixture(scope="module")
def tier_refs(rand_data):
    """Reference trees of the tier-boundary batch, computed once."""
    codes, y = rand_data
    return _reference(codes, y, TIER_SIZES, 16)


def test_tier_boundaries(ops, dev, rand_data, tier_refs):
    codes, y = rand_data
    _check(ops, dev, codes, y, TIER_SIZES, refs=tier_refs)


def test_tier_boundaries_unstaged(ops, dev, rand_data, tier_refs,
                                  monkeypatch):
    """The same batch through mid_subtree_kernel<false>, which reads code
    rows from global memory instead of the LDS-staged copy."""
    monkeypatch.setenv("FLAKE16_MID_UNSTAGED", "1")
    codes, y = rand_data
    _check(ops, dev, codes, y, TIER_SIZES, refs=tier_refs)


@pytest.mark.parametrize("F", [1, 2, 7, 16])
def test_f_below_pad(ops, dev, rand_data, F):
    """Permutation length, F = 1 (no swap) and the pass-1 bound.  Columns
    >= F hold random data: a read past F changes a tree."""
    codes, y = rand_data
    _check(ops, dev, codes, y, [40, 64, 65, 300, 1100], F=F)


@pytest.mark.parametrize("n_const", [12, 14, 15, 16])
def test_constant_columns(ops, dev, rand_data, n_const):
    """The candidate walk skips constant features: it ends with fewer than
    max_features candidates (14, 15) or with none and a leaf (16)."""
    codes, y = rand_data
    codes = codes.copy()
    rng = np.random.RandomState(n_const)
    const_cols = rng.permutation(16)[:n_const]
    codes[:, const_cols] = (const_cols + 3).astype(np.uint8)
    _check(ops, dev, codes, y, [50, 64, 65, 700])


def test_constant_deep_in_subtree(ops, dev):
    """Sparse codes (the deep_data of test_gpu_forest_drain.py): columns
    become constant only deep inside a subtree."""
    rng = np.random.RandomState(7)
    n = 2048
    codes = ((rng.rand(n, 16) < 0.08)
             * rng.randint(1, 8, (n, 16))).astype(np.uint8)
    y = (rng.rand(n) < 0.3).astype(np.uint8)
    _check(ops, dev, codes, y, [64, 500, 2048])


def _tie_codes(name, n=700):
    rng = np.random.RandomState(5)
    if name == "duplicated_columns":
        # equal scores across candidates: strict > in permutation order
        return np.tile(rng.randint(0, 256, (n, 4)), (1, 4)).astype(np.uint8)
    if name == "binary":
        # many equal-score bins: the lowest bin wins
        return rng.randint(0, 2, (n, 16)).astype(np.uint8)
    if name == "byte_range_ends":
        # both ends of the byte range in the u16 unpacking
        return rng.choice([0, 254, 255], (n, 16)).astype(np.uint8)
    assert name == "across_bit_7"
    return rng.randint(127, 129, (n, 16)).astype(np.uint8)


@pytest.mark.parametrize("name", ["duplicated_columns", "binary",
                                  "byte_range_ends", "across_bit_7"])
def test_ties(ops, dev, name):
    codes = _tie_codes(name)
    y = (np.random.RandomState(6).rand(len(codes)) < 0.3).astype(np.uint8)
    _check(ops, dev, codes, y, [48, 64, 65, 700])


@pytest.mark.parametrize("labels", ["all_zero", "all_one", "one_positive"])
def test_labels(ops, dev, rand_data, labels):
    codes, _ = rand_data
    y = np.full(N_ROWS, labels == "all_one", dtype=np.uint8)
    if labels == "one_positive":
        y[37] = 1   # inside every prefix below
    _check(ops, dev, codes, y, [64, 65, 2048])


# ---------------------------------------------------------------------------
# The level band: nodes above 2048 samples.
# ---------------------------------------------------------------------------
BAND_ROWS = 5000
# 2304 = 9 x 256: 2304 and 2305 sit either side of a partition-tile edge;
# 4096 and up give several band levels.
BAND_SIZES = [2049, 2304, 2305, 4096, 4097, 5000]


@pytest.fixture(scope="module")
def band_data():
    """Random 0..255 codes in all 16 columns, about 30 % positives."""
    rng = np.random.RandomState(11)
    codes = rng.randint(0, 256, (BAND_ROWS, 16)).astype(np.uint8)
    y = (rng.rand(BAND_ROWS) < 0.3).astype(np.uint8)
    return codes, y


@pytest.fixture(scope="module")
def band_refs(band_data):
    """Reference trees of the band-size batch, computed once."""
    codes, y = band_data
    return _reference(codes, y, BAND_SIZES, 16)


def test_band_sizes(ops, dev, band_data, band_refs):
    codes, y = band_data
    _check(ops, dev, codes, y, BAND_SIZES, refs=band_refs)


def test_band_sizes_without_pools(ops, dev, band_data, band_refs,
                                  monkeypatch):
    """No node gets a histogram slot: 65..2048 children go to the mid
    kernel instead of coming back through hist_split_kernel with one."""
    monkeypatch.setenv("FLAKE16_HIST_SAVE_MIN", "1000000")
    codes, y = band_data
    _check(ops, dev, codes, y, BAND_SIZES, refs=band_refs)


@pytest.mark.parametrize("F", [1, 2, 7, 16])
def test_band_f_below_pad(ops, dev, band_data, F):
    """Columns >= F hold random data: a read past F changes a tree."""
    codes, y = band_data
    _check(ops, dev, codes, y, [4097], F=F)


@pytest.mark.parametrize("n_const", [12, 14, 15, 16])
def test_band_constant_columns(ops, dev, band_data, n_const):
    """As test_constant_columns; 16 leaves the root a single leaf, the
    no-candidate exit of both level kernels."""
    codes, y = band_data
    codes = codes.copy()
    rng = np.random.RandomState(n_const)
    const_cols = rng.permutation(16)[:n_const]
    codes[:, const_cols] = (const_cols + 3).astype(np.uint8)
    _check(ops, dev, codes, y, [BAND_ROWS])


@pytest.mark.parametrize("name", ["duplicated_columns", "binary",
                                  "byte_range_ends", "across_bit_7"])
def test_band_ties(ops, dev, name):
    """Strict > across duplicated columns and the lowest-bin rule in the
    level kernels."""
    codes = _tie_codes(name, BAND_ROWS)
    y = (np.random.RandomState(6).rand(BAND_ROWS) < 0.3).astype(np.uint8)
    _check(ops, dev, codes, y, [BAND_ROWS])


@pytest.mark.parametrize("labels", ["all_zero", "all_one", "one_positive"])
def test_band_labels(ops, dev, band_data, labels):
    """The leaf exit before the candidate walk (single-node trees for the
    first two)."""
    codes, _ = band_data
    y = np.full(BAND_ROWS, labels == "all_one", dtype=np.uint8)
    if labels == "one_positive":
        y[37] = 1
    _check(ops, dev, codes, y, [BAND_ROWS])
