"""GPU tests: k-NN and the balancing kernels on tied, duplicated and
offset data — the shape of the raw Flake16 feature table (integer counts,
units to ~1e6, many duplicate rows, many exactly equal distances).

The contract under test is the one of balance/__init__.knn_indices: fp64
feature-sequential distance, ties broken by lower candidate index, output
bit-identical on identical input bits.  Every reference is the numpy code
in balance/__init__.py and models/binning.py; every comparison is
assert_array_equal.

Both k-NN implementations are run: the default two-phase MFMA kernel
(fp32 filter -> fp64 re-rank, exact fallback scan for queries whose filter
may have dropped a contender) and the scalar kernel selected by
FLAKE16_NO_MFMA_KNN=1.  The number of queries the MFMA path sent to its
fallback is read from the `[knn] ... fallback=N` line that
FLAKE16_KNN_DEBUG=1 prints on stderr.

Data sets (float32, seeded, 16 columns):
  identical     every row the same random vector
  heavy_dup     12 distinct integer rows x 64 copies, shuffled: 63
                zero-distance others per query, more than the 4 x 12
                phase-1 pool holds -> every query must fall back
  light_dup     100 distinct integer rows x 6 copies, shuffled: the
                duplicates fit in the pool -> phase-2 index tie-break
  small_counts  integers 0..5 in 5 columns: many ties between distinct
                rows, a few repeated rows
  offset        1e6 + integers 0..50 (exact in fp32): squared distances
                <= 4e4 under squared norms ~1.6e13, so the fp32 expansion
                |q|^2+|c|^2-2q.c carries no information -> all fall back
  near_offset   1400 + integers 0..50: the error bound is of the order of
                the distance spread, so some queries fall back and some
                do not (parity only)
  mixed_scale   rounded log-normal columns, scales 1..1e6
  gauss         the continuous data of test_gpu_kernels (size sweep only)
"""

import functools
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PATHS = ("mfma", "scalar")
KS = (1, 3, 5, 8)


@pytest.fixture(scope="module")
def ops():
    from flake16_framework_amd.ops.backend import get_ops
    return get_ops()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# data sets
# ---------------------------------------------------------------------------
def _f32(X):
    X = np.ascontiguousarray(X, dtype=np.float32)
    assert X.shape[1] == 16
    return X


def _identical(n, seed=21):
    rng = np.random.RandomState(seed)
    return _f32(np.tile(rng.randn(16).astype(np.float32), (n, 1)))


def _dup(n, copies, hi, seed):
    assert n % copies == 0
    rng = np.random.RandomState(seed)
    distinct = rng.randint(0, hi, size=(n // copies, 16))
    assert len(np.unique(distinct, axis=0)) == n // copies
    X = np.repeat(distinct, copies, axis=0)
    return _f32(X[rng.permutation(n)])


def _heavy_dup(n=768, seed=22):
    return _dup(n, 64, 10000, seed)


def _light_dup(n=600, seed=23):
    return _dup(n, 6, 51, seed)


def _small_counts(n, seed=24):
    # 5 real columns, 11 of padding: 6^5 cells, so next to the many ties
    # between distinct rows a few rows repeat — with 16 real columns no
    # row would, and the k = 1 / identity-kept case would hold no tie
    rng = np.random.RandomState(seed)
    X = np.zeros((n, 16))
    X[:, :5] = rng.randint(0, 6, size=(n, 5))
    return _f32(X)


def _offset(n, seed=25):
    rng = np.random.RandomState(seed)
    X = _f32(1.0e6 + rng.randint(0, 51, size=(n, 16)))
    # exact in fp32, or the set would not test what it claims
    assert (X.astype(np.float64) >= 1.0e6).all()
    assert (X.astype(np.float64) == np.rint(X.astype(np.float64))).all()
    return X


def _near_offset(n, seed=27):
    # between `small_counts` and `offset`: slack ~ 1.2e-5 * 4 * 16 * 1425^2
    # ~ 1.6e3 is of the order of the spread of the nearest squared
    # distances (~2e3..4e3), so the error-bound decision falls on either
    # side from query to query
    rng = np.random.RandomState(seed)
    return _f32(1400.0 + rng.randint(0, 51, size=(n, 16)))


def _mixed_scale(n, seed=26):
    rng = np.random.RandomState(seed)
    scales = np.array([1.0, 10.0, 1.0e3, 1.0e5, 1.0e6])[np.arange(16) % 5]
    return _f32(np.rint(scales * rng.lognormal(0.0, 1.0, size=(n, 16))))


def _gauss(n, seed=3, sep=1.4):
    rng = np.random.RandomState(seed)
    y = rng.rand(n) < 0.25
    X = rng.randn(n, 16).astype(np.float32)
    X[y, :8] += sep
    return _f32(X)


BUILDERS = {
    "identical": _identical, "heavy_dup": _heavy_dup,
    "light_dup": _light_dup, "small_counts": _small_counts,
    "offset": _offset, "near_offset": _near_offset,
    "mixed_scale": _mixed_scale, "gauss": _gauss,
}
GRID_N = {"identical": 200, "heavy_dup": 768, "light_dup": 600,
          "small_counts": 600, "offset": 600, "near_offset": 600,
          "mixed_scale": 600}
# sets whose every query is proven (module docstring, knn_balance.hip) to
# take the MFMA path's exact fallback
ALL_FALLBACK = ("identical", "heavy_dup", "offset")


@functools.lru_cache(maxsize=None)
def _build(name, n):
    X = BUILDERS[name](n)
    assert X.shape == (n, 16) and X.dtype == np.float32
    X.setflags(write=False)
    return X


# ---------------------------------------------------------------------------
# CPU reference (shared, read-only)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(name, n, k, skip):
    from flake16_framework_amd.balance import knn_indices
    ref = knn_indices(_build(name, n), _build(name, n), k,
                      skip_identity=skip)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _dist(name, n):
    """fp64 squared distances in the reference's own operation order."""
    X = _build(name, n).astype(np.float64)
    d2 = np.zeros((n, n))
    for f in range(16):
        diff = X[:, f, None] - X[None, :, f]
        d2 = d2 + diff * diff
    d2.setflags(write=False)
    return d2


def _tie_at_k(name, n, k, skip):
    """Per query: is the k-th ranked reference distance equal to the
    (k+1)-th, i.e. does the index rule decide who is in the result?"""
    d2 = _dist(name, n)
    if skip:
        d2 = d2.copy()
        np.fill_diagonal(d2, np.inf)
    ds = np.sort(d2, axis=1)
    return ds[:, k - 1] == ds[:, k]


# ---------------------------------------------------------------------------
# device call
# ---------------------------------------------------------------------------
_KNN_LINE = re.compile(r"\[knn\] R=(\d+) n_seg=(\d+) k=(\d+) fallback=(\d+)")


def _knn(ops, dev, monkeypatch, capfd, path, X, k, skip, seg=None):
    """Run ops.knn (or ops.knn_segmented when seg offsets are given) on
    the requested path.  Returns (indices, fallback count); the count is
    None on the scalar path, which has no fallback."""
    if path == "scalar":
        monkeypatch.setenv("FLAKE16_NO_MFMA_KNN", "1")
    else:
        monkeypatch.delenv("FLAKE16_NO_MFMA_KNN", raising=False)
    monkeypatch.setenv("FLAKE16_KNN_DEBUG", "1")
    Xd = torch.from_numpy(np.array(X, dtype=np.float32, order="C")).to(dev)
    capfd.readouterr()
    if seg is None:
        got = ops.knn(Xd, k, skip)
    else:
        seg_d = torch.tensor(seg, dtype=torch.int32, device=dev)
        got = ops.knn_segmented(Xd, seg_d, k, skip)
    got = got.cpu().numpy()
    err = capfd.readouterr().err
    assert got.shape == (len(X), k) and got.dtype == np.int32
    lines = _KNN_LINE.findall(err)
    if path == "scalar":
        assert not lines, err
        return got, None
    assert len(lines) == 1, err
    R, n_seg, kk, fb = map(int, lines[0])
    assert (R, n_seg, kk) == (len(X), 1 if seg is None else len(seg) - 1, k)
    return got, fb


# ---------------------------------------------------------------------------
# parity grid, fallback count
# ---------------------------------------------------------------------------
class TestKnnTies:
    @pytest.mark.parametrize("path", PATHS)
    @pytest.mark.parametrize("skip", [True, False])
    @pytest.mark.parametrize("k", KS)
    @pytest.mark.parametrize("name", list(GRID_N))
    def test_parity_grid(self, ops, dev, monkeypatch, capfd, name, k, skip,
                         path):
        n = GRID_N[name]
        ref = _ref(name, n, k, skip)

        # the set still tests what it claims (checked on the reference)
        if name in ("identical", "heavy_dup", "light_dup"):
            if (name, k, skip) == ("light_dup", 5, True):
                # 6 copies leave exactly k = 5 zero-distance others, so no
                # tie can straddle rank k here; the tie of this case is
                # among the k results (their ORDER is the index rule's) and
                # shows in the plain distance matrix, query included
                assert _tie_at_k(name, n, k, False).all()
                assert (_dist(name, n)[np.arange(n)[:, None], ref] == 0).all()
            else:
                assert _tie_at_k(name, n, k, skip).all()
        elif name == "small_counts":
            assert _tie_at_k(name, n, k, skip).any()
        if name == "light_dup" and k == 8:
            # ... and that tie is between rows distinct from the query
            d2 = _dist(name, n)
            assert (d2[np.arange(n), ref[:, k - 1]] > 0).all()
        if name == "identical":
            # closed form, no reference needed
            want = np.empty((n, k), dtype=np.int64)
            for q in range(n):
                cand = [c for c in range(k + 1) if not (skip and c == q)]
                want[q] = cand[:k]
            np.testing.assert_array_equal(ref, want)

        got, fb = _knn(ops, dev, monkeypatch, capfd, path, _build(name, n),
                       k, skip)
        print(f"{name} n={n} k={k} skip={skip} {path}: fallback={fb}")
        np.testing.assert_array_equal(got, ref)
        if name == "identical":
            np.testing.assert_array_equal(got, want)

    @pytest.mark.parametrize("skip", [True, False])
    @pytest.mark.parametrize("k", KS)
    @pytest.mark.parametrize("name", ALL_FALLBACK)
    def test_fallback_taken_by_every_query(self, ops, dev, monkeypatch,
                                           capfd, name, k, skip):
        """Each of the 4 lanes of a query sees more than 12 candidates;
        equal (or, for `offset`, indistinguishable within the error
        bound) d32 values do not displace list entries, so they become
        discards no farther than `slack` from the pooled k-th value and
        the query is flagged.  The exact chain scan -> fill -> scatter ->
        fallback then produces the whole output."""
        n = GRID_N[name]
        got, fb = _knn(ops, dev, monkeypatch, capfd, "mfma",
                       _build(name, n), k, skip)
        print(f"{name} n={n} k={k} skip={skip}: fallback={fb} of {n}")
        np.testing.assert_array_equal(got, _ref(name, n, k, skip))
        assert fb == n


# ---------------------------------------------------------------------------
# size sweep: 16-candidate tile, 32-candidate iteration, 64-query block,
# 256-row scalar / fallback tile, each from both sides
# ---------------------------------------------------------------------------
SWEEP_N = (2, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 255, 256, 257)


class TestKnnSizes:
    @pytest.mark.parametrize("path", PATHS)
    @pytest.mark.parametrize("skip", [True, False])
    @pytest.mark.parametrize("n", SWEEP_N)
    @pytest.mark.parametrize("name", ["gauss", "small_counts"])
    def test_size_sweep(self, ops, dev, monkeypatch, capfd, name, n, skip,
                        path):
        k = min(5, n - 1) if skip else min(5, n)
        got, fb = _knn(ops, dev, monkeypatch, capfd, path, _build(name, n),
                       k, skip)
        print(f"{name} n={n} k={k} skip={skip} {path}: fallback={fb}")
        np.testing.assert_array_equal(got, _ref(name, n, k, skip))


# ---------------------------------------------------------------------------
# segmented
# ---------------------------------------------------------------------------
SEGMENTS = (("gauss", 70), ("identical", 300), ("gauss", 257),
            ("offset", 65), ("small_counts", 16), ("heavy_dup", 768),
            ("gauss", 9))


def _concat(segments):
    X = np.concatenate([_build(name, n) for name, n in segments])
    off = np.concatenate([[0], np.cumsum([n for _, n in segments])])
    return _f32(X), [int(o) for o in off]


class TestKnnSegmented:
    @pytest.mark.parametrize("path", PATHS)
    @pytest.mark.parametrize("k", [1, 3, 5])
    def test_segments_of_every_kind(self, ops, dev, monkeypatch, capfd, k,
                                    path):
        """Flagged queries in several segments, one fallback region wider
        than 256 (several blocks), segments with few or no flagged rows
        between flagged ones, every boundary off the tile multiples;
        outputs are segment-local."""
        X, off = _concat(SEGMENTS)
        got, fb = _knn(ops, dev, monkeypatch, capfd, path, X, k, True,
                       seg=off)
        alone = [_knn(ops, dev, monkeypatch, capfd, path,
                      X[off[s]:off[s + 1]], k, True)[0]
                 for s in range(len(SEGMENTS))]
        print(f"segmented k={k} {path}: fallback={fb} of {len(X)}")
        for s, (name, n) in enumerate(SEGMENTS):
            np.testing.assert_array_equal(
                got[off[s]:off[s + 1]], _ref(name, n, k, True),
                err_msg=f"segment {s} ({name} {n})")
        if path == "mfma":
            assert fb >= 300 + 65 + 768
        for s, (name, n) in enumerate(SEGMENTS):
            np.testing.assert_array_equal(
                got[off[s]:off[s + 1]], alone[s],
                err_msg=f"segment {s} ({name} {n}) vs stand-alone call")


# ---------------------------------------------------------------------------
# downstream balancing kernels on tied data
# ---------------------------------------------------------------------------
LABELLED = (("light_dup", 600), ("small_counts", 600), ("mixed_scale", 600))
LABELLED_SEGS = (("light_dup", 300), ("small_counts", 257),
                 ("mixed_scale", 130))


@functools.lru_cache(maxsize=None)
def _labels(name, n):
    """~25 % positives; in every third group of duplicate rows the two
    lowest-index copies get opposite labels.  Those two are each other's
    nearest neighbour (distance 0, lowest index), i.e. a Tomek link at
    distance zero."""
    X = _build(name, n)
    rng = np.random.RandomState(1000 + n)
    y = (rng.rand(n) < 0.25).astype(np.uint8)
    _, inv = np.unique(X, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    for g in range(0, int(inv.max()) + 1, 3):
        m = np.flatnonzero(inv == g)
        if len(m) >= 2:
            y[m[0]], y[m[1]] = 1, 0
    assert 0.15 < y.mean() < 0.35
    y.setflags(write=False)
    return y


def _maj(y):
    return 1 if int(y.sum()) > len(y) - int(y.sum()) else 0


def _check_zero_links(name, n):
    """light_dup must contain mutual nearest pairs at distance zero with
    opposite labels."""
    if name != "light_dup":
        return
    y = _labels(name, n)
    nn1 = _ref(name, n, 1, True)[:, 0]
    i = np.arange(n)
    link = (nn1[nn1] == i) & (y != y[nn1]) & (_dist(name, n)[i, nn1] == 0)
    assert link.any()


def _enn_check(ops, dev, X, y, nn):
    from flake16_framework_amd.balance import enn_mask
    yd = torch.from_numpy(np.array(y)).to(dev)
    nn_d = torch.from_numpy(np.ascontiguousarray(nn)).to(dev)
    for clean_all in (False, True):
        ref = enn_mask(X, y, "all" if clean_all else "auto")
        assert not ref.all()            # something is removed
        got = ops.enn_keep(yd, nn_d, 3, _maj(y), clean_all)
        np.testing.assert_array_equal(got.cpu().numpy().astype(bool), ref)


def _tomek_check(ops, dev, X, y, nn1):
    from flake16_framework_amd.balance import tomek_links_mask
    yd = torch.from_numpy(np.array(y)).to(dev)
    nn_d = torch.from_numpy(np.ascontiguousarray(nn1[:, 0])).to(dev)
    for remove_all in (False, True):
        ref = tomek_links_mask(X, y, "all" if remove_all else "auto")
        assert not ref.all()            # at least one link
        got = ops.tomek_keep(yd, nn_d, _maj(y), remove_all)
        np.testing.assert_array_equal(got.cpu().numpy().astype(bool), ref)


class TestBalancingOnTies:
    """The k-NN indices are compared with the reference BEFORE they are
    handed to the next kernel: a wrong index may be -1 or out of range,
    and a kernel that dereferences it would fault instead of failing."""

    @pytest.mark.parametrize("path", PATHS)
    @pytest.mark.parametrize("name,n", LABELLED)
    def test_enn(self, ops, dev, monkeypatch, capfd, name, n, path):
        X, y = _build(name, n), _labels(name, n)
        nn, _ = _knn(ops, dev, monkeypatch, capfd, path, X, 3, True)
        np.testing.assert_array_equal(nn, _ref(name, n, 3, True))
        _enn_check(ops, dev, X, y, nn)

    @pytest.mark.parametrize("path", PATHS)
    @pytest.mark.parametrize("name,n", LABELLED)
    def test_tomek(self, ops, dev, monkeypatch, capfd, name, n, path):
        X, y = _build(name, n), _labels(name, n)
        _check_zero_links(name, n)
        nn1, _ = _knn(ops, dev, monkeypatch, capfd, path, X, 1, True)
        np.testing.assert_array_equal(nn1, _ref(name, n, 1, True))
        _tomek_check(ops, dev, X, y, nn1)

    @pytest.mark.parametrize("path", PATHS)
    @pytest.mark.parametrize("name,n", LABELLED)
    def test_smote(self, ops, dev, monkeypatch, capfd, name, n, path):
        from flake16_framework_amd.balance import knn_indices, smote
        X, y = _build(name, n), _labels(name, n)
        Xb_ref, yb_ref = smote(X, y, 0, 77)

        n1 = int(y.sum())
        n0 = n - n1
        min_label = 1 if n1 < n0 else 0
        min_rows = np.flatnonzero(y == min_label).astype(np.int32)
        k = min(5, len(min_rows) - 1)
        n_new = abs(n0 - n1)
        assert k == 5 and n_new > 0

        X_min = _f32(X[min_rows])
        nn, _ = _knn(ops, dev, monkeypatch, capfd, path, X_min, k, True)
        np.testing.assert_array_equal(
            nn, knn_indices(X_min, X_min, k, skip_identity=True))

        X_new = ops.smote_interpolate(
            torch.from_numpy(np.array(X)).to(dev),
            torch.from_numpy(min_rows).to(dev),
            torch.from_numpy(nn).to(dev), n_new, 0, 77)
        np.testing.assert_array_equal(X_new.cpu().numpy(), Xb_ref[n:])
        assert (yb_ref[n:] == min_label).all()

    @pytest.mark.parametrize("path", PATHS)
    @pytest.mark.parametrize("kind", ["enn", "tomek"])
    def test_segmented_enn_tomek(self, ops, dev, monkeypatch, capfd, kind,
                                 path):
        """The fold-batched form of engine/hip_cell._clean_folds: one
        segmented k-NN, then the mask kernel per segment on segment-local
        indices."""
        k = 3 if kind == "enn" else 1
        X, off = _concat(LABELLED_SEGS)
        nn, _ = _knn(ops, dev, monkeypatch, capfd, path, X, k, True, seg=off)
        for s, (name, n) in enumerate(LABELLED_SEGS):
            np.testing.assert_array_equal(
                nn[off[s]:off[s + 1]], _ref(name, n, k, True),
                err_msg=f"segment {s} ({name} {n})")
        for s, (name, n) in enumerate(LABELLED_SEGS):
            Xs, ys = _build(name, n), _labels(name, n)
            nn_s = nn[off[s]:off[s + 1]]
            if kind == "enn":
                _enn_check(ops, dev, Xs, ys, nn_s)
            else:
                _check_zero_links(name, n)
                _tomek_check(ops, dev, Xs, ys, nn_s)


# ---------------------------------------------------------------------------
# bin encoding on discrete columns
# ---------------------------------------------------------------------------
def _discrete_matrix(n=700, seed=31):
    """6 real feature columns (the other 10 are padding):
      0 constant                      -> zero cuts
      1 two-valued                    -> one cut
      2 exactly 256 distinct integers -> 255 midpoint cuts, codes to 255
      3 > 256 distinct values         -> quantile cuts that ARE data values
      4 integers 0..5
      5 1e6 + integers 0..50
    """
    rng = np.random.RandomState(seed)
    X = np.zeros((n, 16), dtype=np.float32)
    X[:, 0] = 7.0
    X[:, 1] = np.where(rng.rand(n) < 0.3, 3.0, 11.0)
    X[:, 2] = rng.permutation(
        np.concatenate([np.arange(256), rng.randint(0, 256, n - 256)]))
    X[:, 3] = np.rint(1.0e3 * rng.lognormal(0.0, 1.0, n))
    X[:, 4] = rng.randint(0, 6, n)
    X[:, 5] = 1.0e6 + rng.randint(0, 51, n)
    return X


def _dev_bin_codes(ops, dev, X, cuts, F):
    flat = np.concatenate(cuts).astype(np.float32)
    off = np.zeros(17, dtype=np.int32)
    off[1:17] = np.cumsum([len(c) for c in cuts] + [0] * (16 - len(cuts)))
    got = ops.bin_codes(torch.from_numpy(X).to(dev),
                        torch.from_numpy(flat).to(dev),
                        torch.from_numpy(off).to(dev), F)
    return got.cpu().numpy()


class TestBinCodesDiscrete:
    F = 6

    def _cuts(self):
        from flake16_framework_amd.models.binning import compute_bin_cuts
        X = _discrete_matrix()
        cuts = compute_bin_cuts(X[:, :self.F])
        # the columns are what they claim to be
        assert [len(c) for c in cuts[:3]] == [0, 1, 255]
        assert len(np.unique(X[:, 3])) > 256
        assert np.isin(cuts[3], X[:, 3]).all()
        return X, cuts

    def test_fit_matrix(self, ops, dev):
        from flake16_framework_amd.models.binning import bin_codes
        X, cuts = self._cuts()
        ref = bin_codes(X[:, :self.F], cuts)
        assert ref[:, 0].max() == 0 and set(ref[:, 1]) == {0, 1}
        assert ref[:, 2].min() == 0 and ref[:, 2].max() == 255
        got = _dev_bin_codes(ops, dev, X, cuts, self.F)
        np.testing.assert_array_equal(got[:, :self.F], ref)
        np.testing.assert_array_equal(got[:, self.F:], 0)

    def test_other_matrix_with_saved_cuts(self, ops, dev):
        """The `detect` situation: new rows encoded with the cuts of the
        fit matrix — values below the first cut, above the last cut,
        exactly on a cut, and one float step to either side of it."""
        from flake16_framework_amd.models.binning import bin_codes
        _, cuts = self._cuts()
        rng = np.random.RandomState(32)
        n2 = 800
        X2 = np.zeros((n2, 16), dtype=np.float32)
        for f, c in enumerate(cuts):
            if len(c) == 0:
                pool = np.array([-1.0, 7.0, 1.0e9], dtype=np.float32)
            else:
                pool = np.concatenate([
                    [c[0] - 1.0e3, c[-1] + 1.0e3], c,
                    np.nextafter(c, np.float32(-np.inf)),
                    np.nextafter(c, np.float32(np.inf))]).astype(np.float32)
            assert len(pool) <= n2
            col = rng.choice(pool, n2)
            col[:len(pool)] = pool                    # every edge at least once
            X2[:, f] = col
        ref = bin_codes(X2[:, :self.F], cuts)
        for f, c in enumerate(cuts):
            assert ref[:, f].min() == 0 and ref[:, f].max() == len(c)
        got = _dev_bin_codes(ops, dev, X2, cuts, self.F)
        np.testing.assert_array_equal(got[:, :self.F], ref)
        np.testing.assert_array_equal(got[:, self.F:], 0)
