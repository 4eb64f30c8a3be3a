"""interact on the numpy backend: SHAP interaction values against the
Shapley interaction index by subset enumeration, a tree worked by hand,
the invariants on fitted detectors, degenerate forests, explain's fields,
the JSON artifact and the CLI."""

import itertools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_explain import (
    CONFIGS, N_TREES, _as_tests, _chain_desc, _codes, _detector, _first,
    _random_desc, _spine_desc, _tree,
)

from flake16_framework_amd.dataset.synthetic import make_synthetic_tests

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _interact(det, codes):
    from flake16_framework_amd.engine.interact import interact
    return interact(det, tests=_as_tests(codes, det.feature_cols),
                    backend="ref")


def _off_diagonal(a):
    F = a.shape[1]
    return a[:, ~np.eye(F, dtype=bool)]


# -- 1. against the Shapley interaction index ---------------------------------
def _expect(tree, row, S, node=0):
    """Path-dependent expectation of the class-1 leaf value with the
    features of S known: follow the row on them, average by cover on the
    others."""
    f = int(tree.feature[node])
    cover = tree.count0 + tree.count1
    if f < 0:
        return tree.count1[node] / cover[node]
    lt, rt = int(tree.left[node]), int(tree.right[node])
    if f in S:
        nxt = lt if row[f] <= tree.split_bin[node] else rt
        return _expect(tree, row, S, nxt)
    return (cover[lt] * _expect(tree, row, S, lt)
            + cover[rt] * _expect(tree, row, S, rt)) / cover[node]


def _brute_interactions(det, codes):
    """Off-diagonal interaction values by subset enumeration; the
    diagonal stays 0."""
    F, trees = det.n_features, det.trees()
    out = np.zeros((len(codes), F, F))
    for i, row in enumerate(codes):
        v = {}
        for size in range(F + 1):
            for S in itertools.combinations(range(F), size):
                v[frozenset(S)] = sum(
                    _expect(t, row, S) for t in trees) / len(trees)
        for g, f in itertools.permutations(range(F), 2):
            rest = [k for k in range(F) if k not in (g, f)]
            for size in range(len(rest) + 1):
                wgt = (math.factorial(size) * math.factorial(F - size - 2)
                       / (2 * math.factorial(F - 1)))
                for S in itertools.combinations(rest, size):
                    S = frozenset(S)
                    out[i, g, f] += wgt * (v[S | {g, f}] - v[S | {g}]
                                           - v[S | {f}] + v[S])
    return out


@pytest.mark.parametrize("F", [3, 6])
def test_brute_force_hand_built(F):
    # the forests of test_explain.test_brute_force_hand_built
    rng = np.random.RandomState(40 + F)
    trees = [_tree(_random_desc(F, rng, max_depth=7)) for _ in range(2)]
    feats = list(range(F)) + [0, F - 1, 0]
    trees.append(_tree(_spine_desc(
        feats, [int(s) for s in rng.randint(20, 230, size=len(feats))],
        [int(s) for s in rng.randint(0, 2, size=len(feats))], rng)))
    trees.append(_tree(_chain_desc(1, rng)))
    det = _detector(trees, F)
    codes = _codes(12, F, rng)
    assert (codes[0] == 0).all() and (codes[1] == 255).all()
    got = _interact(det, codes)["interactions"]
    want = _brute_interactions(det, codes)
    assert got.shape == (12, F, F) and got.dtype == np.float64
    gap = np.abs(_off_diagonal(got) - _off_diagonal(want)).max()
    print(f"F={F}: largest off-diagonal difference {gap:.3e}, largest "
          f"|off-diagonal| {np.abs(_off_diagonal(want)).max():.3e}")
    assert gap <= 1e-9
    assert np.abs(_off_diagonal(want)).max() > 1e-3


# -- 2. one tree worked by hand -------------------------------------------------
def _two_level(leaves):
    """Root on f0 at 100, both children on f1 at 50; leaves in the order
    (f0 low, f1 low), (low, high), (high, low), (high, high)."""
    ll, lh, hl, hh = (("leaf", c0, c1) for c0, c1 in leaves)
    return _tree((0, 100, (1, 50, ll, lh), (1, 50, hl, hh)))


def test_one_tree_by_hand():
    leaves = [(3, 7), (12, 8), (1, 4), (20, 15)]      # (cnt0, cnt1)
    det = _detector([_two_level(leaves)], 2)
    codes = np.array([[0, 0], [0, 255], [255, 0], [255, 255], [100, 50],
                      [101, 51]])
    res = _interact(det, codes)
    cover = np.array([c0 + c1 for c0, c1 in leaves], dtype=np.float64)
    value = np.array([c1 / (c0 + c1) for c0, c1 in leaves])
    for row, got in zip(codes, res["interactions"]):
        a, b = int(row[0] > 100), int(row[1] > 50)
        v01 = value[2 * a + b]
        # f0 known: its child's two leaves by their covers
        pair = [2 * a, 2 * a + 1]
        v0 = (cover[pair] * value[pair]).sum() / cover[pair].sum()
        # f1 known: leaf b of either child by the children's covers
        child = np.array([cover[:2].sum(), cover[2:].sum()])
        v1 = (child * value[[b, 2 + b]]).sum() / child.sum()
        v_none = (cover * value).sum() / cover.sum()
        want = (v01 - v0 - v1 + v_none) / 2
        assert abs(want) > 1e-3
        # a few dozen fp64 operations on values below 1
        assert abs(got[0, 1] - want) <= 1e-12
        assert abs(got[1, 0] - want) <= 1e-12


def test_additive_tree_has_no_interaction():
    # equal covers, cnt1 = a[f0 side] + b[f1 side]
    a, b, cover = (2, 6), (4, 8), 20
    leaves = [(cover - a[i] - b[j], a[i] + b[j])
              for i in range(2) for j in range(2)]
    det = _detector([_two_level(leaves)], 2)
    codes = np.array([[0, 0], [0, 255], [255, 0], [255, 255], [100, 51]])
    res = _interact(det, codes)
    assert np.abs(_off_diagonal(res["interactions"])).max() <= 1e-15
    assert np.ptp(res["phi"], axis=0).min() > 1e-3     # phi is not zero


# -- 3. invariants on fitted detectors ---------------------------------------------
@pytest.fixture(scope="module")
def train_tests():
    return make_synthetic_tests(n_tests=300, seed=2)


@pytest.fixture(scope="module")
def fitted(train_tests):
    from flake16_framework_amd.engine.detector import fit_detector
    return {name: fit_detector(keys, tests=train_tests, backend="ref",
                               n_trees=N_TREES)
            for name, keys in CONFIGS.items()}


def _check_invariants(res):
    phi, inter = res["phi"], res["interactions"]
    assert np.abs(inter.sum(axis=2) - phi).max() <= 1e-12
    gap = res["base_value"] + inter.sum(axis=(1, 2)) - res["proba"]
    assert np.abs(gap).max() <= 1e-9
    # the two triangles come from different reduced paths
    assert np.abs(inter - inter.transpose(0, 2, 1)).max() <= 1e-9


@pytest.mark.parametrize("name", list(CONFIGS))
def test_invariants_fitted(name, fitted, train_tests):
    from flake16_framework_amd.engine.explain import explain
    from flake16_framework_amd.engine.interact import interact
    det = fitted[name]
    res = interact(det, tests=train_tests, backend="ref")
    F = det.n_features
    assert res["interactions"].shape == (300, F, F)
    assert res["interactions"].dtype == np.float64
    _check_invariants(res)
    assert np.abs(_off_diagonal(res["interactions"])).max() > 1e-3
    # 5. explain's fields, bit for bit
    want = explain(det, tests=train_tests, backend="ref")
    assert sorted(res) == sorted([*want, "interactions"])
    for key in ("proba", "pred", "phi", "projects", "nodeids"):
        np.testing.assert_array_equal(res[key], want[key])
    assert res["base_value"] == want["base_value"]
    assert res["feature_names"] == want["feature_names"]


# -- 4. degenerate forests -----------------------------------------------------------
def test_forest_of_root_leaves():
    det = _detector([_tree(("leaf", 4, 3)), _tree(("leaf", 1, 9))], 16)
    res = _interact(det, _codes(5, 16, np.random.RandomState(0)))
    assert res["interactions"].shape == (5, 16, 16)
    assert (res["interactions"] == 0.0).all()


def test_one_feature_chain():
    rng = np.random.RandomState(1)
    det = _detector([_tree(_chain_desc(1, rng))], 16)
    res = _interact(det, _codes(40, 16, rng))
    inter = res["interactions"]
    assert (_off_diagonal(inter) == 0.0).all()
    np.testing.assert_array_equal(
        np.diagonal(inter, axis1=1, axis2=2), res["phi"])
    assert np.ptp(res["phi"][:, 1]) > 1e-3


def test_sixteen_element_leaf():
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    rng = np.random.RandomState(16)
    perm = [int(f) for f in rng.permutation(16)]
    det = _detector([_tree(_spine_desc(
        perm, [100] * 16, [1] * 16, rng))], 16)
    assert np.diff(build_merged_paths(det).leaf_off).max() == 16
    codes = _codes(6, 16, rng)
    codes[2] = 101                      # reaches the end of the spine
    res = _interact(det, codes)
    assert np.isfinite(res["interactions"]).all()
    _check_invariants(res)
    assert np.abs(_off_diagonal(res["interactions"])).max() > 0


def test_no_rows(fitted):
    from flake16_framework_amd.engine.interact import interact
    for name, F in (("nod", 16), ("pca", 7)):
        for tests in ({}, {"proj": {}}):
            res = interact(fitted[name], tests=tests, backend="ref")
            assert res["interactions"].shape == (0, F, F)
            assert res["interactions"].dtype == np.float64
            assert res["phi"].shape == (0, F) and len(res["proba"]) == 0


# -- 6. the artifact -------------------------------------------------------------------
def test_write_interactions_round_trip(fitted, train_tests, tmp_path):
    from flake16_framework_amd.engine.interact import write_interactions
    det = fitted["pca"]
    rows = _first(train_tests, 30)
    path, npy = tmp_path / "in.json", tmp_path / "in.npy"
    res = write_interactions(det, tests=rows, out_file=str(path), top=4,
                             matrix_out=str(npy), backend="ref")
    inter, names = res["interactions"], res["feature_names"]
    with open(path) as fd:
        out = json.load(fd)
    assert list(out) == ["feature_names", "base_value", "mean_abs", "pairs",
                         "tests"]
    assert out["feature_names"] == list(names)
    assert out["base_value"] == res["base_value"]
    np.testing.assert_array_equal(out["mean_abs"], np.abs(inter).mean(axis=0))
    assert list(out["tests"]) == list(rows)
    assert [nid for proj in out["tests"].values() for nid in proj] == \
        list(res["nodeids"])
    flat = [v for proj in out["tests"].values() for v in proj.values()]
    np.testing.assert_array_equal([r[0] for r in flat], res["proba"])
    np.testing.assert_array_equal([r[1] for r in flat], res["pred"])
    np.testing.assert_array_equal(
        [r[2] for r in flat], np.diagonal(inter, axis1=1, axis2=2))
    sym = inter + inter.transpose(0, 2, 1)
    for i, r in enumerate(flat):
        assert len(r) == 4 and len(r[3]) == 4
        for g, f, value in r[3]:
            assert g < f and value == sym[i, g, f]
        size = [abs(p[2]) for p in r[3]]
        assert size == sorted(size, reverse=True)
        others = np.abs(sym[i][np.triu_indices(7, k=1)])
        assert (np.sort(others)[::-1][:4] == size).all()
    # all 21 pairs, by name, descending
    assert len(out["pairs"]) == 21
    gs, fs = np.triu_indices(7, k=1)
    mean = np.zeros((7, 7))             # summed test by test, as [M, 21]
    mean[gs, fs] = np.abs(sym[:, gs, fs]).mean(axis=0)
    idx = {n: k for k, n in enumerate(names)}
    for ng, nf, value in out["pairs"]:
        assert idx[ng] < idx[nf] and value == mean[idx[ng], idx[nf]]
    size = [p[2] for p in out["pairs"]]
    assert size == sorted(size, reverse=True)
    np.testing.assert_array_equal(np.load(npy), inter)


def test_pair_order_with_ties():
    from flake16_framework_amd.engine.interact import top_pairs
    F = 4                               # pairs 01 02 03 12 13 23
    inter = np.zeros((3, F, F))
    # test 0: |value| 2 for (0, 3), (1, 2) and (2, 3), 1 for (0, 1); the
    # sign does not count and the halves may sit in either triangle
    inter[0, 0, 3], inter[0, 3, 0] = 0.5, 1.5
    inter[0, 2, 1] = -2.0
    inter[0, 2, 3], inter[0, 3, 2] = 1.0, 1.0
    inter[0, 0, 1] = 1.0
    inter[0, 1, 1] = 99.0               # the diagonal is no pair
    # test 1: all equal, so (g, f) order; test 2: all zero likewise
    inter[1] = 0.25
    every = [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    got = top_pairs(inter, 6)
    assert got[0] == [[0, 3, 2.0], [1, 2, -2.0], [2, 3, 2.0], [0, 1, 1.0],
                      [0, 2, 0.0], [1, 3, 0.0]]
    assert got[1] == [[g, f, 0.5] for g, f in every]
    assert got[2] == [[g, f, 0.0] for g, f in every]
    assert [r[:2] for r in top_pairs(inter, 2)] == \
        [got[0][:2], got[1][:2], got[2][:2]]
    assert top_pairs(inter, 0) == [[], [], []]


def test_top_range(fitted, train_tests, tmp_path):
    from flake16_framework_amd.engine.interact import write_interactions
    det = fitted["pca"]                 # F = 7: 21 pairs
    rows = _first(train_tests, 3)
    path = tmp_path / "in.json"
    for top in (0, 21):
        write_interactions(det, tests=rows, out_file=str(path), top=top,
                           backend="ref")
        with open(path) as fd:
            out = json.load(fd)
        for proj in out["tests"].values():
            for r in proj.values():
                assert len(r[3]) == top
    for top in (-1, 22, 2.5, None):
        with pytest.raises(ValueError, match="top"):
            write_interactions(det, tests=rows, out_file=str(path), top=top,
                               backend="ref")


def test_cli_interact(train_tests, tmp_path):
    from flake16_framework_amd.constants import (
        DETECTOR_FILE, INTERACTIONS_FILE, TESTS_FILE,
    )
    from flake16_framework_amd.engine.detector import Detector
    from flake16_framework_amd.engine.interact import interact
    assert INTERACTIONS_FILE == "interactions.json"
    with open(tmp_path / TESTS_FILE, "w") as fd:
        json.dump(train_tests, fd)
    rows = _first(make_synthetic_tests(n_tests=257, seed=5), 40)
    with open(tmp_path / "other.json", "w") as fd:
        json.dump(rows, fd)

    def run(*args):
        done = subprocess.run(
            [sys.executable, os.path.join(REPO, "experiment.py"), *args],
            cwd=tmp_path, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        return done.stdout.strip()

    run("fit", "--config", "nod", "--backend", "ref", "--n-trees", "3")
    line = run("interact", "--backend", "ref", "--tests-file", "other.json",
               "--top", "2", "--matrix-out", "m.npy")
    assert line.startswith(f"wrote {INTERACTIONS_FILE} (40 tests")
    with open(tmp_path / INTERACTIONS_FILE) as fd:
        out = json.load(fd)
    res = interact(Detector.load(str(tmp_path / DETECTOR_FILE)), tests=rows,
                   backend="ref")
    np.testing.assert_array_equal(np.load(tmp_path / "m.npy"),
                                  res["interactions"])
    for ng, nf, value in out["pairs"][:3]:
        assert f"{ng} x {nf} {value:.4f}" in line
    flat = [v for proj in out["tests"].values() for v in proj.values()]
    assert all(len(r[3]) == 2 for r in flat)
    np.testing.assert_array_equal(
        [r[2] for r in flat],
        np.diagonal(res["interactions"], axis1=1, axis2=2))

    bad = subprocess.run(
        [sys.executable, os.path.join(REPO, "experiment.py"), "interact",
         "--backend", "ref", "--tests-file", "other.json", "--top", "121"],
        cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "top takes 0..120" in bad.stderr
