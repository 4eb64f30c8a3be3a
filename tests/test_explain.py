"""explain on the numpy backend: the merged-path table, the attributions
against brute-force Shapley values and the TreeSHAP recursion, additivity,
refusals, the JSON artifact and the CLI."""

import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.constants import (
    FEATURE_NAMES, FLAKEFLAGGER_COLUMNS,
)
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
from flake16_framework_amd.models.binning import bin_codes
from flake16_framework_amd.models.forest_ref import Tree, canonicalize_tree
from flake16_framework_amd.models.treeshap_ref import (
    brute_force_shap, forest_shap,
)
from flake16_framework_amd.preprocess import transform_preprocessing

N_TREES = 12
CHAIN_DEPTH = 24
PCA_KEYS = ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN", "Random Forest")
CONFIGS = {"nod": SHAP_CONFIGS[0], "od": SHAP_CONFIGS[1], "pca": PCA_KEYS}


# -- hand-built trees with consistent counts --------------------------------
# A tree is described as ("leaf", cnt0, cnt1) or (feature, split, left,
# right); internal counts are the sums of their children's.
def _tree(desc):
    rows = []

    def add(d):
        i = len(rows)
        rows.append(None)
        if d[0] == "leaf":
            rows[i] = [-1, 0, -1, -1, float(d[1]), float(d[2])]
            return i
        lt, rt = add(d[2]), add(d[3])
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


def _random_desc(F, rng, depth=0, max_depth=6):
    if depth == max_depth or (depth > 0 and rng.rand() < 0.25):
        return _leaf(rng)
    return (int(rng.randint(F)), int(rng.randint(0, 255)),
            _random_desc(F, rng, depth + 1, max_depth),
            _random_desc(F, rng, depth + 1, max_depth))


def _chain_desc(f, rng):
    """Level d sends code <= 10 d to a leaf, the rest one level down."""
    desc = _leaf(rng)
    for d in range(CHAIN_DEPTH - 1, -1, -1):
        desc = (f, 10 * d, _leaf(rng), desc)
    return desc


def _spine_desc(feats, splits, sides, rng):
    """One long path: at step k the path continues on side sides[k] of a
    split of feats[k] at splits[k]; the other child is a leaf."""
    desc = _leaf(rng)
    for f, s, side in reversed(list(zip(feats, splits, sides))):
        desc = (f, s, _leaf(rng), desc) if side else (f, s, desc, _leaf(rng))
    return desc


def _detector(trees, F):
    """Spec None, 255 cuts k + 0.5 per feature: an integer input 0..255 is
    its own code."""
    from flake16_framework_amd.engine.detector import assemble_detector
    cols = tuple(range(16)) if F == 16 else FLAKEFLAGGER_COLUMNS[:F]
    params = {"spec": None, "mean": np.zeros(F), "scale": np.ones(F),
              "pca_mean": np.zeros(F), "W": np.eye(F)}
    cuts = [np.arange(255, dtype=np.float32) + 0.5 for _ in range(F)]
    return assemble_detector(
        ("NOD", "Flake16", "None", "None", "Random Forest"), 2, cols,
        params, cuts, trees, len(trees), 0, 100)


def _as_tests(codes, cols):
    rows = {}
    for i, row in enumerate(codes):
        full = [-7.0] * 16
        for j, c in enumerate(cols):
            full[c] = float(row[j])
        rows[f"t{i:04d}"] = [0, 0, *full]
    return {"proj": rows}


def _codes(m, F, rng):
    codes = rng.randint(0, 256, size=(m, F))
    codes[0], codes[1] = 0, 255
    return codes


def _explain(det, codes):
    from flake16_framework_amd.engine.explain import explain
    return explain(det, tests=_as_tests(codes, det.feature_cols),
                   backend="ref")


# -- 1. the merged-path table ------------------------------------------------
def test_root_leaf():
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    det = _detector([_tree(("leaf", 4, 3))], 16)
    p = build_merged_paths(det)
    assert p.n_leaves == 1 and p.n_elements == 0
    np.testing.assert_array_equal(p.leaf_off, [0, 0])
    np.testing.assert_array_equal(p.tree_leaf_off, [0, 1])
    res = _explain(det, _codes(5, 16, np.random.RandomState(0)))
    assert res["phi"].shape == (5, 16) and (res["phi"] == 0.0).all()
    assert res["base_value"] == 3.0 / 7.0
    np.testing.assert_array_equal(res["proba"], np.full(5, 3.0 / 7.0))


def test_chain_merges_into_one_element():
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    rng = np.random.RandomState(1)
    det = _detector([_tree(_chain_desc(1, rng))], 16)
    p = build_merged_paths(det)
    tree = det.trees()[0]
    cover = tree.count0 + tree.count1
    assert p.n_leaves == CHAIN_DEPTH + 1
    np.testing.assert_array_equal(np.diff(p.leaf_off), 1)   # one element each
    assert (p.feature == 1).all()
    assert (np.diff(p.leaf_node) > 0).all()                 # ascending ids
    seen = set()
    for leaf in range(p.n_leaves):
        # walk the tree to the leaf, narrowing by hand
        node, lo, hi, z = 0, -1, 255, None
        target = int(p.leaf_node[leaf])
        while node != target:
            # canonical chain: the left child is the leaf, the right the
            # next level (or the last leaf)
            lt, rt = int(tree.left[node]), int(tree.right[node])
            s = int(tree.split_bin[node])
            if target == lt:
                nxt, hi = lt, min(hi, s)
            else:
                nxt, lo = rt, max(lo, s)
            r = cover[nxt] / cover[node]
            z = r if z is None else z * r
            node = nxt
        (f, elo, ehi, ez), = p.elements(leaf)
        assert (elo, ehi) == (lo, hi) and ez == z
        assert p.leaf_value[leaf] == tree.count1[target] / cover[target]
        seen.add((lo, hi))
    want = {(10 * (d - 1) if d else -1, 10 * d) for d in range(CHAIN_DEPTH)}
    want.add((10 * (CHAIN_DEPTH - 1), 255))
    assert seen == want


@pytest.mark.parametrize("F", [16, 7])
def test_all_features_then_repeats(F):
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    rng = np.random.RandomState(F)
    perm = [int(f) for f in rng.permutation(F)]
    feats = perm + [perm[2], perm[0], perm[2]]
    splits = [100] * F + [150, 40, 120]
    sides = [1] * F + [1, 0, 0]     # right, ..., right, right, left, left
    det = _detector([_tree(_spine_desc(feats, splits, sides, rng))], F)
    p = build_merged_paths(det)
    n_el = np.diff(p.leaf_off)
    assert n_el.max() == F
    deepest = [leaf for leaf in range(p.n_leaves) if n_el[leaf] == F]
    for leaf in deepest:
        assert [e[0] for e in p.elements(leaf)] == perm  # first appearance
    # the leaf at the end of the spine: perm[2] in (150, 255] cut to
    # (150, 120] -> empty, perm[0] in (100, 40] -> empty
    tree = det.trees()[0]
    node = 0
    for side in sides:
        node = int(tree.right[node] if side else tree.left[node])
    end, = [leaf for leaf in deepest if p.leaf_node[leaf] == node]
    by_feat = {e[0]: e for e in p.elements(end)}
    assert by_feat[perm[2]][1:3] == (150, 120)
    assert by_feat[perm[0]][1:3] == (100, 40)
    assert by_feat[perm[1]][1:3] == (100, 255)
    cover = tree.count0 + tree.count1
    prod = np.prod([e[3] for e in p.elements(end)])
    np.testing.assert_allclose(
        prod, cover[int(p.leaf_node[end])] / cover[0], rtol=1e-13)


# -- 2. against brute-force Shapley values ------------------------------------
def _brute(det, codes):
    """Class-1 forest attributions by subset enumeration."""
    F = det.n_features
    out = np.zeros((len(codes), F))
    for tree in det.trees():
        for i, row in enumerate(codes):
            out[i] -= brute_force_shap(tree, row, F)
    return out / det.n_trees


@pytest.mark.parametrize("F", [3, 6])
def test_brute_force_hand_built(F):
    rng = np.random.RandomState(40 + F)
    trees = [_tree(_random_desc(F, rng, max_depth=7)) for _ in range(2)]
    feats = list(range(F)) + [0, F - 1, 0]
    trees.append(_tree(_spine_desc(
        feats, [int(s) for s in rng.randint(20, 230, size=len(feats))],
        [int(s) for s in rng.randint(0, 2, size=len(feats))], rng)))
    trees.append(_tree(_chain_desc(1, rng)))
    det = _detector(trees, F)
    # the random trees do repeat a feature on a path
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    p = build_merged_paths(det)
    assert any(
        len(p.elements(leaf)) < _depth_of(det, p, leaf)
        for leaf in range(p.n_leaves))
    codes = _codes(12, F, rng)
    res = _explain(det, codes)
    np.testing.assert_allclose(res["phi"], _brute(det, codes), rtol=0,
                               atol=1e-9)


def _depth_of(det, p, leaf):
    tree = det.trees()[int(p.leaf_tree[leaf])]
    parent = {}
    for j in np.flatnonzero(tree.feature >= 0):
        parent[int(tree.left[j])] = parent[int(tree.right[j])] = int(j)
    node, depth = int(p.leaf_node[leaf]), 0
    while node in parent:
        node, depth = parent[node], depth + 1
    return depth


@pytest.fixture(scope="module")
def train_tests():
    return make_synthetic_tests(n_tests=300, seed=2)


@pytest.fixture(scope="module")
def other_tests():
    return make_synthetic_tests(n_tests=257, seed=5)


@pytest.fixture(scope="module")
def fitted(train_tests):
    from flake16_framework_amd.engine.detector import fit_detector
    return {name: fit_detector(keys, tests=train_tests, backend="ref",
                               n_trees=N_TREES)
            for name, keys in CONFIGS.items()}


def _first(tests, m):
    out, left = {}, m
    for proj, rows in tests.items():
        take = dict(list(rows.items())[:left])
        if take:
            out[proj] = take
        left -= len(take)
    return out


def _codes_of(det, tests):
    from flake16_framework_amd.engine.detector import load_rows
    X, _, _ = load_rows(det, tests, None)
    T = transform_preprocessing(X, det.preprocessing_params())
    return bin_codes(T.astype(np.float32), det.cut_list())


def test_brute_force_fitted(train_tests, other_tests):
    """7-input fitted trees (deep, features repeat on most paths)."""
    from flake16_framework_amd.engine.detector import fit_detector
    from flake16_framework_amd.engine.explain import explain
    det = fit_detector(
        ("NOD", "FlakeFlagger", "Scaling", "None", "Random Forest"),
        tests=train_tests, backend="ref", n_trees=2)
    rows = _first(other_tests, 4)
    res = explain(det, tests=rows, backend="ref")
    np.testing.assert_allclose(res["phi"], _brute(det, _codes_of(det, rows)),
                               rtol=0, atol=1e-9)


# -- 3. against the TreeSHAP recursion -----------------------------------------
def test_matches_recursion(fitted, other_tests):
    from flake16_framework_amd.engine.explain import explain
    det = fitted["nod"]
    rows = _first(other_tests, 50)
    res = explain(det, tests=rows, backend="ref")
    assert res["phi"].shape == (50, 16)
    want = -forest_shap(SimpleNamespace(trees=det.trees()),
                        _codes_of(det, rows), det.n_features)
    np.testing.assert_allclose(res["phi"], want, rtol=0, atol=1e-9)
    assert np.abs(want).max() > 1e-3


# -- 4. additivity ---------------------------------------------------------------
def _check_additive(det, tests):
    from flake16_framework_amd.engine.detector import detect
    from flake16_framework_amd.engine.explain import explain
    res = explain(det, tests=tests, backend="ref")
    want = detect(det, tests=tests, backend="ref")
    np.testing.assert_array_equal(res["proba"], want["proba"])
    np.testing.assert_array_equal(res["pred"], want["pred"])
    assert list(res["nodeids"]) == list(want["nodeids"])
    assert list(res["projects"]) == list(want["projects"])
    gap = np.abs(res["base_value"] + res["phi"].sum(axis=1) - res["proba"])
    assert gap.max() <= 1e-9
    assert res["phi"].dtype == np.float64
    return res


@pytest.mark.parametrize("name", list(CONFIGS))
def test_additive_fitted(name, fitted, other_tests):
    res = _check_additive(fitted[name], other_tests)
    assert res["phi"].shape == (257, fitted[name].n_features)
    assert np.ptp(res["phi"], axis=0).max() > 1e-3      # rows do differ


@pytest.mark.parametrize("n_trees", [1, 7, 23])
def test_additive_hand_built(n_trees):
    rng = np.random.RandomState(n_trees)
    F = 16
    trees = []
    for t in range(n_trees):
        kind = t % 3
        if kind == 0:
            trees.append(_tree(_random_desc(F, rng)))
        elif kind == 1:
            trees.append(_tree(_leaf(rng)))
        else:
            trees.append(_tree(_chain_desc(1, rng)))
    det = _detector(trees, F)
    codes = _codes(40, F, rng)
    _check_additive(det, _as_tests(codes, det.feature_cols))


# -- 5. refusals, names, artifact, CLI --------------------------------------------
def test_zero_cover_internal_node_refused():
    from flake16_framework_amd.engine.explain import explain
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    rng = np.random.RandomState(3)
    det = _detector([_tree(_random_desc(5, rng)) for _ in range(3)], 5)
    build_merged_paths(det)
    internal = np.flatnonzero(det.feat >= 0)
    assert len(internal) > 2
    j = internal[-1]
    det.cnt0[j] = det.cnt1[j] = 0.0
    det.validate()                      # validate covers leaves only
    with pytest.raises(ValueError, match="zero cover"):
        build_merged_paths(det)
    with pytest.raises(ValueError, match="zero cover"):
        explain(det, tests=_as_tests(_codes(3, 5, rng), det.feature_cols),
                backend="ref")


def test_element_count_limit():
    from flake16_framework_amd.models import mergedpaths
    mergedpaths._check_element_count((1 << 31) - 1)
    with pytest.raises(ValueError, match="int32"):
        mergedpaths._check_element_count(1 << 31)


def test_no_rows(fitted):
    from flake16_framework_amd.engine.explain import explain
    for tests in ({}, {"proj": {}}):
        res = explain(fitted["nod"], tests=tests, backend="ref")
        assert res["phi"].shape == (0, 16) and res["phi"].dtype == np.float64
        assert len(res["proba"]) == 0 and len(res["pred"]) == 0
        assert 0.0 < res["base_value"] < 1.0


def test_feature_names(fitted):
    from flake16_framework_amd.engine.explain import explain
    names = {k: explain(d, tests={}, backend="ref")["feature_names"]
             for k, d in fitted.items()}
    assert names["nod"] == tuple(FEATURE_NAMES)
    assert names["od"] == tuple(FEATURE_NAMES)
    assert names["pca"] == tuple(f"pc{k}" for k in range(7))
    ff = _detector([_tree(("leaf", 1, 1))], 7)
    assert (explain(ff, tests={}, backend="ref")["feature_names"]
            == tuple(FEATURE_NAMES[c] for c in FLAKEFLAGGER_COLUMNS))


def test_write_explanations_round_trip(fitted, other_tests, tmp_path):
    from flake16_framework_amd.engine.explain import (
        explain, write_explanations,
    )
    det = fitted["pca"]
    rows = _first(other_tests, 30)
    path = tmp_path / "ex.json"
    res = write_explanations(det, tests=rows, out_file=str(path),
                             backend="ref")
    with open(path) as fd:
        out = json.load(fd)
    assert list(out) == ["feature_names", "base_value", "tests"]
    assert out["feature_names"] == [f"pc{k}" for k in range(7)]
    assert out["base_value"] == res["base_value"]
    assert list(out["tests"]) == list(rows)
    flat = [v for proj in out["tests"].values() for v in proj.values()]
    assert [nid for proj in out["tests"].values() for nid in proj] == \
        list(res["nodeids"])
    np.testing.assert_array_equal([r[0] for r in flat], res["proba"])
    np.testing.assert_array_equal([r[1] for r in flat], res["pred"])
    np.testing.assert_array_equal([r[2:] for r in flat], res["phi"])
    again = explain(det, tests=rows, backend="ref")
    np.testing.assert_array_equal(again["phi"], res["phi"])


def test_cli_explain(train_tests, other_tests, tmp_path, monkeypatch,
                     capsys):
    from flake16_framework_amd import cli
    from flake16_framework_amd.constants import (
        DETECTOR_FILE, EXPLANATIONS_FILE, TESTS_FILE,
    )
    from flake16_framework_amd.engine.detector import Detector
    from flake16_framework_amd.engine.explain import explain
    assert EXPLANATIONS_FILE == "explanations.json"
    monkeypatch.chdir(tmp_path)
    with open(TESTS_FILE, "w") as fd:
        json.dump(train_tests, fd)
    rows = _first(other_tests, 40)
    with open("other.json", "w") as fd:
        json.dump(rows, fd)
    cli.main(["fit", "--config", "nod", "--backend", "ref", "--n-trees", "3"])
    capsys.readouterr()
    cli.main(["explain", "--backend", "ref", "--tests-file", "other.json"])
    line = capsys.readouterr().out.strip()
    assert line.startswith(f"wrote {EXPLANATIONS_FILE} (40 tests")
    assert os.path.exists(EXPLANATIONS_FILE)
    with open(EXPLANATIONS_FILE) as fd:
        out = json.load(fd)
    res = explain(Detector.load(DETECTOR_FILE), tests=rows, backend="ref")
    flat = [v for proj in out["tests"].values() for v in proj.values()]
    np.testing.assert_array_equal([r[2:] for r in flat], res["phi"])
    top = np.argsort(-np.abs(res["phi"]).mean(axis=0), kind="stable")[:3]
    for f in top:
        assert res["feature_names"][f] in line
    for r in flat:
        assert abs(out["base_value"] + sum(r[2:]) - r[0]) <= 1e-9

    cli.main(["explain", "--detector", DETECTOR_FILE, "--out", "e2.json",
              "--backend", "ref"])
    with open("e2.json") as fd:
        assert list(json.load(fd)["tests"]) == list(train_tests)
