"""fit / detect on the numpy backend: saved-parameter preprocessing,
canonical node numbering, the detector artifact and the CLI."""

import json
import os

import numpy as np
import pytest

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
from flake16_framework_amd.models.binning import bin_codes
from flake16_framework_amd.models.forest_ref import (
    Forest, ForestParams, Tree, canonicalize_tree, predict_forest,
)
from flake16_framework_amd.preprocess import (
    fit_preprocessing, pca_fit_transform, scaler_fit_transform,
    transform_preprocessing,
)

N_TREES = 12

# one configuration per preprocessing spec, plus a 7-column one
CONFIGS = {
    "none": ("NOD", "Flake16", "None", "SMOTE", "Random Forest"),
    "scale": SHAP_CONFIGS[0],
    "pca": ("OD", "Flake16", "PCA", "Tomek Links", "Extra Trees"),
    "flakeflagger": ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN",
                     "Random Forest"),
}


@pytest.fixture(scope="module")
def train_tests():
    return make_synthetic_tests(n_tests=300, seed=2)


@pytest.fixture(scope="module")
def fitted(train_tests):
    from flake16_framework_amd.engine.detector import fit_detector
    return {name: fit_detector(keys, tests=train_tests, backend="ref",
                               n_trees=N_TREES)
            for name, keys in CONFIGS.items()}


def _assert_same_detector(a, b):
    aa, bb = a.arrays(), b.arrays()
    assert aa.keys() == bb.keys()
    for name in aa:
        assert aa[name].dtype == bb[name].dtype, name
        np.testing.assert_array_equal(aa[name], bb[name], err_msg=name)


# -- 1. saved-parameter preprocessing --------------------------------------
def _matrices():
    rng = np.random.RandomState(7)
    A = rng.randn(500, 16) * rng.uniform(0.1, 50.0, size=16) + rng.randn(16)
    B = rng.lognormal(1.0, 1.5, size=(300, 7))
    B[:, 3] = 4.25                      # zero-variance column
    return [A, B]


@pytest.mark.parametrize("X", _matrices(), ids=["500x16", "300x7const"])
def test_transform_on_fitting_matrix(X):
    p = fit_preprocessing(X, None)
    np.testing.assert_array_equal(transform_preprocessing(X, p), X)

    p = fit_preprocessing(X, "scale")
    np.testing.assert_array_equal(transform_preprocessing(X, p),
                                  scaler_fit_transform(X))

    p = fit_preprocessing(X, "scale+pca")
    got = transform_preprocessing(X, p)
    want = pca_fit_transform(scaler_fit_transform(X))
    print("max |saved-parameter PCA - pca_fit_transform| =",
          np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)


def test_transform_other_matrix_hand_computed():
    X, _ = _matrices()
    rng = np.random.RandomState(11)
    Y = rng.randn(5, 16) * 30.0
    for spec in ("scale", "scale+pca"):
        p = fit_preprocessing(X, spec)
        want = np.empty_like(Y)
        for i in range(Y.shape[0]):
            z = [(float(Y[i, f]) - float(p["mean"][f])) / float(p["scale"][f])
                 for f in range(16)]
            if spec == "scale":
                want[i] = z
                continue
            for k in range(16):
                t = 0.0
                for f in range(16):
                    t = t + (z[f] - float(p["pca_mean"][f])) \
                        * float(p["W"][f, k])
                want[i, k] = t
        np.testing.assert_array_equal(transform_preprocessing(Y, p), want)
    with pytest.raises(ValueError):
        fit_preprocessing(X, "whiten")


# -- 2. canonical numbering ------------------------------------------------
def _scrambled_tree():
    """        0:f2<=5
              /       \\
          4:f0<=1     2:leaf(1,3)
          /     \\
     1:leaf(4,0)  5:f1<=7
                  /     \\
             3:leaf(0,2) 6:leaf(2,2)
    Right children are not next to their left siblings."""
    L = -1
    return Tree(
        feature=np.array([2, L, L, L, 0, 1, L], dtype=np.int32),
        split_bin=np.array([5, 9, 9, 9, 1, 7, 9], dtype=np.int32),
        threshold=np.arange(7, dtype=np.float32),
        left=np.array([4, 9, 9, 9, 1, 3, 9], dtype=np.int32),
        right=np.array([2, 9, 9, 9, 5, 6, 9], dtype=np.int32),
        count0=np.array([7, 4, 1, 0, 6, 2, 2], dtype=np.float64),
        count1=np.array([7, 0, 3, 2, 4, 4, 2], dtype=np.float64))


def test_canonical_numbering():
    L = -1
    tree = _scrambled_tree()
    canon = canonicalize_tree(tree)
    np.testing.assert_array_equal(canon.feature, [2, 0, L, L, 1, L, L])
    np.testing.assert_array_equal(canon.split_bin, [5, 1, 0, 0, 7, 0, 0])
    np.testing.assert_array_equal(canon.left, [1, 3, L, L, 5, L, L])
    np.testing.assert_array_equal(canon.right, [2, 4, L, L, 6, L, L])
    np.testing.assert_array_equal(canon.count0, [7, 6, 1, 4, 2, 0, 2])
    np.testing.assert_array_equal(canon.count1, [7, 4, 3, 0, 4, 2, 2])

    again = canonicalize_tree(canon)
    for name in ("feature", "split_bin", "threshold", "left", "right",
                 "count0", "count1"):
        np.testing.assert_array_equal(getattr(again, name),
                                      getattr(canon, name))
        assert getattr(again, name).dtype == getattr(canon, name).dtype

    rng = np.random.RandomState(0)
    codes = rng.randint(0, 12, size=(200, 3)).astype(np.uint8)
    # a second tree that votes the other way makes ties and both classes
    stump = Tree(np.array([L], dtype=np.int32), np.zeros(1, np.int32),
                 np.zeros(1, np.float32), np.array([L], dtype=np.int32),
                 np.array([L], dtype=np.int32), np.array([1.0]),
                 np.array([1.0]))
    before = predict_forest(Forest([tree, stump], ForestParams()), codes)
    after = predict_forest(Forest([canon, stump], ForestParams()), codes)
    assert 0 < before.sum() < len(before)
    np.testing.assert_array_equal(after, before)


# -- 3. round trip ---------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_round_trip(name, fitted, train_tests, tmp_path):
    from flake16_framework_amd.engine.detector import (
        Detector, detect, fit_detector,
    )
    det = fitted[name]
    keys = CONFIGS[name]
    assert det.config_keys == keys and det.n_trees == N_TREES
    assert det.n_features == (7 if keys[1] == "FlakeFlagger" else 16)
    assert det.n_train == 300 and det.cut_off.shape == (17,)
    # canonical numbering: siblings adjacent, one child array
    internal = det.feat >= 0
    assert (det.left[~internal] == -1).all() and internal.any()

    path = tmp_path / "detector.npz"
    det.save(path)
    with np.load(path, allow_pickle=False) as z:     # no pickled objects
        assert set(z.files) == set(det.arrays())
    loaded = Detector.load(path)
    _assert_same_detector(loaded, det)

    res = detect(loaded, tests=train_tests, backend="ref")
    from flake16_framework_amd.dataset.tests_io import load_feat_lab_proj
    feats, _, projects = load_feat_lab_proj(
        det.flaky_label, list(det.feature_cols), tests=train_tests)
    X = transform_preprocessing(feats, det.preprocessing_params())
    codes = bin_codes(X.astype(np.float32), det.cut_list())
    want = predict_forest(Forest(det.trees(), ForestParams()), codes)
    np.testing.assert_array_equal(res["pred"], want)
    assert res["pred"].dtype == np.uint8 and res["proba"].dtype == np.float64
    assert ((res["proba"] >= 0.0) & (res["proba"] <= 1.0)).all()
    assert 0 < res["pred"].sum() < len(want)
    np.testing.assert_array_equal(res["projects"], projects)
    assert list(res["nodeids"]) == [
        nid for tests_proj in train_tests.values() for nid in tests_proj]

    _assert_same_detector(
        fit_detector(keys, tests=train_tests, backend="ref",
                     n_trees=N_TREES), det)


def test_seed_changes_extra_trees(fitted, train_tests):
    from flake16_framework_amd.engine.detector import fit_detector
    det = fitted["scale"]
    assert det.config_keys[4] == "Extra Trees"
    other = fit_detector(det.config_keys, tests=train_tests, backend="ref",
                         n_trees=N_TREES, seed=1)
    assert other.seed == 1
    assert (len(other.feat) != len(det.feat)
            or not np.array_equal(other.feat, det.feat)
            or not np.array_equal(other.split, det.split))


def test_n_trees_defaults_to_axis_value(train_tests):
    from flake16_framework_amd.engine.detector import fit_detector
    keys = ("NOD", "FlakeFlagger", "None", "None", "Decision Tree")
    det = fit_detector(keys, tests=train_tests, backend="ref")
    assert det.n_trees == 1 and det.tree_off.shape == (2,)


# -- 4. loader errors ------------------------------------------------------
def test_loader_errors(fitted, train_tests, tmp_path):
    from flake16_framework_amd.engine.detector import Detector, detect
    det = fitted["scale"]
    arrays = det.arrays()

    bad = dict(arrays, version=np.asarray(99))
    np.savez(tmp_path / "version.npz", **bad)
    with pytest.raises(ValueError, match="version"):
        Detector.load(tmp_path / "version.npz")

    for field in ("left", "cuts", "version"):
        part = {k: v for k, v in arrays.items() if k != field}
        np.savez(tmp_path / "missing.npz", **part)
        with pytest.raises(ValueError, match=field):
            Detector.load(tmp_path / "missing.npz")

    # a child id that would walk out of its tree is refused at load
    left = arrays["left"].copy()
    left[0] = len(left)
    np.savez(tmp_path / "child.npz", **dict(arrays, left=left))
    with pytest.raises(ValueError):
        Detector.load(tmp_path / "child.npz")

    proj = next(iter(train_tests))
    nid = next(iter(train_tests[proj]))
    row = list(train_tests[proj][nid])
    row[2 + int(det.feature_cols[3])] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        detect(det, tests={proj: {nid: row}}, backend="ref")
    # the ignored columns may hold anything
    row = list(train_tests[proj][nid])
    row[0], row[1] = float("nan"), -5
    assert len(detect(det, tests={proj: {nid: row}},
                      backend="ref")["proba"]) == 1


# -- 5. CLI ----------------------------------------------------------------
def test_cli_fit_then_detect(train_tests, tmp_path, monkeypatch):
    from flake16_framework_amd import cli
    from flake16_framework_amd.constants import (
        DETECTIONS_FILE, DETECTOR_FILE, TESTS_FILE,
    )
    from flake16_framework_amd.engine.detector import Detector, detect
    monkeypatch.chdir(tmp_path)
    with open(TESTS_FILE, "w") as fd:
        json.dump(train_tests, fd)
    other = make_synthetic_tests(n_tests=120, seed=9)
    with open("other.json", "w") as fd:
        json.dump(other, fd)

    cli.main(["fit", "--config", "od", "--backend", "ref",
              "--n-trees", str(N_TREES)])
    assert os.path.exists(DETECTOR_FILE)
    det = Detector.load(DETECTOR_FILE)
    assert det.config_keys == SHAP_CONFIGS[1] and det.n_trees == N_TREES

    cli.main(["detect", "--backend", "ref", "--tests-file", "other.json"])
    with open(DETECTIONS_FILE) as fd:
        out = json.load(fd)
    assert list(out) == list(other)
    for proj in other:
        assert list(out[proj]) == list(other[proj])
    res = detect(det, tests=other, backend="ref")
    rows = [v for tests_proj in out.values() for v in tests_proj.values()]
    np.testing.assert_array_equal([r[0] for r in rows], res["proba"])
    np.testing.assert_array_equal([r[1] for r in rows], res["pred"])

    cli.main(["fit", "--keys", *CONFIGS["flakeflagger"], "--backend", "ref",
              "--n-trees", "3", "--detector", "ff.npz"])
    assert Detector.load("ff.npz").config_keys == CONFIGS["flakeflagger"]
    cli.main(["detect", "--detector", "ff.npz", "--out", "ff.json",
              "--backend", "ref"])
    with open("ff.json") as fd:
        assert list(json.load(fd)) == list(train_tests)
