"""dependence on the CPU: the ref backend against the definition (a loop
over the public detect on overwritten tests dicts, the pinned reduction
written out here), the grid rule on hand-written columns, a one-split tree
whose curve is read off by hand, the baseline identities, the errors, the
JSON file and the command."""

import json

import numpy as np
import pytest

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.constants import FEATURE_NAMES
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests

NOD = SHAP_CONFIGS[0]
PCA_FF = ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN", "Random Forest")
DT = ("NOD", "Flake16", "None", "None", "Decision Tree")
GRID = 5


@pytest.fixture(scope="module")
def tests600():
    return make_synthetic_tests(n_tests=600, seed=0)


@pytest.fixture(scope="module")
def fitted(tests600):
    from flake16_framework_amd.engine.detector import fit_detector
    dets = {name: fit_detector(keys, tests=tests600, seed=0, backend="ref",
                               n_trees=10)
            for name, keys in (("nod", NOD), ("pca-ff", PCA_FF))}
    assert dets["nod"].preproc == "scale"
    assert dets["pca-ff"].preproc == "scale+pca"
    return dets


@pytest.fixture(scope="module")
def curves(tests600, fitted):
    """dependence() once per configuration and rule, shared."""
    from flake16_framework_amd.engine.dependence import dependence
    return {(name, t): dependence(det, tests=tests600, grid=GRID,
                                  threshold=t, ice=True, backend="ref")
            for name, det in fitted.items() for t in (None, 0.3)}


# -- the definition ---------------------------------------------------------
def _pinned_sum(acc1, seg_off):
    """Definition steps 1 to 4 with Python floats, element by element."""
    S = []
    for a, b in zip(seg_off[:-1], seg_off[1:]):
        s = 0.0
        for first in range(a, b, 64):
            v = [float(x) for x in acc1[first:min(b, first + 64)]]
            v += [0.0] * (64 - len(v))
            for _ in range(6):
                v = [v[2 * i] + v[2 * i + 1] for i in range(len(v) // 2)]
            assert len(v) == 1
            s = s + v[0]
        S.append(s)
    total = 0.0
    for s in S:
        total = total + s
    return S + [total]


def _acc1(det, X):
    """acc1 as detect forms it, before the division by n_trees."""
    from flake16_framework_amd.models.binning import bin_codes
    from flake16_framework_amd.models.forest_ref import accumulate_proba
    from flake16_framework_amd.preprocess import transform_preprocessing
    T = transform_preprocessing(X, det.preprocessing_params())
    codes = bin_codes(T.astype(np.float32), det.cut_list())
    return accumulate_proba(det.trees(), codes)[1]


@pytest.mark.parametrize("name", ["nod", "pca-ff"])
def test_ref_is_the_definition(name, tests600, fitted, curves):
    from flake16_framework_amd.engine.dependence import make_grids
    from flake16_framework_amd.engine.detector import detect, load_rows
    det = fitted[name]
    names = list(tests600)
    G, n_trees = len(names), det.n_trees
    seg_off = [0, *np.cumsum([len(tests600[p]) for p in names])]
    M = seg_off[-1]
    n_rows = [b - a for a, b in zip(seg_off[:-1], seg_off[1:])] + [M]
    assert min(n_rows) > 0 and max(n_rows[:G]) > 64     # several blocks
    X, _, _ = load_rows(det, tests600, None)
    cols = [int(c) for c in det.feature_cols]
    grids = make_grids(X, GRID)

    def by_definition(tests, Xp):
        out = detect(det, tests=tests, backend="ref")
        acc1 = _acc1(det, Xp)
        np.testing.assert_array_equal(acc1 / n_trees, out["proba"])
        S = _pinned_sum(acc1, seg_off)
        mean = [S[g] / float(n_trees * n_rows[g]) for g in range(G + 1)]
        counts = {}
        for t, pred in ((None, out["pred"].astype(bool)),
                        (0.3, out["proba"] >= 0.3)):
            counts[t] = [int(pred[a:b].sum()) for a, b in
                         [*zip(seg_off[:-1], seg_off[1:]), (0, M)]]
        return out["proba"], mean, counts

    arg, thr = curves[name, None], curves[name, 0.3]
    assert arg["config_keys"] == det.config_keys
    assert (arg["rule"], arg["threshold"]) == ("argmax", None)
    assert (thr["rule"], thr["threshold"]) == ("threshold", 0.3)
    assert arg["n_tests"] == M
    assert list(arg["features"]) == [FEATURE_NAMES[c] for c in cols]
    assert arg["ice"].shape == (M, len(arg["jobs"]))
    assert arg["ice"].dtype == np.float64
    np.testing.assert_array_equal(arg["ice"], thr["ice"])

    _, mean, counts = by_definition(tests600, X)
    for res, t in ((arg, None), (thr, 0.3)):
        assert res["baseline"]["mean_proba"] == mean[G]
        assert res["baseline"]["flagged"] == counts[t][G]
        for g, p in enumerate(names):
            assert res["baseline"]["projects"][p] == [mean[g], counts[t][g]]

    j = moved = 0
    for f, c in enumerate(cols):
        entry = arg["features"][FEATURE_NAMES[c]]
        assert entry["grid"] == grids[f].tolist()
        assert entry["grid"] == thr["features"][FEATURE_NAMES[c]]["grid"]
        assert entry["range"] == (max(entry["mean_proba"])
                                  - min(entry["mean_proba"]))
        for k, v in enumerate(entry["grid"]):
            assert arg["jobs"][j] == [c, v]
            over = {p: {nid: [*row[:2 + c], v, *row[3 + c:]]
                        for nid, row in rows.items()}
                    for p, rows in tests600.items()}
            Xp = X.copy()
            Xp[:, f] = v
            proba, mean, counts = by_definition(over, Xp)
            np.testing.assert_array_equal(arg["ice"][:, j], proba)
            moved += int((proba != arg["ice"][:, 0]).any())
            for res, t in ((arg, None), (thr, 0.3)):
                e = res["features"][FEATURE_NAMES[c]]
                assert e["mean_proba"][k] == mean[G]
                assert e["flagged"][k] == counts[t][G]
                for g, p in enumerate(names):
                    assert e["projects"][p]["mean_proba"][k] == mean[g]
                    assert e["projects"][p]["flagged"][k] == counts[t][g]
            j += 1
    assert j == len(arg["jobs"]) and moved > 0
    assert any(e["range"] > 0 for e in arg["features"].values())
    assert sum(thr["baseline"]["projects"][p][1] for p in names) == \
        thr["baseline"]["flagged"] > 0


@pytest.mark.parametrize("name", ["nod", "pca-ff"])
def test_own_value_on_the_grid_gives_the_detect_probability(
        name, tests600, fitted, curves):
    """Grid values are order statistics of the column, so every job
    leaves some rows as they are."""
    from flake16_framework_amd.engine.detector import detect, load_rows
    det = fitted[name]
    res = curves[name, None]
    proba = detect(det, tests=tests600, backend="ref")["proba"]
    X, _, _ = load_rows(det, tests600, None)
    cols = [int(c) for c in det.feature_cols]
    for j, (c, v) in enumerate(res["jobs"]):
        own = X[:, cols.index(c)] == v
        assert own.any()
        np.testing.assert_array_equal(res["ice"][own, j], proba[own])


# -- the grid ---------------------------------------------------------------
def test_make_grids_on_hand_written_columns():
    from flake16_framework_amd.engine.dependence import make_grids
    rng = np.random.RandomState(0)
    counts = rng.permutation(np.repeat(np.arange(6.0), [40, 30, 15, 10, 4,
                                                        1]))
    X = np.stack([np.full(100, 7.25), counts,
                  rng.permutation(np.arange(100.0))], axis=1)
    const, cnt, ramp = make_grids(X, 20)
    assert all(g.dtype == np.float64 for g in (const, cnt, ramp))
    assert const.tolist() == [7.25]
    # positions 4 .. 95 of the sorted column: 0 x 40, 1 x 30, 2 x 15,
    # 3 x 10, 4 x 4, and the single 5 at position 99 is past the 95 %
    assert cnt.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    lo, hi = 99 * 5 // 100, 99 - 99 * 5 // 100
    assert (lo, hi) == (4, 95)
    assert ramp.tolist() == [float(lo + k * (hi - lo) // 19)
                             for k in range(20)]
    assert ramp[0] == 4.0 and ramp[-1] == 95.0 and len(ramp) == 20

    # fewer rows than grid values: every value at most once, ascending
    few = make_grids(np.array([[3.0], [1.0], [2.0]]), 20)[0]
    assert few.tolist() == [1.0, 2.0, 3.0]
    two = make_grids(np.array([[3.0], [1.0], [2.0]]), 2)[0]
    assert two.tolist() == [1.0, 3.0]

    # the index formula: M -> (lo, hi), and the V = 4 positions
    for M, lo, hi, idx in ((1, 0, 0, [0, 0, 0, 0]),
                           (2, 0, 1, [0, 0, 0, 1]),
                           (21, 1, 19, [1, 7, 13, 19]),
                           (101, 5, 95, [5, 35, 65, 95])):
        assert ((M - 1) * 5 // 100, (M - 1) - (M - 1) * 5 // 100) == (lo, hi)
        col = rng.permutation(np.arange(M, dtype=np.float64) * 10.0)
        got = make_grids(col[:, None], 4)[0]
        assert got.tolist() == sorted({10.0 * i for i in idx}), M

    for bad in (1, 65, 0):
        with pytest.raises(ValueError):
            make_grids(X, bad)
    with pytest.raises(ValueError):
        make_grids(np.zeros((0, 3)), 20)


# -- a case small enough to check by hand -----------------------------------
CUT = np.float32(0.1)


def _one_split_detector():
    """One tree, one split on column 0 at the single cut 0.1f: the left
    leaf holds counts (3, 1), probability 0.25; the right leaf (0, 2)."""
    from flake16_framework_amd.engine.detector import assemble_detector
    from flake16_framework_amd.models.forest_ref import Tree
    F = 16
    params = {"spec": None, "mean": np.zeros(F), "scale": np.ones(F),
              "pca_mean": np.zeros(F), "W": np.eye(F)}
    cuts = [np.array([CUT], dtype=np.float32)] + [
        np.zeros(0, dtype=np.float32)] * (F - 1)
    tree = Tree(np.array([0, -1, -1], dtype=np.int32),
                np.array([0, 0, 0], dtype=np.int32),
                np.zeros(3, dtype=np.float32),
                np.array([1, -1, -1], dtype=np.int32),
                np.array([2, -1, -1], dtype=np.int32),
                np.array([3.0, 3.0, 0.0]), np.array([3.0, 1.0, 2.0]))
    return assemble_detector(DT, 2, tuple(range(16)), params, cuts, [tree],
                             1, 0, 6)


def _hand_tests():
    """70 rows left of the cut and 30 right of it in "a", nothing in "b",
    one row on each side in "c"."""
    rng = np.random.RandomState(1)
    row = lambda f0: [0, 0, float(f0), *(float(v) for v in rng.randn(15))]
    a = {f"t{i:03d}": row(-1.0 - i if i < 70 else 1.0 + i)
         for i in range(100)}
    return {"a": a, "b": {}, "c": {"l": row(-5.0), "r": row(5.0)}}


def test_one_split_tree_by_hand():
    from flake16_framework_amd.engine.dependence import dependence
    det = _one_split_detector()
    tests = _hand_tests()
    c64 = np.float64(CUT)
    below = np.nextafter(c64, -np.inf)
    assert below < c64 and np.float32(below) == CUT      # rounds UP to c
    grid = [-3.0, float(below), float(c64), 2.0]
    res = dependence(det, tests=tests, grids={0: grid}, ice=True,
                     backend="ref")
    assert list(res["features"]) == ["Covered Lines"]
    e = res["features"]["Covered Lines"]
    assert e["grid"] == grid
    # code = #{cut <= (float)v}: left for v < c, right from (float)v == c
    assert e["mean_proba"] == [0.25, 1.0, 1.0, 1.0]
    assert e["flagged"] == [0, 102, 102, 102]
    assert e["range"] == 0.75
    assert e["projects"]["a"] == {"mean_proba": [0.25, 1.0, 1.0, 1.0],
                                  "flagged": [0, 100, 100, 100]}
    assert e["projects"]["b"] == {"mean_proba": [None] * 4,
                                  "flagged": [0] * 4}
    assert e["projects"]["c"]["flagged"] == [0, 2, 2, 2]
    assert res["ice"].shape == (102, 4)
    assert (res["ice"][:, 0] == 0.25).all() and (res["ice"][:, 1:] == 1).all()
    assert res["jobs"] == [[0, v] for v in grid]
    # the unmodified rows: 71 x 0.25 and 31 x 1.0
    base = res["baseline"]
    assert base["mean_proba"] == (71 * 0.25 + 31) / 102
    assert base["flagged"] == 31
    assert base["projects"] == {"a": [(70 * 0.25 + 30) / 100, 30],
                                "b": [None, 0], "c": [0.625, 1]}
    assert res["n_tests"] == 102

    # 0.25 >= 0.25: under a threshold rule the left leaf is flagged too
    thr = dependence(det, tests=tests, grids={0: grid}, threshold=0.25,
                     backend="ref")
    assert thr["features"]["Covered Lines"]["flagged"] == [102] * 4
    assert thr["baseline"]["flagged"] == 102
    assert "ice" not in thr and "jobs" not in thr


def test_unused_feature_gives_the_baseline():
    """Without a projection a column that no tree reads cannot move a
    probability: its curve is the baseline, bit for bit."""
    from flake16_framework_amd.engine.dependence import dependence
    det = _one_split_detector()
    tests = _hand_tests()
    res = dependence(det, tests=tests, grid=7, backend="ref")
    assert list(res["features"]) == list(FEATURE_NAMES)
    base = res["baseline"]
    assert 0.25 < base["mean_proba"] < 1.0
    for name in FEATURE_NAMES[1:]:
        e = res["features"][name]
        assert len(e["grid"]) == 7
        assert e["mean_proba"] == [base["mean_proba"]] * 7
        assert e["flagged"] == [base["flagged"]] * 7
        assert e["range"] == 0.0
        for p in tests:
            assert e["projects"][p]["mean_proba"] == \
                [base["projects"][p][0]] * 7
            assert e["projects"][p]["flagged"] == \
                [base["projects"][p][1]] * 7
    assert res["features"]["Covered Lines"]["range"] == 0.75


# -- errors -----------------------------------------------------------------
def test_errors(tests600, fitted):
    from flake16_framework_amd.engine.dependence import dependence
    ff, nod = fitted["pca-ff"], fitted["nod"]
    kw = dict(tests=tests600, backend="ref")
    for grid in (1, 65):
        with pytest.raises(ValueError):
            dependence(nod, grid=grid, **kw)
    with pytest.raises(ValueError):      # column 8 is not a FlakeFlagger one
        dependence(ff, grids={8: [1.0]}, **kw)
    for values in ([], [1.0] * 65, list(range(65)), [2.0, 1.0], [1.0, 1.0],
                   [0.0, float("nan")], [float("inf")], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            dependence(nod, grids={3: values}, **kw)
    with pytest.raises(ValueError):
        dependence(nod, grids={}, **kw)
    for threshold in (1.5, -0.1):
        with pytest.raises(ValueError):
            dependence(nod, threshold=threshold, **kw)
    with pytest.raises(ValueError):
        dependence(nod, backend="cuda", tests=tests600)
    with pytest.raises(ValueError):
        dependence(nod, tests={"p": {}}, backend="ref")
    bad = {p: dict(rows) for p, rows in tests600.items()}
    proj = next(iter(bad))
    nid = next(iter(bad[proj]))
    bad[proj][nid] = list(bad[proj][nid])
    bad[proj][nid][5] = float("nan")
    with pytest.raises(ValueError):
        dependence(nod, tests=bad, backend="ref")
    # 64 values for one column are accepted
    res = dependence(nod, grids={3: list(range(64))}, **kw)
    assert len(res["features"]["Execution Time"]["grid"]) == 64


# -- files and the command --------------------------------------------------
def test_cli_round_trip(tests600, tmp_path, monkeypatch, capsys):
    from flake16_framework_amd import cli
    from flake16_framework_amd.constants import DEPENDENCE_FILE
    from flake16_framework_amd.engine.dependence import dependence
    from flake16_framework_amd.engine.detector import Detector
    assert DEPENDENCE_FILE == "dependence.json"
    monkeypatch.chdir(tmp_path)
    some = {p: tests600[p] for p in list(tests600)[:4]}
    some["empty"] = {}
    with open("tests.json", "w") as fd:
        json.dump(tests600, fd)
    with open("other.json", "w") as fd:
        json.dump(some, fd)
    cli.main(["fit", "--config", "nod", "--backend", "ref", "--n-trees",
              "3"])
    cli.main(["dependence", "--backend", "ref", "--grid", "4",
              "--tests-file", "other.json"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    det = Detector.load("detector.npz")
    want = dependence(det, tests=some, grid=4, backend="ref")
    doc = dict(want, config_keys=list(want["config_keys"]))
    with open("dependence.json") as fd:
        text = fd.read()
    assert text == json.dumps(doc, indent=4)
    assert "null" in text and "NaN" not in text
    assert json.loads(text)["baseline"]["projects"]["empty"] == [None, 0]
    top = sorted(want["features"],
                 key=lambda n: -want["features"][n]["range"])[:3]
    assert "dependence.json" in line and "argmax rule" in line
    for name in top:
        assert f"{name} {want['features'][name]['range']:.4f}" in line
    assert line.index(top[0]) < line.index(top[1]) < line.index(top[2])

    cli.main(["dependence", "--backend", "ref", "--grid", "3",
              "--tests-file", "other.json", "--threshold", "0.3", "--out",
              "thr.json", "--ice-out", "ice.npy"])
    want = dependence(det, tests=some, grid=3, threshold=0.3, ice=True,
                      backend="ref")
    with open("thr.json") as fd:
        doc = json.load(fd)
    assert (doc["rule"], doc["threshold"]) == ("threshold", 0.3)
    assert "ice" not in doc and "jobs" not in doc
    assert doc["features"] == want["features"]
    ice = np.load("ice.npy")
    assert ice.dtype == np.float64
    np.testing.assert_array_equal(ice, want["ice"])
