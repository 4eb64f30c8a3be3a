"""importance on the CPU: the permutation table against Philox draws
written out here, the ref backend against the definition (a loop over the
public detect), a hand-checkable case, the two rules, the list form, the
errors, the JSON file and the command."""

import json

import numpy as np
import pytest

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.constants import FEATURE_NAMES
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
from flake16_framework_amd.engine.metrics import get_prf

NOD = SHAP_CONFIGS[0]
PCA_FF = ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN", "Random Forest")
DT = ("NOD", "Flake16", "None", "None", "Decision Tree")


@pytest.fixture(scope="module")
def tests5():
    return make_synthetic_tests(n_tests=300, n_projects=5, seed=2)


@pytest.fixture(scope="module")
def fitted(tests5):
    from flake16_framework_amd.engine.detector import fit_detector
    return {name: fit_detector(keys, tests=tests5, seed=0, backend="ref",
                               n_trees=6)
            for name, keys in (("nod", NOD), ("pca-ff", PCA_FF))}


# -- the permutation table --------------------------------------------------
def test_permutation_table():
    from flake16_framework_amd.engine.importance import (
        IMPORTANCE_KEY, make_permutations,
    )
    from flake16_framework_amd.utils.philox import TAG_PERMUTE, philox4x32
    assert TAG_PERMUTE == 6 and IMPORTANCE_KEY == 1 << 24

    seg_off = [0, 5, 5, 6, 30]           # an empty and a one-row segment
    perm = make_permutations(seg_off, 3, seed=7)
    assert perm.shape == (3, 30) and perm.dtype == np.int32
    for r in range(3):
        for a, b in zip(seg_off[:-1], seg_off[1:]):
            assert sorted(perm[r, a:b]) == list(range(a, b))
    assert (perm[:, 5] == 5).all()                      # identity
    assert not (perm[0] == perm[1]).all()
    assert not (perm[1] == perm[2]).all()
    assert not (perm[0] == make_permutations(seg_off, 1, seed=8)[0]).all()
    assert make_permutations([0, 0], 2, 0).shape == (2, 0)

    # written out from philox4x32 on three segments
    seg3, seed = [0, 4, 7, 16], 3
    want = np.empty((2, 16), dtype=np.int32)
    for r in range(2):
        for g in range(3):
            a, b = seg3[g], seg3[g + 1]
            u = [int(philox4x32(6, r, g, i, seed, 1 << 24)[0])
                 for i in range(b - a)]
            order = sorted(range(b - a), key=lambda i: u[i])     # stable
            want[r, a:b] = [a + i for i in order]
    np.testing.assert_array_equal(make_permutations(seg3, 2, seed), want)


def test_permutations_do_not_depend_on_groups(tests5, fitted):
    """Common random numbers: a group's counts are the same whatever other
    groups it is evaluated with."""
    from flake16_framework_amd.engine.importance import importance
    det = fitted["nod"]
    kw = dict(tests=tests5, repeats=2, seed=4, backend="ref")
    full = importance(det, **kw)["importance"]
    some = importance(det, groups={"Static": list(range(9, 16)),
                                   "Read Count": [4]}, **kw)["importance"]
    assert list(some) == ["Static", "Read Count"]
    for name in some:
        assert some[name] == full[name]


# -- the definition ---------------------------------------------------------
def _by_definition(det, tests, groups, repeats, seed, threshold):
    """importance's counts from permuted tests dicts and the public
    detect."""
    from flake16_framework_amd.engine.detector import detect
    from flake16_framework_amd.engine.importance import make_permutations
    names = list(tests)
    rows = [(p, nid, row) for p in names for nid, row in tests[p].items()]
    seg_off = np.concatenate(
        ([0], np.cumsum([len(tests[p]) for p in names])))
    y = np.array([row[1] == det.flaky_label for _, _, row in rows])
    perm = make_permutations(seg_off, repeats, seed)

    def counts(t):
        out = detect(det, tests=t, backend="ref")
        pred = (out["pred"].astype(bool) if threshold is None
                else out["proba"] >= threshold)
        res = []
        for a, b in [*zip(seg_off[:-1], seg_off[1:]), (0, len(y))]:
            p, t_ = pred[a:b], y[a:b]
            res.append([int((p & ~t_).sum()), int((~p & t_).sum()),
                        int((p & t_).sum())])
        return res

    baseline = counts(tests)
    per_group = {}
    for name, cols in groups.items():
        per_group[name] = []
        for r in range(repeats):
            permuted = {p: {} for p in names}
            for i, (p, nid, row) in enumerate(rows):
                new = list(row)
                for c in cols:
                    new[2 + c] = rows[perm[r, i]][2][2 + c]
                permuted[p][nid] = new
            per_group[name].append(counts(permuted))
    return baseline, per_group


@pytest.mark.parametrize("threshold", [None, 0.5])
@pytest.mark.parametrize("name", ["nod", "pca-ff"])
def test_ref_is_the_definition(name, threshold, tests5, fitted):
    from flake16_framework_amd.engine.importance import (
        default_groups, importance,
    )
    det = fitted[name]
    groups = default_groups(det)
    res = importance(det, tests=tests5, repeats=2, seed=1,
                     threshold=threshold, backend="ref")
    baseline, per_group = _by_definition(det, tests5, groups, 2, 1,
                                         threshold)
    names = list(tests5)
    G = len(names)

    assert res["config_keys"] == det.config_keys
    assert (res["seed"], res["repeats"]) == (1, 2)
    assert res["rule"] == ("argmax" if threshold is None else "threshold")
    assert res["threshold"] == threshold
    assert res["groups"] == groups
    assert res["baseline"]["total"] == [*baseline[G],
                                        *get_prf(*baseline[G])]
    for g, p in enumerate(names):
        assert res["baseline"]["projects"][p] == [*baseline[g],
                                                  *get_prf(*baseline[g])]
    f1_base, rec_base = get_prf(*baseline[G])[2], get_prf(*baseline[G])[1]
    assert f1_base is not None
    assert list(res["importance"]) == list(groups)
    changed = 0
    for gname, entry in res["importance"].items():
        want = per_group[gname]
        assert entry["counts"] == [want[r][G] for r in range(2)]
        for g, p in enumerate(names):
            assert entry["projects"][p] == [want[r][g] for r in range(2)]
        f1 = [get_prf(*want[r][G])[2] for r in range(2)]
        rec = [get_prf(*want[r][G])[1] for r in range(2)]
        assert None not in rec           # the pooled file has flaky tests
        assert entry["f1_drop"] == [
            None if f is None else f1_base - f for f in f1]
        assert entry["f1_drop_mean"] == (
            None if None in f1 else sum(entry["f1_drop"]) / 2)
        assert entry["recall_drop"] == [rec_base - v for v in rec]
        assert entry["recall_drop_mean"] == sum(entry["recall_drop"]) / 2
        changed += entry["counts"] != [baseline[G]] * 2
    assert changed >= 3                  # the permutations do something


def test_default_groups(fitted):
    from flake16_framework_amd.engine.importance import default_groups
    groups = default_groups(fitted["nod"])
    assert list(groups) == [*FEATURE_NAMES, "Coverage", "Resource Usage",
                            "Static"]
    assert len(groups) == 19
    assert groups["Coverage"] == [0, 1, 2]
    assert groups["Resource Usage"] == [3, 4, 5, 6, 7, 8]
    assert groups["Static"] == [9, 10, 11, 12, 13, 14, 15]
    assert groups["Max. Memory"] == [8]
    # FlakeFlagger columns (0, 1, 2, 3, 10, 11, 14): the resource family
    # shrinks to the one-feature group it then equals, and is kept
    ff = default_groups(fitted["pca-ff"])
    assert list(ff)[7:] == ["Coverage", "Resource Usage", "Static"]
    assert ff["Resource Usage"] == ff["Execution Time"] == [3]
    assert ff["Static"] == [10, 11, 14]


# -- a case small enough to check by hand -----------------------------------
def _hand_tests():
    rng = np.random.RandomState(0)
    tests = {}
    for proj, n in (("a", 80), ("b", 1), ("c", 120)):
        tests[proj] = {}
        for i in range(n):
            f = rng.randn(16) * 10
            tests[proj][f"t{i:03d}"] = [0, 2 if f[0] > 0 else 0,
                                        *(float(v) for v in f)]
    return tests


def test_hand_checkable_case():
    """The label is f0 > 0, so the tree splits on feature 0 alone: no
    other column can change a prediction, and permuting column 0 leaves
    the predictions of a balanced label at chance."""
    from flake16_framework_amd.engine.detector import fit_detector
    from flake16_framework_amd.engine.importance import importance
    tests = _hand_tests()
    det = fit_detector(DT, tests=tests, seed=0, backend="ref")
    assert det.n_trees == 1 and det.feat.tolist() == [0, -1, -1]

    res = importance(det, tests=tests, repeats=3, seed=0, backend="ref")
    assert res["baseline"]["total"] == [0, 0, 101, 1.0, 1.0, 1.0]
    assert res["baseline"]["projects"]["b"] == [0, 0, 0, None, None, None]
    for name, entry in res["importance"].items():
        if 0 in res["groups"][name]:
            continue
        assert entry["counts"] == [[0, 0, 101]] * 3, name
        assert entry["f1_drop_mean"] == 0.0, name
        assert entry["recall_drop_mean"] == 0.0, name
    for name in ("Covered Lines", "Coverage"):
        assert res["importance"][name]["f1_drop_mean"] > 0.3
        assert res["importance"][name]["counts"][0] == [50, 50, 51]
        # the one-row project can only borrow from itself
        assert res["importance"][name]["projects"]["b"] == [[0, 0, 0]] * 3


# -- the two rules ----------------------------------------------------------
def _tie_detector():
    """One tree, one split on column 0 at its single cut: the left leaf
    holds counts (1, 1), probability exactly 0.5; the right leaf (0, 2)."""
    from flake16_framework_amd.engine.detector import assemble_detector
    from flake16_framework_amd.models.forest_ref import Tree
    F = 16
    params = {"spec": None, "mean": np.zeros(F), "scale": np.ones(F),
              "pca_mean": np.zeros(F), "W": np.eye(F)}
    cuts = [np.array([0.0], dtype=np.float32)] + [
        np.zeros(0, dtype=np.float32)] * (F - 1)
    tree = Tree(np.array([0, -1, -1], dtype=np.int32),
                np.array([0, 0, 0], dtype=np.int32),
                np.zeros(3, dtype=np.float32),
                np.array([1, -1, -1], dtype=np.int32),
                np.array([2, -1, -1], dtype=np.int32),
                np.array([2.0, 1.0, 0.0]), np.array([2.0, 1.0, 2.0]))
    return assemble_detector(DT, 2, tuple(range(16)), params, cuts, [tree],
                             1, 0, 4)


def test_rule_split_on_a_tie():
    from flake16_framework_amd.engine.detector import detect
    from flake16_framework_amd.engine.importance import importance
    det = _tie_detector()
    row = lambda label, f0: [0, label, f0, *([0.0] * 15)]
    tests = {"p": {"tie-flaky": row(2, -1.0), "tie-clean": row(0, -2.0),
                   "sure": row(2, 1.0)}}
    out = detect(det, tests=tests, backend="ref")
    assert out["proba"].tolist() == [0.5, 0.5, 1.0]
    assert out["pred"].tolist() == [0, 0, 1]

    groups = {"Assertions": [10]}        # a column the tree never reads
    arg = importance(det, tests=tests, groups=groups, repeats=1,
                     backend="ref")
    thr = importance(det, tests=tests, groups=groups, repeats=1,
                     threshold=0.5, backend="ref")
    assert arg["rule"] == "argmax" and arg["threshold"] is None
    assert thr["rule"] == "threshold" and thr["threshold"] == 0.5
    assert arg["baseline"]["total"][:3] == [0, 1, 1]    # ties are not flaky
    assert thr["baseline"]["total"][:3] == [1, 0, 2]    # 0.5 >= 0.5
    assert arg["importance"]["Assertions"]["counts"] == [[0, 1, 1]]
    assert thr["importance"]["Assertions"]["counts"] == [[1, 0, 2]]


# -- one detector per project -----------------------------------------------
def test_list_form_equals_single(tests5, fitted):
    from flake16_framework_amd.engine.importance import importance
    det = fitted["pca-ff"]
    kw = dict(tests=tests5, repeats=2, seed=2, backend="ref")
    assert importance([det] * 5, **kw) == importance(det, **kw)


def test_holdout_importance_uses_the_fold_detectors(tests5):
    from flake16_framework_amd.engine.holdout import holdout
    from flake16_framework_amd.engine.importance import (
        holdout_importance, importance,
    )
    groups = {"Coverage": [0, 1, 2], "Max. Memory": [8]}
    got = holdout_importance(NOD, tests=tests5, n_trees=4, seed=0,
                             groups=groups, repeats=2, backend="ref")
    folds = holdout(NOD, tests=tests5, seed=0, backend="ref", n_trees=4,
                    keep_detectors=True)
    want = importance(folds["detectors"], tests=tests5, groups=groups,
                      repeats=2, seed=0, backend="ref")
    assert got == want
    # the baseline of the list form is holdout's own out-of-fold result
    assert got["baseline"]["total"] == folds["total"]["argmax"]
    for p in tests5:
        assert got["baseline"]["projects"][p] == \
            folds["projects"][p]["argmax"]


# -- errors -----------------------------------------------------------------
def test_errors(tests5, fitted):
    from flake16_framework_amd.engine.importance import (
        importance, make_permutations,
    )
    ff, nod = fitted["pca-ff"], fitted["nod"]
    kw = dict(tests=tests5, backend="ref")
    with pytest.raises(ValueError):      # column 8 is not a FlakeFlagger one
        importance(ff, groups={"Max. Memory": [8]}, **kw)
    with pytest.raises(ValueError):
        importance(nod, groups={"nothing": []}, **kw)
    with pytest.raises(ValueError):
        importance(nod, groups={}, **kw)
    with pytest.raises(ValueError):
        importance(nod, repeats=0, **kw)
    with pytest.raises(ValueError):
        make_permutations([0, 3], 0, 0)
    with pytest.raises(ValueError):
        importance(nod, threshold=1.5, **kw)
    with pytest.raises(ValueError):      # 4 detectors, 5 projects
        importance([nod] * 4, **kw)
    with pytest.raises(ValueError):      # two configurations
        importance([nod, nod, nod, nod, ff], **kw)
    bad = {p: dict(rows) for p, rows in tests5.items()}
    proj = next(iter(bad))
    nid = next(iter(bad[proj]))
    bad[proj][nid] = list(bad[proj][nid])
    bad[proj][nid][5] = float("nan")
    with pytest.raises(ValueError):
        importance(nod, tests=bad, backend="ref")
    with pytest.raises(ValueError):
        importance(nod, tests={"p": {}}, backend="ref")


# -- files and the command --------------------------------------------------
def test_json_round_trip(tmp_path):
    from flake16_framework_amd.engine.detector import fit_detector
    from flake16_framework_amd.engine.importance import (
        importance, write_importance,
    )
    tests = _hand_tests()
    det = fit_detector(DT, tests=tests, seed=0, backend="ref")
    out = tmp_path / "imp.json"
    res = write_importance(det, tests=tests, out_file=str(out), repeats=2,
                           backend="ref")
    assert res == importance(det, tests=tests, repeats=2, backend="ref")
    text = out.read_text()
    assert "null" in text and "NaN" not in text
    doc = json.loads(text)
    assert doc.pop("config_keys") == list(res["config_keys"])
    want = dict(res)
    del want["config_keys"]
    assert doc == want                                   # None <-> null
    assert doc["baseline"]["projects"]["b"][3:] == [None, None, None]


def test_cli(tests5, tmp_path, monkeypatch, capsys):
    from flake16_framework_amd import cli
    from flake16_framework_amd.engine.detector import Detector
    from flake16_framework_amd.engine.importance import (
        holdout_importance, importance,
    )
    monkeypatch.chdir(tmp_path)
    with open("tests.json", "w") as fd:
        json.dump(tests5, fd)
    cli.main(["fit", "--config", "nod", "--backend", "ref", "--n-trees",
              "4"])
    cli.main(["importance", "--backend", "ref", "--repeats", "2", "--seed",
              "3"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert "importance.json" in line and "baseline F1" in line
    assert "19 groups x 2 repeats" in line and "argmax" in line
    want = importance(Detector.load("detector.npz"), tests=tests5,
                      repeats=2, seed=3, backend="ref")
    with open("importance.json") as fd:
        doc = json.load(fd)
    assert doc["importance"] == want["importance"]
    assert doc["baseline"] == want["baseline"]
    assert (doc["seed"], doc["repeats"], doc["rule"]) == (3, 2, "argmax")
    top = max(want["importance"],
              key=lambda n: want["importance"][n]["f1_drop_mean"])
    assert f"{top} " in line

    cli.main(["importance", "--backend", "ref", "--repeats", "1",
              "--threshold", "0.25", "--out", "thr.json"])
    with open("thr.json") as fd:
        doc = json.load(fd)
    assert (doc["rule"], doc["threshold"]) == ("threshold", 0.25)

    cli.main(["importance", "--holdout", "--keys", *PCA_FF, "--backend",
              "ref", "--n-trees", "3", "--repeats", "1", "--out",
              "loo.json"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert "loo.json" in line and "leave-one-project-out" in line
    want = holdout_importance(PCA_FF, tests=tests5, n_trees=3, repeats=1,
                              backend="ref")
    with open("loo.json") as fd:
        doc = json.load(fd)
    assert doc["config_keys"] == list(PCA_FF)
    assert doc["importance"] == want["importance"]
    assert list(doc["groups"])[:3] == list(FEATURE_NAMES[:3])  # raw names
