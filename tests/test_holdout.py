"""holdout on the CPU: the ref backend against the definition (a loop of
fit_detector + detect written here), the counting rules on a hand-written
table, edge cases and the command."""

import json

import numpy as np
import pytest

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests

CONFIGS = {
    "nod": SHAP_CONFIGS[0],
    "od": SHAP_CONFIGS[1],
    "pca-flakeflagger": ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN",
                         "Random Forest"),
}
N_TREES = 12

# (acc0, acc1, label, project) with n_trees = 4 and K = 5: probabilities
# fall exactly on the thresholds 0, .25, .5, .75, 1.
#   A  one of each argmax outcome; row 2 is a tie: argmax says 0, the 0.5
#      threshold says 1
#   B  no flaky test (recall undefined); row 8 is a tie on a negative
#   C  both flaky tests missed by argmax (precision undefined)
TABLE = [
    (0, 4, 1, "A"), (2, 2, 1, "A"), (1, 3, 0, "A"), (4, 0, 0, "A"),
    (3, 1, 0, "B"), (4, 0, 0, "B"), (0, 4, 0, "B"), (2, 2, 0, "B"),
    (3, 1, 1, "C"), (4, 0, 1, "C"), (4, 0, 0, "C"), (3, 1, 0, "C"),
]
TABLE_TREES, TABLE_K = 4, 5
TABLE_SEG = [0, 4, 8, 12]
# [FP, FN, TP] written out by hand; last entry pooled
TABLE_ARGMAX = [[1, 1, 1], [1, 0, 0], [0, 2, 0], [2, 3, 1]]
TABLE_CURVE = [
    [[2, 0, 2], [1, 0, 2], [1, 0, 2], [1, 1, 1], [0, 1, 1]],
    [[4, 0, 0], [3, 0, 0], [2, 0, 0], [1, 0, 0], [1, 0, 0]],
    [[2, 0, 2], [1, 1, 1], [0, 2, 0], [0, 2, 0], [0, 2, 0]],
    [[8, 0, 4], [5, 1, 3], [3, 2, 2], [2, 3, 1], [1, 3, 1]],
]


def table_arrays():
    t = np.array([r[:3] for r in TABLE], dtype=np.float64)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].astype(np.uint8)


@pytest.fixture(scope="module")
def tests5():
    return make_synthetic_tests(n_tests=300, n_projects=5, seed=2)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ref_is_the_definition(name, tests5):
    from flake16_framework_amd.engine.detector import detect, fit_detector
    from flake16_framework_amd.engine.holdout import holdout
    keys = CONFIGS[name]
    res = holdout(keys, tests=tests5, backend="ref", n_trees=N_TREES,
                  keep_detectors=True)

    proba, pred, nodeids, dets = [], [], [], []
    for held in tests5:
        train = {p: rows for p, rows in tests5.items() if p != held}
        det = fit_detector(keys, tests=train, seed=0, backend="ref",
                           n_trees=N_TREES)
        out = detect(det, tests={held: tests5[held]}, backend="ref")
        proba.append(out["proba"])
        pred.append(out["pred"])
        nodeids += list(out["nodeids"])
        dets.append(det)
    np.testing.assert_array_equal(res["oof"]["proba"],
                                  np.concatenate(proba))
    np.testing.assert_array_equal(res["oof"]["pred"], np.concatenate(pred))
    assert list(res["oof"]["nodeids"]) == nodeids
    assert list(res["oof"]["projects"]) == [
        p for p, rows in tests5.items() for _ in rows]

    assert len(res["detectors"]) == len(tests5) == 5
    for got, want in zip(res["detectors"], dets):
        a, b = got.arrays(), want.arrays()
        assert a.keys() == b.keys()
        for field in a:
            np.testing.assert_array_equal(a[field], b[field], err_msg=field)

    N = sum(len(rows) for rows in tests5.values())
    assert list(res["projects"]) == list(tests5)
    for proj, entry in res["projects"].items():
        assert entry["n_test"] == len(tests5[proj])
        assert entry["n_train"] + entry["n_test"] == N
        assert len(entry["curve"]) == 101
    assert res["n_trees"] == N_TREES and res["config_keys"] == keys
    np.testing.assert_array_equal(res["thresholds"],
                                  np.arange(101) / 100)
    # the rules agree with recounting the returned arrays
    flaky = np.concatenate([[row[1] == 2 if keys[0] == "NOD" else
                             row[1] == 1 for row in rows.values()]
                            for rows in tests5.values()])
    p = res["oof"]["pred"].astype(bool)
    assert res["total"]["argmax"][:3] == [
        int((p & ~flaky).sum()), int((~p & flaky).sum()),
        int((p & flaky).sum())]
    assert res["total"]["n_flaky"] == int(flaky.sum())
    assert res["total"]["curve"][0] == [int((~flaky).sum()), 0,
                                        int(flaky.sum())]


def test_counts_on_hand_written_table():
    from flake16_framework_amd.engine.holdout import (
        best_f1_threshold, counts_ref, curve_prf, make_thresholds,
    )
    acc0, acc1, labels = table_arrays()
    thresholds = make_thresholds(TABLE_K)
    np.testing.assert_array_equal(thresholds, [0, .25, .5, .75, 1])
    proba = acc1 / TABLE_TREES
    pred = acc1 > acc0
    curve, argmax = counts_ref(proba, pred, labels, TABLE_SEG, thresholds)
    assert curve.dtype == argmax.dtype == np.int32
    assert argmax.tolist() == TABLE_ARGMAX
    assert curve.tolist() == TABLE_CURVE

    # the tie: argmax says 0, the 0.5 threshold says 1
    assert acc0[1] == acc1[1] and not pred[1] and proba[1] >= thresholds[2]
    assert argmax[0].tolist() != curve[0, 2].tolist()

    n_pos, n_neg = int(labels.sum()), int((labels == 0).sum())
    assert curve[-1, 0].tolist() == [n_neg, 0, n_pos]
    for g in range(4):
        assert (np.diff(curve[g, :, 0]) <= 0).all()      # FP
        assert (np.diff(curve[g, :, 2]) <= 0).all()      # TP
        assert (curve[g, :, 1] + curve[g, :, 2] == curve[g, 0, 2]).all()
    np.testing.assert_array_equal(curve[:3].sum(axis=0), curve[3])
    np.testing.assert_array_equal(argmax[:3].sum(axis=0), argmax[3])

    # zero denominators: B has no flaky test, C predicts none at k >= 2
    assert curve_prf(curve[1])[0] == [0.0, None, None]
    assert curve_prf(curve[2])[2] == [None, 0.0, None]
    assert curve_prf(curve[0])[4] == [1.0, 0.5, 2 * 0.5 / 1.5]
    prf = curve_prf(curve[3])
    assert prf[1] == [3 / 8, 3 / 4, 2 * (3 / 8) * (3 / 4) / (3 / 8 + 3 / 4)]

    # A: thresholds .25 and .5 have the same counts and the largest F1
    # (P 2/3, R 1); the lowest threshold wins the tie
    assert curve[0, 1].tolist() == curve[0, 2].tolist()
    k, t, f = best_f1_threshold(curve[0], thresholds)
    assert (k, t) == (1, 0.25) and f == curve_prf(curve[0])[1][2]
    assert f == max(p[2] for p in curve_prf(curve[0]))
    # no F1 anywhere gives None
    assert best_f1_threshold(curve[1], thresholds) is None


def test_thresholds_validated():
    from flake16_framework_amd.engine.holdout import make_thresholds
    assert make_thresholds(1).tolist() == [0.0]
    assert make_thresholds(2).tolist() == [0.0, 1.0]
    for bad in (0, 257):
        with pytest.raises(ValueError):
            make_thresholds(bad)


def test_one_project_raises(tests5):
    from flake16_framework_amd.engine.holdout import holdout
    name = next(iter(tests5))
    with pytest.raises(ValueError):
        holdout(CONFIGS["nod"], tests={name: tests5[name]}, backend="ref",
                n_trees=2)


def test_single_class_training_fold(tests5):
    """All NOD-flaky tests moved into one project: the fold holding it out
    trains on a single class and still reports, and the other projects
    have no flaky test, so their recall is None."""
    from flake16_framework_amd.engine.holdout import holdout
    names = list(tests5)
    tests = {p: {} for p in names}
    for p, rows in tests5.items():
        for nid, row in rows.items():
            tests[names[0] if row[1] == 2 else p][f"{p}::{nid}"] = row
    n_flaky = sum(row[1] == 2 for row in tests[names[0]].values())
    assert n_flaky > 0

    res = holdout(CONFIGS["nod"], tests=tests, backend="ref", n_trees=3,
                  n_thresholds=5, keep_detectors=True)
    lone = res["detectors"][0]
    assert (np.diff(lone.tree_off) == 1).all()           # single-leaf trees
    first = res["projects"][names[0]]
    assert first["n_flaky"] == n_flaky
    assert first["argmax"][:3] == [0, n_flaky, 0]        # never predicted
    assert first["argmax"][3:] == [None, 0.0, None]
    for p in names[1:]:
        entry = res["projects"][p]
        assert entry["n_flaky"] == 0
        assert entry["argmax"][1:3] == [0, 0]
        assert entry["argmax"][4] is None
    assert res["total"]["curve"][0][2] == n_flaky


def test_cli_round_trip(tests5, tmp_path, monkeypatch, capsys):
    from flake16_framework_amd import cli
    from flake16_framework_amd.engine.holdout import holdout
    monkeypatch.chdir(tmp_path)
    with open("tests.json", "w") as fd:
        json.dump(tests5, fd)
    cli.main(["holdout", "--config", "od", "--backend", "ref", "--n-trees",
              "4", "--thresholds", "11", "--detections", "oof.json"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert "holdout.json" in line and "best-F1 threshold" in line

    want = holdout(CONFIGS["od"], tests=tests5, backend="ref", n_trees=4,
                   n_thresholds=11)
    with open("holdout.json") as fd:
        doc = json.load(fd)
    assert set(doc) == {"config_keys", "seed", "n_trees", "thresholds",
                        "projects", "total"}
    assert tuple(doc["config_keys"]) == want["config_keys"]
    assert doc["thresholds"] == want["thresholds"].tolist()
    assert doc["projects"] == want["projects"]            # None <-> null
    assert doc["total"] == want["total"]
    assert (doc["seed"], doc["n_trees"]) == (0, 4)

    with open("oof.json") as fd:
        oof = json.load(fd)
    flat = [(p, nid, v) for p, rows in oof.items()
            for nid, v in rows.items()]
    assert [f[0] for f in flat] == list(want["oof"]["projects"])
    assert [f[1] for f in flat] == list(want["oof"]["nodeids"])
    assert [f[2][0] for f in flat] == want["oof"]["proba"].tolist()
    assert [f[2][1] for f in flat] == want["oof"]["pred"].tolist()

    cli.main(["holdout", "--keys", *CONFIGS["pca-flakeflagger"],
              "--backend", "ref", "--n-trees", "2", "--thresholds", "3",
              "--out", "ff.json"])
    with open("ff.json") as fd:
        assert json.load(fd)["config_keys"] == list(
            CONFIGS["pca-flakeflagger"])
