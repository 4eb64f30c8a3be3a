"""similar on the CPU: the ref backend against a brute-force double loop,
leaf ids read off a hand-built forest, identical rows, skip_self,
flaky_only, padding, a one-tree detector, the JSON file and the command."""

import json

import numpy as np
import pytest

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests

NOD = SHAP_CONFIGS[0]
DT = ("NOD", "Flake16", "None", "None", "Decision Tree")
N_TREES = 7


@pytest.fixture(scope="module")
def corpus300():
    return make_synthetic_tests(n_tests=300, n_projects=5, seed=2)


@pytest.fixture(scope="module")
def queries():
    # other values under partly the same (project, nodeid) names
    return make_synthetic_tests(n_tests=120, n_projects=5, seed=3)


@pytest.fixture(scope="module")
def fitted(corpus300):
    from flake16_framework_amd.engine.detector import fit_detector
    return fit_detector(NOD, tests=corpus300, seed=0, backend="ref",
                        n_trees=N_TREES)


def _leaf_rows(detector, tests):
    """Leaf ids by walking every row down every tree, one step at a time,
    on the detector's own arrays."""
    from flake16_framework_amd.engine.detector import load_rows
    from flake16_framework_amd.engine.similar import _codes_ref
    X, projects, nodeids = load_rows(detector, tests, None)
    codes = _codes_ref(detector, X)
    out = np.zeros((len(X), detector.n_trees), dtype=np.int64)
    for i in range(len(X)):
        for t in range(detector.n_trees):
            base, node = int(detector.tree_off[t]), 0
            while detector.feat[base + node] >= 0:
                f = detector.feat[base + node]
                left = detector.left[base + node]
                go_left = codes[i, f] <= detector.split[base + node]
                node = int(left if go_left else left + 1)
            out[i, t] = node
    return out, projects, nodeids


def _brute(leaf_q, leaf_c, self_idx, k):
    idx = np.full((len(leaf_q), k), -1, dtype=np.int32)
    shared = np.zeros((len(leaf_q), k), dtype=np.int32)
    for q in range(len(leaf_q)):
        cand = []
        for c in range(len(leaf_c)):
            if c == self_idx[q]:
                continue
            s = sum(int(a == b) for a, b in zip(leaf_q[q], leaf_c[c]))
            cand.append((-s, c))
        for j, (neg, c) in enumerate(sorted(cand)[:k]):
            idx[q, j], shared[q, j] = c, -neg
    return idx, shared


@pytest.mark.parametrize("skip_self", [True, False])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_ref_against_brute_force(k, skip_self, corpus300, queries, fitted):
    from flake16_framework_amd.engine.detector import detect
    from flake16_framework_amd.engine.similar import similar
    res = similar(fitted, tests=queries, corpus=corpus300, k=k,
                  skip_self=skip_self, backend="ref")
    leaf_q, qp, qn = _leaf_rows(fitted, queries)
    leaf_c, cp, cn = _leaf_rows(fitted, corpus300)
    where = {(p, n): i for i, (p, n) in enumerate(zip(cp, cn))}
    self_idx = [where.get((p, n), -1) if skip_self else -1
                for p, n in zip(qp, qn)]
    assert skip_self is False or max(self_idx) >= 0   # names do overlap
    idx, shared = _brute(leaf_q, leaf_c, self_idx, k)
    assert res["idx"].dtype == res["shared"].dtype == np.int32
    assert np.array_equal(res["idx"], idx)
    assert np.array_equal(res["shared"], shared)
    assert res["k"] == k and res["n_trees"] == N_TREES
    assert res["n_candidates"] == 300

    det = detect(fitted, tests=queries, backend="ref")
    for name in ("proba", "pred", "projects", "nodeids"):
        assert np.array_equal(res[name], det[name]), name
    assert res["pred"].dtype == np.uint8
    assert np.array_equal(res["corpus_projects"], cp)
    assert np.array_equal(res["corpus_nodeids"], cn)
    labels = [row[1] == fitted.flaky_label for rows in corpus300.values()
              for row in rows.values()]
    assert res["corpus_labels"].tolist() == labels


# -- a forest whose leaf ids can be read off by eye -------------------------
def _two_tree_detector():
    """Tree 0:  f0 <= cut ? leaf 1 : (f1 <= cut ? leaf 3 : leaf 4)
    Tree 1:  f1 <= cut ? leaf 1 : leaf 2.      Both cuts are 0.0, and
    code = #{cut <= x}, so x < 0 goes left and x >= 0 right."""
    from flake16_framework_amd.engine.detector import assemble_detector
    from flake16_framework_amd.models.forest_ref import Tree
    F = 16
    params = {"spec": None, "mean": np.zeros(F), "scale": np.ones(F),
              "pca_mean": np.zeros(F), "W": np.eye(F)}
    cuts = [np.array([0.0], dtype=np.float32)] * 2 + [
        np.zeros(0, dtype=np.float32)] * (F - 2)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    t0 = Tree(i32(0, -1, 1, -1, -1), i32(0, 0, 0, 0, 0),
              np.zeros(5, dtype=np.float32), i32(1, -1, 3, -1, -1),
              i32(2, -1, 4, -1, -1), np.array([4.0, 2.0, 2.0, 1.0, 1.0]),
              np.array([4.0, 1.0, 3.0, 1.0, 2.0]))
    t1 = Tree(i32(1, -1, -1), i32(0, 0, 0), np.zeros(3, dtype=np.float32),
              i32(1, -1, -1), i32(2, -1, -1), np.array([3.0, 2.0, 1.0]),
              np.array([3.0, 1.0, 2.0]))
    keys = ("NOD", "Flake16", "None", "None", "Random Forest")
    return assemble_detector(keys, 2, tuple(range(16)), params, cuts,
                             [t0, t1], 2, 0, 8)


def _file(rows, proj="p", label=None):
    """{proj: {name: row}} from (f0, f1) pairs; label defaults to 0."""
    label = label or [0] * len(rows)
    return {proj: {f"t{i}": [0, label[i], f0, f1] + [0.0] * 14
                   for i, (f0, f1) in enumerate(rows)}}


def test_leaf_ids_by_hand():
    from flake16_framework_amd.engine.similar import (
        _codes_ref, leaves_ref, similar,
    )
    det = _two_tree_detector()
    rows = [(-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0), (0.0, 0.0)]
    X = np.zeros((5, 16))
    X[:, :2] = rows
    assert leaves_ref(det, _codes_ref(det, X)).tolist() == [
        [1, 1], [1, 2], [3, 1], [4, 2], [4, 2]]

    # query (1, 1) -> leaves (4, 2): rows 3 and 4 share both, row 1 one
    res = similar(det, tests=_file([(1.0, 1.0)], proj="q"),
                  corpus=_file(rows), k=5, backend="ref")
    assert res["idx"].tolist() == [[3, 4, 1, 0, 2]]
    assert res["shared"].tolist() == [[2, 2, 1, 0, 0]]


def test_identical_rows_rank_first_and_by_index(corpus300, fitted):
    """Rows equal to the query share every tree; among them the lower
    corpus index wins, wherever they sit in the file."""
    from flake16_framework_amd.engine.similar import similar
    proj = list(corpus300)[2]
    nid = list(corpus300[proj])[4]
    query = {"elsewhere": {"the_query": list(corpus300[proj][nid])}}
    corpus = {p: dict(rows) for p, rows in corpus300.items()}
    last = list(corpus)[-1]
    corpus[last]["a_copy"] = list(corpus300[proj][nid])
    res = similar(fitted, tests=query, corpus=corpus, k=5, backend="ref")
    names = list(zip(res["corpus_projects"], res["corpus_nodeids"]))
    first, second = names.index((proj, nid)), names.index((last, "a_copy"))
    assert first < second
    same = int((res["shared"][0] == N_TREES).sum())
    assert same >= 2
    assert res["idx"][0, :2].tolist() == sorted(res["idx"][0, :same])[:2]
    assert first in res["idx"][0, :same] and (
        second in res["idx"][0, :same] or same == 5)
    assert (np.diff(res["shared"][0]) <= 0).all()


def test_skip_self_removes_exactly_the_same_name(corpus300, fitted):
    from flake16_framework_amd.engine.similar import similar
    kept = similar(fitted, tests=corpus300, corpus=corpus300, k=4,
                   skip_self=False, backend="ref")
    skipped = similar(fitted, tests=corpus300, corpus=corpus300, k=4,
                      skip_self=True, backend="ref")
    M = len(kept["pred"])
    rows = np.arange(M)
    assert (kept["shared"][:, 0] == N_TREES).all()
    assert not (skipped["idx"] == rows[:, None]).any()
    for q in range(M):
        # the kept list is the skipped list with q put in at its rank
        full = kept["idx"][q].tolist()
        if q in full:
            full.remove(q)
            assert full == skipped["idx"][q, :3].tolist()
        else:       # q tied at T with four lower-indexed rows
            assert (kept["shared"][q] == N_TREES).all()
            assert (kept["idx"][q] < q).all()
    # an identical row under another name is not skipped
    proj = list(corpus300)[0]
    nid = list(corpus300[proj])[0]
    res = similar(fitted, tests={"x": {"y": list(corpus300[proj][nid])}},
                  corpus=corpus300, k=1, skip_self=True, backend="ref")
    assert res["shared"][0, 0] == N_TREES


def test_keep_self_puts_the_row_first():
    """Distinct leaf vectors: only the row itself shares both trees."""
    from flake16_framework_amd.engine.similar import similar
    det = _two_tree_detector()
    rows = [(-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0)]
    corpus = _file(rows)
    kept = similar(det, tests=corpus, corpus=corpus, k=2, skip_self=False,
                   backend="ref")
    assert kept["idx"][:, 0].tolist() == [0, 1, 2, 3]
    assert kept["shared"][:, 0].tolist() == [2, 2, 2, 2]
    skipped = similar(det, tests=corpus, corpus=corpus, k=2, backend="ref")
    assert skipped["idx"].tolist() == [[1, 2], [0, 3], [0, 1], [1, 0]]
    assert skipped["shared"].tolist() == [[1, 1], [1, 1], [1, 0], [1, 0]]


def test_flaky_only_maps_back_to_the_whole_corpus(corpus300, queries,
                                                  fitted):
    from flake16_framework_amd.engine.similar import similar
    res = similar(fitted, tests=queries, corpus=corpus300, k=5,
                  flaky_only=True, backend="ref")
    labels = res["corpus_labels"]
    assert 5 < labels.sum() < 300
    assert res["n_candidates"] == int(labels.sum())
    assert (res["idx"] >= 0).all() and labels[res["idx"]].all()

    leaf_q, qp, qn = _leaf_rows(fitted, queries)
    leaf_c, cp, cn = _leaf_rows(fitted, corpus300)
    keep = np.flatnonzero(labels)
    where = {(cp[i], cn[i]): j for j, i in enumerate(keep)}
    self_idx = [where.get((p, n), -1) for p, n in zip(qp, qn)]
    idx, shared = _brute(leaf_q, leaf_c[keep], self_idx, 5)
    assert np.array_equal(res["idx"], keep[idx])
    assert np.array_equal(res["shared"], shared)


def test_padding_empty_files_and_one_tree(corpus300):
    from flake16_framework_amd.engine.detector import fit_detector
    from flake16_framework_amd.engine.similar import similar
    det = _two_tree_detector()
    rows = [(-1.0, -1.0), (1.0, 1.0), (1.0, -1.0)]
    res = similar(det, tests=_file(rows), corpus=_file(rows), k=5,
                  backend="ref")                    # two candidates each
    # leaves: (1, 1), (4, 2), (3, 1); only rows 0 and 2 share a leaf
    assert res["idx"].tolist() == [
        [2, 1, -1, -1, -1], [0, 2, -1, -1, -1], [0, 1, -1, -1, -1]]
    assert res["shared"].tolist() == [
        [1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0]]

    none = similar(det, tests=_file(rows), corpus={"p": {}}, k=3,
                   backend="ref")
    assert none["idx"].tolist() == [[-1] * 3] * 3
    assert none["shared"].tolist() == [[0] * 3] * 3
    assert none["corpus_labels"].shape == (0,)
    empty = similar(det, tests={}, corpus=_file(rows), k=3, backend="ref")
    assert empty["idx"].shape == empty["shared"].shape == (0, 3)
    assert empty["proba"].shape == empty["pred"].shape == (0,)
    only_clean = similar(det, tests=_file(rows), corpus=_file(rows), k=2,
                         flaky_only=True, backend="ref")
    assert only_clean["idx"].tolist() == [[-1, -1]] * 3

    tree = fit_detector(DT, tests=corpus300, seed=0, backend="ref")
    assert tree.n_trees == 1
    res = similar(tree, tests=corpus300, corpus=corpus300, k=16,
                  backend="ref")
    assert set(np.unique(res["shared"])) <= {0, 1}
    assert (np.diff(res["shared"], axis=1) <= 0).all()


def test_errors(corpus300, fitted):
    from flake16_framework_amd.engine.similar import similar
    for k in (0, 17, -1):
        with pytest.raises(ValueError):
            similar(fitted, tests=corpus300, corpus=corpus300, k=k,
                    backend="ref")
    with pytest.raises(ValueError):
        similar(fitted, tests=corpus300, corpus=corpus300, backend="cuda")
    bad = {"p": {"t": [0, 0] + [float("nan")] * 16}}
    with pytest.raises(ValueError):
        similar(fitted, tests=bad, corpus=corpus300, backend="ref")


def test_json_drops_zero_counts_and_padding(tmp_path):
    from flake16_framework_amd.engine.similar import write_similar
    det = _two_tree_detector()
    rows = [(-1.0, -1.0), (1.0, 1.0), (1.0, -1.0)]
    out = tmp_path / "similar.json"
    res = write_similar(det, tests=_file([(1.0, 1.0), (-1.0, 1.0)], "q"),
                        corpus=_file(rows, label=[2, 0, 2]), out_file=out,
                        k=5, backend="ref")
    doc = json.loads(out.read_text())
    assert set(doc) == {"k", "n_trees", "corpus_tests", "tests"}
    assert (doc["k"], doc["n_trees"], doc["corpus_tests"]) == (5, 2, 3)
    # (1, 1) -> leaves (4, 2): row 1 shares both, rows 0 and 2 nothing
    # (-1, 1) -> leaves (1, 2): row 0 shares tree 0, row 1 tree 1
    assert res["shared"].tolist() == [[2, 0, 0, 0, 0], [1, 1, 0, 0, 0]]
    assert doc["tests"] == {"q": {
        "t0": [float(res["proba"][0]), int(res["pred"][0]),
               [["p", "t1", 0, 2]]],
        "t1": [float(res["proba"][1]), int(res["pred"][1]),
               [["p", "t0", 1, 1], ["p", "t1", 0, 1]]]}}


def test_cli(corpus300, queries, tmp_path, monkeypatch, capsys):
    from flake16_framework_amd import cli
    from flake16_framework_amd.engine.detector import Detector
    from flake16_framework_amd.engine.similar import similar
    monkeypatch.chdir(tmp_path)
    (tmp_path / "tests.json").write_text(json.dumps(corpus300))
    (tmp_path / "new.json").write_text(json.dumps(queries))
    cli.main(["fit", "--config", "nod", "--backend", "ref", "--n-trees",
              "5"])
    capsys.readouterr()
    cli.main(["similar", "--tests-file", "new.json", "--backend", "ref",
              "--k", "3"])
    line = capsys.readouterr().out
    assert "wrote similar.json (120 tests against 300 corpus tests, k 3" \
        in line
    det = Detector.load("detector.npz")
    want = similar(det, tests=queries, corpus=corpus300, k=3, backend="ref")
    doc = json.loads((tmp_path / "similar.json").read_text())
    assert (doc["k"], doc["n_trees"], doc["corpus_tests"]) == (3, 5, 300)
    q = 0
    for proj, rows in queries.items():
        for nid in rows:
            proba, pred, near = doc["tests"][proj][nid]
            assert proba == float(want["proba"][q])
            assert pred == int(want["pred"][q])
            keep = want["shared"][q] > 0
            assert [n[3] for n in near] == want["shared"][q][keep].tolist()
            assert [n[1] for n in near] == \
                want["corpus_nodeids"][want["idx"][q][keep]].tolist()
            q += 1
    flagged = want["pred"] == 1
    hits = want["corpus_labels"][want["idx"][flagged, 0]].sum()
    assert f"{int(flagged.sum())} predicted flaky" in line
    assert f"{hits / flagged.sum():.4f}" in line

    # the corpus queried against itself: --keep-self returns each test
    cli.main(["similar", "--out", "self.json", "--backend", "ref", "--k",
              "1", "--keep-self", "--flaky-only"])
    capsys.readouterr()
    doc = json.loads((tmp_path / "self.json").read_text())
    assert doc["corpus_tests"] == int(want["corpus_labels"].sum())
    for proj, rows in corpus300.items():
        for nid, row in rows.items():
            near = doc["tests"][proj][nid][2]
            assert all(n[2] == 1 for n in near)
            if row[1] == det.flaky_label:
                assert near[0][3] == 5

    for k in ("0", "17"):
        with pytest.raises(ValueError):
            cli.main(["similar", "--backend", "ref", "--k", k])
