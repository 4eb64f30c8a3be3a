"""GPU tests for the deferred mid/small subtree drain in forest_fit.

The level loop only splits the > 2048-sample band; children routed to the
mid (65..2048) and small (<= 64) queues accumulate, tagged with the sample
buffer they live in, and are drained once after the band is exhausted (or
earlier when a queue passes its threshold).  Trees must stay bit-identical
to models/forest_ref.py under every schedule.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_DEEP = 6000
JOB_BASE = 40
# (kind, n_trees, max_features, bootstrap, random splitter)
DEEP_MODELS = [
    ("extra_trees", 3, 4, 0, 1),
    ("random_forest", 3, 4, 1, 0),
    ("decision_tree", 1, 16, 0, 0),
]
RAGGED_SIZES = [6000, 2100, 2048, 500, 65, 64, 2]


@pytest.fixture(scope="module")
def ops():
    from flake16_framework_amd.ops.backend import get_ops
    return get_ops()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def deep_data():
    """Sparse codes: most samples share bin 0 on most features, so splits
    peel a few samples at a time and the > 2048-sample band runs 27-41
    levels deep, routing mid and small children at both depth parities."""
    rng = np.random.RandomState(7)
    n = N_DEEP
    codes = ((rng.rand(n, 16) < 0.08)
             * rng.randint(1, 8, (n, 16))).astype(np.uint8)
    y = (rng.rand(n) < 0.3).astype(np.uint8)
    return codes, y


def _ref_params(kind, n_trees):
    from flake16_framework_amd.models.forest_ref import params_for_model
    params = params_for_model({"kind": kind, "n_estimators": n_trees}, seed=0)
    params.n_trees = n_trees
    return params


@pytest.fixture(scope="module")
def deep_refs(deep_data):
    """Reference forests for DEEP_MODELS, computed once and left unchanged."""
    from flake16_framework_amd.models.forest_ref import fit_forest
    codes, y = deep_data
    return [fit_forest(codes, y, _ref_params(kind, n_trees),
                       job_base=JOB_BASE)
            for kind, n_trees, _, _, _ in DEEP_MODELS]


def _fit_multi(ops, dev, codes, y, jobs):
    """jobs: list of (n_prefix, key, max_features, bootstrap, random)."""
    codes_d = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
    y_d = torch.from_numpy(y).to(dev)
    col = lambda i, dt: torch.tensor([j[i] for j in jobs], dtype=dt)
    j_row_off = torch.zeros(len(jobs), dtype=torch.int32, device=dev)
    out = ops.forest_fit_multi(
        codes_d, y_d, j_row_off, col(0, torch.int32),
        col(1, torch.int32).to(dev), col(2, torch.int32),
        col(4, torch.uint8), col(3, torch.uint8), 16, 0)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _deep_jobs():
    return [(N_DEEP, JOB_BASE + t, mf, boot, rnd)
            for _, n_trees, mf, boot, rnd in DEEP_MODELS
            for t in range(n_trees)]


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


def test_deep_band_both_parities(ops, dev, deep_data, deep_refs):
    codes, y = deep_data
    out = _fit_multi(ops, dev, codes, y, _deep_jobs())
    _assert_trees_equal(out, [t for f in deep_refs for t in f.trees])


def test_ragged_batch(ops, dev, deep_data, deep_refs):
    """Jobs that finish early (down to 2 samples: never in the band) must
    not disturb the ones still in it."""
    from flake16_framework_amd.models.forest_ref import fit_forest
    codes, y = deep_data
    jobs, expected = [], []
    for i, m in enumerate(RAGGED_SIZES):
        for ri, (kind, _, mf, boot, rnd) in enumerate(DEEP_MODELS[:2]):
            key = JOB_BASE + 8 * i
            jobs.append((m, key, mf, boot, rnd))
            if m == N_DEEP:   # first tree of the shared reference
                expected.append(deep_refs[ri].trees[0].n_nodes)
            else:
                ref = fit_forest(codes[:m], y[:m], _ref_params(kind, 1),
                                 job_base=key)
                expected.append(ref.trees[0].n_nodes)
    out = _fit_multi(ops, dev, codes, y, jobs)
    np.testing.assert_array_equal(out[6], expected)


def test_forced_early_drains(ops, dev, deep_data, deep_refs, monkeypatch):
    """A threshold of 8 items drains and resets both queues at every chunk
    sync of the band; the trees must not change."""
    monkeypatch.setenv("FLAKE16_DRAIN_AT", "8")
    codes, y = deep_data
    out = _fit_multi(ops, dev, codes, y, _deep_jobs())
    _assert_trees_equal(out, [t for f in deep_refs for t in f.trees])


def test_schedule_equivalence(ops, monkeypatch):
    """Deferred drain (default) vs the per-level drain schedule."""
    from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
    from flake16_framework_amd.engine.scores import run_scores

    tests = make_synthetic_tests(400, seed=2)
    monkeypatch.delenv("FLAKE16_LEVEL_DRAIN", raising=False)
    deferred = run_scores(tests=tests, backend="hip", cells=[0, 1, 107])
    monkeypatch.setenv("FLAKE16_LEVEL_DRAIN", "1")
    per_level = run_scores(tests=tests, backend="hip", cells=[0, 1, 107])
    assert set(deferred) == set(per_level) and len(deferred) == 3
    for keys in deferred:
        assert deferred[keys][2] == per_level[keys][2], keys
        assert deferred[keys][3] == per_level[keys][3], keys
