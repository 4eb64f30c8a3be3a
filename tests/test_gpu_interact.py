"""GPU tests for interact: the detector_shap.hip kernels against the numpy
reference bit for bit on the hand-built detectors of test_gpu_explain
(16-element leaves, root leaves, a chain, rows on interval edges) and on
hip-fitted detectors."""

import numpy as np
import pytest
import torch

from test_gpu_explain import (
    M_POOL, _as_tests, _check_edges, _hand_built, _leaf, _tree,
)

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests

pytestmark = pytest.mark.gpu

FIELDS = ("proba", "pred", "phi", "interactions", "projects", "nodeids")


def _assert_same(got, want, m=None):
    for key in FIELDS:
        np.testing.assert_array_equal(got[key], want[key][:m], err_msg=key)
    assert got["base_value"] == want["base_value"]
    assert got["feature_names"] == want["feature_names"]


def _raw(ops, det, paths, X):
    """(codes, table, phi, raw op output) on the device."""
    from flake16_framework_amd.engine.explain import explain_device
    from flake16_framework_amd.engine.interact import device_interactions
    codes, table, _, phi = explain_device(ops, det, paths, X)
    return codes, table, phi, device_interactions(
        ops, codes, table, phi, det.n_trees, det.n_features)


def _check_positions(paths, F):
    """The dropped element sits at either end of a path: some leaf has its
    conditioned feature g as the first of several elements and some leaf
    has it as the last, on the longest path (F elements) among others."""
    n_el = np.diff(paths.leaf_off)
    assert n_el.max() == F >= 2
    several = np.flatnonzero((n_el >= 2) & (n_el < F))
    assert len(several)
    # the grid runs every g, so each of these leaves is visited with its
    # first and with its last element dropped; they are different features
    first = paths.feature[paths.leaf_off[several]]
    last = paths.feature[paths.leaf_off[several + 1] - 1]
    assert (first != last).all()


@pytest.mark.parametrize("n_trees", [1, 7, 23])
@pytest.mark.parametrize("spec", [None, "scale+pca"])
@pytest.mark.parametrize("F", [16, 7])
def test_kernel_bitwise_on_hand_built(F, spec, n_trees):
    from flake16_framework_amd.engine.detector import FPAD
    from flake16_framework_amd.engine.interact import interact
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    det, X, codes = _hand_built(F, spec, n_trees, seed=100 * F + n_trees)
    paths = build_merged_paths(det)
    _check_edges(det, paths, codes, F, n_trees)
    _check_positions(paths, F)

    want = interact(det, tests=_as_tests(X, det.feature_cols, M_POOL),
                    backend="ref")      # rows are independent: prefixes
    inter = want["interactions"]
    assert inter.shape == (M_POOL, F, F)
    off = inter[:, ~np.eye(F, dtype=bool)]
    assert np.abs(off).max() > 1e-3 and np.ptp(off, axis=0).max() > 1e-3
    assert np.abs(inter.sum(axis=2) - want["phi"]).max() <= 1e-12

    for m in (1, 63, 65, M_POOL):
        got = interact(det, tests=_as_tests(X, det.feature_cols, m),
                       backend="hip")
        assert got["interactions"].dtype == np.float64
        assert got["interactions"].shape == (m, F, F)
        _assert_same(got, want, m)

        raw = _raw(ops, det, paths, X[:m])[3]
        assert raw.dtype == torch.float64
        assert tuple(raw.shape) == (m, FPAD, FPAD)
        raw = raw.cpu().numpy()
        np.testing.assert_array_equal(raw[:, :F, :F], inter[:m])
        assert (raw[:, F:, :] == 0.0).all() and (raw[:, :, F:] == 0.0).all()


@pytest.mark.parametrize("n_trees", [10, 11])
def test_either_side_of_the_tree_block(n_trees):
    from flake16_framework_amd.engine.interact import interact
    from flake16_framework_amd.models.forest_ref import PREDICT_TREE_BLOCK
    assert PREDICT_TREE_BLOCK == 10
    det, X, _ = _hand_built(7, None, n_trees, seed=900 + n_trees)
    tests = _as_tests(X, det.feature_cols, 65)
    _assert_same(interact(det, tests=tests, backend="hip"),
                 interact(det, tests=tests, backend="ref"))


def _root_leaf_forest(det, trees, n_trees):
    from flake16_framework_amd.engine.detector import assemble_detector
    return assemble_detector(
        det.config_keys, 2, tuple(det.feature_cols),
        det.preprocessing_params(), det.cut_list(), trees, n_trees, 0,
        M_POOL)


def test_forest_of_root_leaves():
    """No path elements at all: an empty element table reaches the op."""
    from flake16_framework_amd.engine.interact import interact
    det, X, _ = _hand_built(7, "scale+pca", 1, seed=3)
    rng = np.random.RandomState(4)
    flat = _root_leaf_forest(det, [_tree(_leaf(rng)) for _ in range(3)], 3)
    tests = _as_tests(X, flat.feature_cols, 63)
    got = interact(flat, tests=tests, backend="hip")
    assert got["interactions"].shape == (63, 7, 7)
    assert (got["interactions"] == 0.0).all()
    _assert_same(got, interact(flat, tests=tests, backend="ref"))


def test_rows_in_two_chunks():
    """The op bounds its [T, F, 16, rows] workspace at 256 MiB; with F = 16
    and 512 trees that is 256 rows per chunk, so 257 rows take two chunks.
    Most of the trees are root leaves to keep the forest small."""
    from flake16_framework_amd.engine.interact import interact
    n_trees = 512
    assert (256 << 20) // (n_trees * 16 * 16 * 8) // 256 * 256 == 256
    det, X, _ = _hand_built(16, None, 23, seed=77)
    rng = np.random.RandomState(78)
    trees = det.trees() + [_tree(_leaf(rng)) for _ in range(n_trees - 23)]
    big = _root_leaf_forest(det, trees, n_trees)
    tests = _as_tests(X, big.feature_cols, M_POOL)
    want = interact(big, tests=tests, backend="ref")
    _assert_same(interact(big, tests=tests, backend="hip"), want)
    tail = want["interactions"][255:].reshape(2, -1)
    assert np.ptp(tail, axis=0).max() > 0       # rows 255, 256 differ


def test_rows_in_two_chunks_below_the_padded_width():
    """As test_rows_in_two_chunks with F = 7: the workspace is
    [T, 7, 16, rows] and the grid has 7 slots g, so neither equals the
    padded 16.  1024 trees make a chunk 256 rows again."""
    from flake16_framework_amd.engine.interact import interact
    n_trees, F = 1024, 7
    assert (256 << 20) // (n_trees * F * 16 * 8) // 256 * 256 == 256
    det, X, _ = _hand_built(F, None, 23, seed=79)
    rng = np.random.RandomState(80)
    trees = det.trees() + [_tree(_leaf(rng)) for _ in range(n_trees - 23)]
    big = _root_leaf_forest(det, trees, n_trees)
    tests = _as_tests(X, big.feature_cols, M_POOL)
    want = interact(big, tests=tests, backend="ref")
    _assert_same(interact(big, tests=tests, backend="hip"), want)
    assert want["interactions"].shape == (257, F, F)
    tail = want["interactions"][255:].reshape(2, -1)
    assert np.ptp(tail, axis=0).max() > 0       # rows 255, 256 differ


def test_op_refuses_malformed_input():
    from flake16_framework_amd.engine.explain import device_shap, device_table
    from flake16_framework_amd.engine.interact import device_interactions
    from flake16_framework_amd.models.mergedpaths import build_merged_paths
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    det, X, codes = _hand_built(16, None, 7, seed=5)
    paths = build_merged_paths(det)
    dev = torch.device("cuda:0")
    dev_codes = torch.from_numpy(np.zeros((4, 16), dtype=np.uint8)).to(dev)
    table = device_table(paths, dev)
    phi = device_shap(ops, dev_codes, table, 7, 16)
    device_interactions(ops, dev_codes, table, phi, 7, 16)
    # what detector_shap refuses
    with pytest.raises(RuntimeError):       # an element names feature >= F
        device_interactions(ops, dev_codes, table, phi, 7, 7)
    bad = dict(table, leaf_off=table["leaf_off"].clone())
    bad["leaf_off"][1] = paths.n_elements + 5
    with pytest.raises(RuntimeError):       # offsets step back / too far
        device_interactions(ops, dev_codes, bad, phi, 7, 16)
    with pytest.raises(RuntimeError):       # tree count against the ranges
        device_interactions(ops, dev_codes, table, phi, 6, 16)
    with pytest.raises(RuntimeError):       # dtype
        device_interactions(
            ops, dev_codes, dict(table, elem_z=table["elem_z"].float()),
            phi, 7, 16)
    # and a phi that is not detector_shap's output for these rows
    for wrong in (phi[:3].contiguous(), phi[:, :7].contiguous(),
                  phi.reshape(-1), phi.float(), phi.cpu()):
        with pytest.raises(RuntimeError):
            device_interactions(ops, dev_codes, table, wrong, 7, 16)


@pytest.fixture(scope="module")
def train_tests():
    return make_synthetic_tests(n_tests=300, seed=2)


@pytest.fixture(scope="module")
def other_tests():
    return make_synthetic_tests(n_tests=257, seed=5)


@pytest.mark.parametrize("keys", [
    SHAP_CONFIGS[0], SHAP_CONFIGS[1],
    ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN", "Random Forest"),
], ids=["nod", "od", "pca-flakeflagger"])
def test_fitted_equal_across_backends(keys, train_tests, other_tests,
                                      tmp_path):
    from flake16_framework_amd.engine.detector import fit_detector
    from flake16_framework_amd.engine.interact import write_interactions
    det = fit_detector(keys, tests=train_tests, backend="hip", n_trees=12)
    res = {}
    for backend in ("ref", "hip"):
        res[backend] = write_interactions(
            det, tests=other_tests, out_file=str(tmp_path / backend),
            matrix_out=str(tmp_path / (backend + ".npy")), backend=backend)
    got, want = res["hip"], res["ref"]
    F = det.n_features
    assert got["interactions"].shape == (257, F, F)
    _assert_same(got, want)
    inter = got["interactions"]
    assert np.abs(inter[:, ~np.eye(F, dtype=bool)]).max() > 1e-3
    assert np.abs(inter.sum(axis=2) - got["phi"]).max() <= 1e-12
    for name in ("ref", "ref.npy"):
        with open(tmp_path / name, "rb") as a, \
                open(tmp_path / name.replace("ref", "hip"), "rb") as b:
            assert a.read() == b.read()
