"""GPU tests for importance: the fused permuted_counts op of
ops/hip/importance.hip against a numpy reference and against the existing
grouped ops run per job on an explicitly gathered matrix, integer for
integer, on hand-built groups; the identity permutation; the device
backend of importance() and holdout_importance() against the ref backend;
the op's host checks."""

import numpy as np
import pytest
import torch

from flake16_framework_amd.configgrid import SHAP_CONFIGS
from flake16_framework_amd.constants import FLAKEFLAGGER_COLUMNS
from flake16_framework_amd.dataset.synthetic import make_synthetic_tests
from flake16_framework_amd.models.binning import bin_codes
from flake16_framework_amd.models.forest_ref import (
    Tree, accumulate_proba, canonicalize_tree,
)
from flake16_framework_amd.preprocess import transform_preprocessing

pytestmark = pytest.mark.gpu

M_POOL = 257          # > one 256-thread block and > four 64-row blocks
CHAIN_DEPTH = 24
ONE_CUT, MANY_CUTS, CONST_COL = 0, 1, 2   # feature roles
# rows per group: the empty group first, in the middle, last
GROUP_ORDERS = [(0, 1, 63, 257), (63, 0, 257, 1), (257, 63, 1, 0)]
G = 4


# -- hand-built detectors (the construction of tests/test_gpu_holdout.py,
# -- with tied leaf counts added) -------------------------------------------
def _params(F, spec, rng):
    p = {"spec": spec, "mean": np.zeros(F), "scale": np.ones(F),
         "pca_mean": np.zeros(F), "W": np.eye(F)}
    if spec is not None:
        p["mean"] = rng.uniform(-20.0, 20.0, size=F)
        p["scale"] = rng.uniform(0.05, 30.0, size=F)
        p["scale"][CONST_COL] = 1.0          # zero-variance column
    if spec == "scale+pca":
        p["pca_mean"] = rng.randn(F) * 1e-3
        q, _ = np.linalg.qr(rng.randn(F, F))
        p["W"] = q
    return p


def _pool(F, params, rng):
    X = rng.randn(M_POOL, F) * rng.uniform(0.5, 40.0, size=F)
    X[:, CONST_COL] = 3.5
    if params["spec"] is not None:
        X[:, CONST_COL] = params["mean"][CONST_COL]
    return X


def _cuts_from(T32, rng):
    """Cuts taken FROM the transformed inputs, so inputs (and, without a
    projection, the values a row borrows from its group) equal cut values
    exactly; each column's extremes stay outside the cuts."""
    cuts = []
    for f in range(T32.shape[1]):
        vals = np.unique(T32[:, f])
        inner = vals[1:-1] if len(vals) >= 3 else vals[:1]
        if f == ONE_CUT:
            c = inner[len(inner) // 2:len(inner) // 2 + 1]
        elif f == MANY_CUTS:
            assert len(inner) >= 255
            c = inner[:255]
        else:
            k = min(len(inner), int(rng.randint(1, 40)))
            c = np.sort(rng.choice(inner, size=k, replace=False))
        cuts.append(np.ascontiguousarray(c, dtype=np.float32))
    return cuts


class _Builder:
    """Collects nodes in creation order (NOT canonical)."""

    def __init__(self):
        self.rows = []

    def node(self):
        self.rows.append([-1, 0, -1, -1, 0.0, 0.0])
        return len(self.rows) - 1

    def tree(self):
        a = np.array(self.rows, dtype=np.float64)
        return canonicalize_tree(Tree(
            a[:, 0].astype(np.int32), a[:, 1].astype(np.int32),
            np.zeros(len(a), dtype=np.float32), a[:, 2].astype(np.int32),
            a[:, 3].astype(np.int32), a[:, 4].copy(), a[:, 5].copy()))


def _leaf_counts(rng):
    c0, c1 = (float(v) for v in rng.randint(0, 50, size=2))
    if rng.rand() < 0.25:
        c0 = c1 = max(c0, 1.0)               # an argmax tie, proba 0.5
    if c0 + c1 == 0:
        c1 = 3.0
    return c0, c1


def _random_tree(n_cut, rng, max_depth):
    b = _Builder()

    def grow(depth):
        i = b.node()
        if depth == max_depth or (depth > 0 and rng.rand() < 0.25):
            b.rows[i][4:6] = _leaf_counts(rng)
            return i
        f = int(rng.randint(len(n_cut))) if depth else MANY_CUTS
        b.rows[i][0] = f
        b.rows[i][1] = int(rng.randint(0, n_cut[f] + 1)) if depth else 127
        b.rows[i][3] = grow(depth + 1)       # right subtree first
        b.rows[i][2] = grow(depth + 1)
        b.rows[i][4:6] = (1.0, 1.0)
        return i

    grow(0)
    return b.tree()


def _root_leaf_tree(rng):
    b = _Builder()
    b.rows[b.node()][4:6] = _leaf_counts(rng)
    return b.tree()


def _chain_tree(n_cut, rng):
    """Degenerate chain on the 255-cut feature: level d sends
    code <= 10 d to a leaf and everything else one level down."""
    b = _Builder()
    node = b.node()
    for d in range(CHAIN_DEPTH):
        leaf, nxt = b.node(), b.node()
        b.rows[leaf][4:6] = _leaf_counts(rng)
        b.rows[node][:4] = [MANY_CUTS, 10 * d, leaf, nxt]
        b.rows[node][4:6] = (1.0, 1.0)
        node = nxt
    b.rows[node][4:6] = _leaf_counts(rng)
    return b.tree()


def _hand_built(F, spec, n_trees, g, seed):
    """Group g's detector: tree kinds rotate with t + g, so with one tree
    per forest the groups still hold a random tree, a single leaf and a
    chain, and forests of different groups differ in node count."""
    from flake16_framework_amd.engine.detector import assemble_detector
    rng = np.random.RandomState(seed)
    params = _params(F, spec, rng)
    X = _pool(F, params, rng)
    T32 = transform_preprocessing(X, params).astype(np.float32)
    cuts = _cuts_from(T32, rng)
    n_cut = [len(c) for c in cuts]
    trees = []
    for t in range(n_trees):
        kind = (t + g) % 3
        if kind == 0:
            trees.append(_random_tree(n_cut, rng, max_depth=4 + g))
        elif kind == 1:
            trees.append(_root_leaf_tree(rng))
        else:
            trees.append(_chain_tree(n_cut, rng))
    cols = tuple(range(16)) if F == 16 else FLAKEFLAGGER_COLUMNS
    det = assemble_detector(
        ("NOD", "Flake16" if F == 16 else "FlakeFlagger", "None", "None",
         "Random Forest"), 2, cols, params, cuts, trees, n_trees, 0, M_POOL)
    return det, X


def _masks(F):
    """A single low column (the 255-cut one every chain and root reads),
    column F - 1 (with F = 16 the top byte of the high code word), all F
    columns, and a mixed mask across both code words."""
    mixed = 1 << ONE_CUT | 1 << CONST_COL | 1 << (F // 2) | 1 << (F - 2)
    return np.array([1 << MANY_CUTS, 1 << (F - 1), (1 << F) - 1, mixed],
                    dtype=np.int32)


def _triples(pred, y, seg_off):
    out = np.zeros((G + 1, 3), dtype=np.int32)
    for g, (a, b) in enumerate(
            [*zip(seg_off[:-1], seg_off[1:]), (0, len(y))]):
        p, t = pred[a:b], y[a:b]
        out[g] = [(p & ~t).sum(), (~p & t).sum(), (p & t).sum()]
    return out


def _acc_numpy(dets, det_of_group, X, seg_off):
    acc = np.zeros((len(X), 2))
    for g, d in enumerate(det_of_group):
        s = slice(seg_off[g], seg_off[g + 1])
        if seg_off[g + 1] > seg_off[g]:
            det = dets[d]
            T = transform_preprocessing(X[s], det.preprocessing_params())
            codes = bin_codes(T.astype(np.float32), det.cut_list())
            acc[s, 0], acc[s, 1] = accumulate_proba(det.trees(), codes)
    return acc


def _permuted(X, perm_r, mask):
    cols = [f for f in range(X.shape[1]) if mask >> f & 1]
    Xp = X.copy()
    Xp[:, cols] = X[perm_r][:, cols]
    return Xp


def _fused(ops, d, labels_dev, det_of_group, perm, masks, threshold):
    from flake16_framework_amd.engine.importance import permuted_counts
    counts, baseline = permuted_counts(
        ops, d, labels_dev, torch.tensor(det_of_group, dtype=torch.int32),
        torch.from_numpy(perm), torch.from_numpy(masks), threshold)
    assert counts.dtype == baseline.dtype == torch.int32
    assert counts.shape == (len(masks), len(perm), G + 1, 3)
    assert baseline.shape == (G + 1, 3)
    return counts.cpu().numpy(), baseline.cpu().numpy()


def _existing_ops(ops, d, X64, labels_dev, threshold):
    """[FP, FN, TP] under (threshold, argmax) from holdout_encode +
    holdout_proba + threshold_counts with K = 1 on the matrix X64."""
    codes = ops.holdout_encode(X64, d["seg_off"], d["mean"], d["scale"],
                               d["pca_mean"], d["W"], d["has_pca"],
                               d["cuts"], d["cut_off"], d["F"])
    acc = ops.holdout_proba(codes, d["seg_off"], d["tree_off"], d["nodes"],
                            d["n_trees"])
    curve, argmax = ops.threshold_counts(
        acc, labels_dev, d["seg_off"], d["n_trees"],
        torch.tensor([threshold], dtype=torch.float64))
    return curve[:, 0].cpu().numpy(), argmax.cpu().numpy()


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("n_trees", [1, 10, 11, 23])
@pytest.mark.parametrize("spec", [None, "scale", "scale+pca"])
@pytest.mark.parametrize("F", [16, 7])
def test_permuted_counts_on_hand_built(F, spec, n_trees, R):
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.engine.importance import make_permutations
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    seed = 1000 * F + 10 * n_trees
    built = [_hand_built(F, spec, n_trees, g, seed=seed + g)
             for g in range(G)]
    dets = [b[0] for b in built]
    kinds = [np.diff(d.tree_off) for d in dets]
    assert any((k == 1).any() for k in kinds)                  # single leaf
    assert any((k == 2 * CHAIN_DEPTH + 1).any() for k in kinds)     # chain
    masks = _masks(F)
    assert len(set(masks.tolist())) == 4 and (masks >> F == 0).all()
    rng = np.random.RandomState(seed + 7)
    tied = exact = moved = 0

    for sizes in GROUP_ORDERS:
        seg_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
        X = np.concatenate([b[1][:m] for b, m in zip(built, sizes)])
        y = rng.rand(len(X)) < 0.4
        labels_dev = torch.from_numpy(y.astype(np.uint8)).cuda()
        perm = make_permutations(seg_off, R, seed)
        d = grouped_inputs(dets, X, seg_off)

        for det_of_group in (list(range(G)), [0] * G):
            # numpy reference: sums once per job, both rules from them
            base_acc = _acc_numpy(dets, det_of_group, X, seg_off)
            # a threshold that probabilities of the reference hit exactly
            threshold = float(np.median(base_acc[:, 1] / n_trees))
            rules = {
                None: lambda a: a[:, 1] > a[:, 0],
                threshold: lambda a: a[:, 1] / n_trees >= threshold,
            }
            exact += int((base_acc[:, 1] / n_trees == threshold).sum())
            tied += int((base_acc[:, 0] == base_acc[:, 1]).sum())
            want_base = {t: _triples(rule(base_acc), y, seg_off)
                         for t, rule in rules.items()}
            want = {t: np.zeros((4, R, G + 1, 3), dtype=np.int32)
                    for t in rules}
            for j, mask in enumerate(masks):
                for r in range(R):
                    acc = _acc_numpy(dets, det_of_group,
                                     _permuted(X, perm[r], int(mask)),
                                     seg_off)
                    moved += int((acc != base_acc).any())
                    for t, rule in rules.items():
                        want[t][j, r] = _triples(rule(acc), y, seg_off)

            got = {}
            for t in rules:
                counts, baseline = _fused(ops, d, labels_dev, det_of_group,
                                          perm, masks, t)
                np.testing.assert_array_equal(baseline, want_base[t])
                np.testing.assert_array_equal(counts, want[t])
                # one mask alone: J * R is 1 or 3
                counts1, baseline1 = _fused(ops, d, labels_dev,
                                            det_of_group, perm, masks[3:],
                                            t)
                np.testing.assert_array_equal(baseline1, want_base[t])
                np.testing.assert_array_equal(counts1, want[t][3:])
                got[t] = counts, baseline

            # second oracle: the existing ops on a gathered matrix
            d_map = grouped_inputs([dets[m] for m in det_of_group], X,
                                   seg_off)
            thr, arg = _existing_ops(ops, d_map, d["X64"], labels_dev,
                                     threshold)
            np.testing.assert_array_equal(got[threshold][1], thr)
            np.testing.assert_array_equal(got[None][1], arg)
            for j, mask in enumerate(masks):
                cols = [f for f in range(F) if int(mask) >> f & 1]
                for r in range(R):
                    src = torch.from_numpy(perm[r]).long().cuda()
                    Xp = d["X64"].clone()
                    Xp[:, cols] = d["X64"][src][:, cols]
                    thr, arg = _existing_ops(ops, d_map, Xp, labels_dev,
                                             threshold)
                    np.testing.assert_array_equal(got[threshold][0][j, r],
                                                  thr)
                    np.testing.assert_array_equal(got[None][0][j, r], arg)

    assert exact > 0 and moved > 0
    if n_trees == 1:
        assert tied > 0                  # argmax ties decided as 0


def test_identity_permutation_gives_the_baseline():
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    for F, spec in ((16, None), (7, "scale+pca")):
        built = [_hand_built(F, spec, 11, g, seed=50 + g) for g in range(G)]
        sizes = GROUP_ORDERS[1]
        seg_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
        X = np.concatenate([b[1][:m] for b, m in zip(built, sizes)])
        y = np.random.RandomState(F).rand(len(X)) < 0.5
        d = grouped_inputs([b[0] for b in built], X, seg_off)
        perm = np.tile(np.arange(len(X), dtype=np.int32), (2, 1))
        counts, baseline = _fused(
            ops, d, torch.from_numpy(y.astype(np.uint8)).cuda(),
            list(range(G)), perm, _masks(F), None)
        assert baseline[G].sum() > 0
        np.testing.assert_array_equal(baseline[:G].sum(axis=0), baseline[G])
        for j in range(4):
            for r in range(2):
                np.testing.assert_array_equal(counts[j, r], baseline)


# -- end to end -------------------------------------------------------------
@pytest.fixture(scope="module")
def tests600():
    return make_synthetic_tests(n_tests=600, seed=0)


@pytest.mark.parametrize("keys", [
    SHAP_CONFIGS[0],
    ("NOD", "FlakeFlagger", "PCA", "SMOTE ENN", "Random Forest"),
], ids=["nod", "pca-flakeflagger"])
def test_importance_equal_across_backends(keys, tests600):
    from flake16_framework_amd.engine.detector import fit_detector
    from flake16_framework_amd.engine.importance import importance
    det = fit_detector(keys, tests=tests600, seed=0, backend="ref",
                       n_trees=12)
    # scored on the file it was fitted on: a synthetic file of another
    # seed has other class profiles, and nothing on it is predicted flaky
    for threshold in (None, 0.25):
        kw = dict(tests=tests600, repeats=2, seed=5, threshold=threshold)
        want = importance(det, backend="ref", **kw)
        got = importance(det, backend="hip", **kw)
        assert got == want
        assert len(want["importance"]) == len(det.feature_cols) + 3
        assert want["baseline"]["total"][2] > 0
        assert any(e["counts"] != [want["baseline"]["total"][:3]] * 2
                   for e in want["importance"].values())


def test_holdout_importance_equal_across_backends():
    from flake16_framework_amd.engine.importance import holdout_importance
    tests5 = make_synthetic_tests(n_tests=300, n_projects=5, seed=2)
    kw = dict(tests=tests5, n_trees=5, seed=0, repeats=2)
    want = holdout_importance(SHAP_CONFIGS[0], backend="ref", **kw)
    got = holdout_importance(SHAP_CONFIGS[0], backend="hip", **kw)
    assert got == want
    assert len(want["importance"]) == 19


# -- host checks ------------------------------------------------------------
def test_op_refuses_bad_arguments():
    """Every refusal is a host check: nothing is launched."""
    from flake16_framework_amd.engine.holdout import grouped_inputs
    from flake16_framework_amd.engine.importance import permuted_counts
    from flake16_framework_amd.ops.backend import get_ops
    ops = get_ops()
    F = 7
    built = [_hand_built(F, "scale", 2, g, seed=g) for g in range(2)]
    X = np.concatenate([b[1][:5] for b in built])
    d = grouped_inputs([b[0] for b in built], X, [0, 5, 10])
    labels_dev = torch.zeros(10, dtype=torch.uint8).cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    good = dict(det_of_group=i32([0, 1]),
                perm=i32([[4, 3, 2, 1, 0, 9, 8, 7, 6, 5]]),
                masks=i32([1, 1 << (F - 1)]))

    def run(inputs=d, **kw):
        a = dict(good, **kw)
        return permuted_counts(ops, inputs, labels_dev, a["det_of_group"],
                               a["perm"], a["masks"], None)

    counts, baseline = run()
    assert counts.shape == (2, 1, 3, 3) and baseline.shape == (3, 3)
    for masks in ([0], [1, 0], [1 << F], [-1]):
        with pytest.raises(RuntimeError):
            run(masks=i32(masks))
    for perm in ([[5, 3, 2, 1, 0, 9, 8, 7, 6, 5]],     # first row leaves
                 [[4, 3, 2, 1, 0, 9, 8, 7, 6, 4]],     # last row leaves
                 [[4, 3, 2, 1, 0, 9, 8, 7, 6, 10]],    # past the end
                 [[4, 3, 2, 1, -1, 9, 8, 7, 6, 5]],
                 [[4, 3, 2, 1, 0, 9, 8, 7, 6]]):       # one entry short
        with pytest.raises(RuntimeError):
            run(perm=i32(perm))
    with pytest.raises(RuntimeError):      # perm on the device: unchecked
        run(perm=good["perm"].cuda())
    for det_of_group in ([0], [0, 1, 0], [0, 2], [-1, 0]):
        with pytest.raises(RuntimeError):
            run(det_of_group=i32(det_of_group))
    for seg in ([0, 5, 9], [0, 5, 11], [1, 5, 10], [0, 7, 5, 10]):
        with pytest.raises(RuntimeError):
            run(inputs=dict(d, seg_off=i32(seg)))
    bad = d["cut_off"].clone()
    bad[1, 16] += 1                        # past the end of the cut array
    with pytest.raises(RuntimeError):
        run(inputs=dict(d, cut_off=bad))
    with pytest.raises(RuntimeError):      # one root id short
        run(inputs=dict(d, tree_off=d["tree_off"][:-1]))
