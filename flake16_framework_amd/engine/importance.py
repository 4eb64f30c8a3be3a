"""importance: permutation feature importance for saved detectors.

`explain` splits one probability into contributions; it does not say
whether detection QUALITY depends on a feature, and it cannot answer for a
whole family of features at once.  This stage does both, and it is defined
through `detect` alone: replace some raw columns of every test by those of
another test of the same project, classify again, count again.

Definition.  For a labelled tests.json with projects p_0 .. p_{G-1} in
file order (project g owning rows seg_off[g]:seg_off[g+1]), column groups
S_0 .. S_{J-1} (non-empty sets of positions into detector.feature_cols),
R repeats and a seed:

  permutation  one per repeat, shared by all groups, acting inside each
               project.  For repeat r and project g with rows a .. b-1:
                 u_i = philox_draw(TAG_PERMUTE, r, g, i; seed,
                                   IMPORTANCE_KEY),  i = 0 .. b-a-1
                 perm_r[a + i] = a + argsort(u, stable)[i]
  job (j, r)   X'[i, c] = X[perm_r[i], c] for c in S_j, else X[i, c], on
               the RAW fp64 rows (before scaling or PCA); then (acc0, acc1)
               is exactly what detect computes on X'
  rule         argmax: acc1 > acc0 (ties 0), or threshold t:
               acc1 / n_trees >= t; one rule per call
  counts       int32 [J, R, G + 1, 3] of [FP, FN, TP], row G pooled, and
               the baseline int32 [G + 1, 3] on the unpermuted X
  importance   drop[j][r] = F1_base - F1[j][r] from engine.metrics.get_prf
               on the pooled integers (None if either side is None), the
               plain Python mean over r (None if any term is None); the
               same for recall.

The same definition holds with one detector per project: the rows of p_g
are then classified by detector g, which with the fold detectors of
`holdout` is the leave-one-project-out form.

Every output is an integer or fp64 arithmetic on integers in a fixed
order, so the two backends agree exactly.  `backend="ref"` is literally
the loop above; `backend="hip"` computes all J * R jobs in one fused
launch (ops/hip/importance.hip).
"""

import json

import numpy as np

from ..constants import FEATURE_NAMES, IMPORTANCE_FILE
from ..dataset.tests_io import load_tests
from ..utils.philox import TAG_PERMUTE, draws_u32
from .detector import Detector, _acc_ref, _resolve_backend, load_rows
from .metrics import get_prf

IMPORTANCE_KEY = 1 << 24      # above DETECT_JOB_BASE's range

FAMILIES = (
    ("Coverage", (0, 1, 2)),
    ("Resource Usage", (3, 4, 5, 6, 7, 8)),
    ("Static", (9, 10, 11, 12, 13, 14, 15)),
)


def default_groups(detector):
    """{name: raw column ids}: one group per input of the detector, named
    by FEATURE_NAMES, then the three collection families restricted to the
    detector's columns.  An empty family is dropped; a family that equals a
    single-feature group is kept."""
    cols = [int(c) for c in detector.feature_cols]
    groups = {FEATURE_NAMES[c]: [c] for c in cols}
    for name, family in FAMILIES:
        used = [c for c in cols if c in family]
        if used:
            groups[name] = used
    return groups


def make_permutations(seg_off, repeats, seed):
    """int32 [R, M]: perm[r, i] is the row whose values row i borrows in
    repeat r, a permutation of every segment (see the module docstring)."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    repeats = int(repeats)
    if repeats < 1:
        raise ValueError("repeats must be >= 1")
    perm = np.empty((repeats, int(seg_off[-1])), dtype=np.int32)
    for r in range(repeats):
        for g in range(len(seg_off) - 1):
            a, b = int(seg_off[g]), int(seg_off[g + 1])
            u = draws_u32(TAG_PERMUTE, r, g, b - a, seed, IMPORTANCE_KEY)
            perm[r, a:b] = a + np.argsort(u, kind="stable")
    return perm


def _group_masks(detector, groups):
    """{name: raw column ids} -> (names, {name: sorted ids}, int32 [J] bit
    masks over positions into detector.feature_cols)."""
    cols = [int(c) for c in detector.feature_cols]
    if not groups:
        raise ValueError("importance needs at least one group")
    named, masks = {}, []
    for name, ids in groups.items():
        ids = sorted({int(c) for c in ids})
        if not ids:
            raise ValueError(f"importance: group {name!r} is empty")
        mask = 0
        for c in ids:
            if c not in cols:
                raise ValueError(
                    f"importance: group {name!r} names column {c}, which "
                    "the detector does not use")
            mask |= 1 << cols.index(c)
        named[str(name)] = ids
        masks.append(mask)
    return list(named), named, np.array(masks, dtype=np.int32)


def _triples(pred, y, seg_off):
    """int32 [G + 1, 3] of [FP, FN, TP], row G pooled."""
    G = len(seg_off) - 1
    out = np.zeros((G + 1, 3), dtype=np.int32)
    bounds = [(seg_off[g], seg_off[g + 1]) for g in range(G)] + [(0, len(y))]
    for g, (a, b) in enumerate(bounds):
        p, t = pred[a:b], y[a:b]
        out[g] = [(p & ~t).sum(), (~p & t).sum(), (p & t).sum()]
    return out


def _predict_ref(detectors, det_of_group, X, seg_off, threshold):
    acc0, acc1 = np.zeros(len(X)), np.zeros(len(X))
    for g, d in enumerate(det_of_group):
        a, b = int(seg_off[g]), int(seg_off[g + 1])
        if b > a:
            acc0[a:b], acc1[a:b] = _acc_ref(detectors[d], X[a:b])
    if threshold is None:
        return acc1 > acc0
    return acc1 / detectors[0].n_trees >= threshold


def _counts_ref(detectors, det_of_group, X, y, seg_off, perm, masks,
                threshold):
    F = X.shape[1]
    G = len(seg_off) - 1
    baseline = _triples(
        _predict_ref(detectors, det_of_group, X, seg_off, threshold), y,
        seg_off)
    counts = np.zeros((len(masks), len(perm), G + 1, 3), dtype=np.int32)
    for j, mask in enumerate(masks):
        cols = [f for f in range(F) if int(mask) >> f & 1]
        for r in range(len(perm)):
            Xp = X.copy()
            Xp[:, cols] = X[perm[r]][:, cols]
            counts[j, r] = _triples(
                _predict_ref(detectors, det_of_group, Xp, seg_off,
                             threshold), y, seg_off)
    return counts, baseline


def _counts_hip(detectors, det_of_group, X, y, seg_off, perm, masks,
                threshold):
    import torch

    from ..ops.backend import get_ops
    from .holdout import grouped_inputs

    d = grouped_inputs(detectors, X, seg_off)
    counts, baseline = permuted_counts(
        get_ops(), d, torch.from_numpy(y.astype(np.uint8)).to(
            d["X64"].device),
        torch.from_numpy(np.asarray(det_of_group, dtype=np.int32)),
        torch.from_numpy(perm), torch.from_numpy(masks), threshold)
    return counts.cpu().numpy(), baseline.cpu().numpy()


def permuted_counts(ops, d, labels_dev, det_of_group, perm, masks,
                    threshold=None):
    """The device hot path on the tensors of holdout.grouped_inputs: every
    job in one fused launch after two launches for the unpermuted rows.
    det_of_group, perm and masks are CPU int32 tensors (the op checks perm
    against seg_off before it uploads it).  Returns device tensors
    (counts [J, R, G + 1, 3], baseline [G + 1, 3])."""
    return ops.permuted_counts(
        d["X64"], labels_dev, d["seg_off"], det_of_group, perm, masks,
        d["mean"], d["scale"], d["pca_mean"], d["W"], d["has_pca"],
        d["cuts"], d["cut_off"], d["F"], d["tree_off"], d["nodes"],
        d["n_trees"], -1.0 if threshold is None else float(threshold))


def _mean_drop(base, values):
    drops = [None if base is None or v is None else base - v for v in values]
    if any(x is None for x in drops):
        return drops, None
    return drops, sum(drops) / len(drops)


def importance(detectors, tests=None, tests_file=None, groups=None,
               repeats=5, seed=0, threshold=None, backend="auto"):
    """Permutation importance of column groups on a labelled tests.json.

    detectors is one Detector, serving every project, or a list of one per
    project in file order, all of one configuration.  groups is {name: raw
    column ids} (default: default_groups); a column the detector does not
    use raises ValueError, as does a non-finite feature value.

    Returns {"config_keys", "seed", "repeats", "rule" ("argmax" or
    "threshold"), "threshold" (None under argmax), "groups": {name: raw
    column ids}, "baseline": {"total": [FP, FN, TP, P, R, F], "projects":
    {proj: the same}}, "importance": {name: {"f1_drop_mean",
    "recall_drop_mean", "f1_drop": [R], "recall_drop": [R], "counts":
    [[FP, FN, TP]] * R pooled, "projects": {proj: [[FP, FN, TP]] * R}}}}."""
    backend = _resolve_backend(backend)
    single = isinstance(detectors, Detector)
    dets = [detectors] if single else list(detectors)
    if not dets:
        raise ValueError("importance needs a detector")
    first = dets[0]
    for det in dets:
        det.validate()
        if (det.config_keys, det.flaky_label, det.n_trees) != (
                first.config_keys, first.flaky_label, first.n_trees) \
                or list(det.feature_cols) != list(first.feature_cols):
            raise ValueError("importance needs one configuration")
    repeats = int(repeats)
    if repeats < 1:
        raise ValueError("repeats must be >= 1")
    if threshold is not None:
        threshold = float(threshold)
        if not 0.0 <= threshold <= 1.0:
            raise ValueError("threshold must be in [0, 1]")
    if tests is None:
        tests = load_tests(tests_file)
    names = list(tests)
    if not single and len(dets) != len(names):
        raise ValueError(
            f"importance: {len(dets)} detectors for {len(names)} projects")
    group_names, named, masks = _group_masks(
        first, default_groups(first) if groups is None else groups)

    seg_off = np.zeros(len(names) + 1, dtype=np.int32)
    seg_off[1:] = np.cumsum([len(tests[p]) for p in names])
    if seg_off[-1] == 0:
        raise ValueError("importance needs at least one test")
    X, _, _ = load_rows(first, tests, None)
    y = np.array([row[1] == first.flaky_label
                  for rows in tests.values() for row in rows.values()],
                 dtype=bool)
    det_of_group = ([0] * len(names) if single
                    else list(range(len(names))))
    perm = make_permutations(seg_off, repeats, seed)

    run = _counts_hip if backend == "hip" else _counts_ref
    counts, baseline = run(dets, det_of_group, X, y, seg_off, perm, masks,
                           threshold)

    G = len(names)
    ints = lambda row: [int(v) for v in row]
    with_prf = lambda row: [*ints(row), *get_prf(*ints(row))]
    base_total = with_prf(baseline[G])
    out = {}
    for j, name in enumerate(group_names):
        prf = [get_prf(*ints(counts[j, r, G])) for r in range(repeats)]
        f1_drop, f1_mean = _mean_drop(base_total[5], [p[2] for p in prf])
        rec_drop, rec_mean = _mean_drop(base_total[4], [p[1] for p in prf])
        out[name] = {
            "f1_drop_mean": f1_mean, "recall_drop_mean": rec_mean,
            "f1_drop": f1_drop, "recall_drop": rec_drop,
            "counts": [ints(counts[j, r, G]) for r in range(repeats)],
            "projects": {p: [ints(counts[j, r, g]) for r in range(repeats)]
                         for g, p in enumerate(names)},
        }
    return {
        "config_keys": tuple(first.config_keys), "seed": int(seed),
        "repeats": repeats,
        "rule": "argmax" if threshold is None else "threshold",
        "threshold": threshold,
        "groups": named,
        "baseline": {"total": base_total,
                     "projects": {p: with_prf(baseline[g])
                                  for g, p in enumerate(names)}},
        "importance": out,
    }


def _write(res, out_file):
    doc = dict(res, config_keys=list(res["config_keys"]))
    with open(out_file, "w") as fd:
        json.dump(doc, fd, indent=4)
    return res


def write_importance(detectors, tests=None, tests_file=None,
                     out_file=IMPORTANCE_FILE, **kwargs):
    """importance() written as JSON, None as null."""
    return _write(importance(detectors, tests=tests, tests_file=tests_file,
                             **kwargs), out_file)


def holdout_importance(keys, tests=None, tests_file=None, n_trees=None,
                       seed=0, groups=None, repeats=5, threshold=None,
                       backend="auto", out_file=None):
    """The leave-one-project-out form: holdout(keys, ...,
    keep_detectors=True) fits one detector per held-out project, and
    importance() then classifies the permuted rows of project g with the
    detector that never saw g.  seed keys both the fits and the
    permutations.

    The groups are RAW features whatever the preprocessing: for a
    scale+pca configuration, whose model inputs (and `explain`'s
    attributions) are the components pc0.., a column is permuted before
    scaling and projection, so the answer is still about the 16 collected
    features.  With out_file the result is written as write_importance
    writes it."""
    from .holdout import holdout

    backend = _resolve_backend(backend)
    if tests is None:
        tests = load_tests(tests_file)
    res = holdout(keys, tests=tests, seed=seed, backend=backend,
                  n_trees=n_trees, keep_detectors=True)
    out = importance(res["detectors"], tests=tests, groups=groups,
                     repeats=repeats, seed=seed, threshold=threshold,
                     backend=backend)
    return _write(out, out_file) if out_file else out
