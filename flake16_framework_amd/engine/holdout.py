"""holdout: leave-one-project-out evaluation with threshold curves.

The scores stage's pooled 10-fold CV fits preprocessing on the whole
dataset and lets tests of one project sit on both sides of every split.
This stage answers what a user of `fit` needs to know instead: how good is
the detector on a project it has never seen?

Definition.  For the projects p_0 .. p_{G-1} of a tests.json in file
order, fold g IS fit_detector(keys, tests = every project but p_g, seed,
n_trees), applied with detect to {p_g: tests[p_g]}.  Preprocessing
parameters and bin cuts therefore come from the training projects only,
and the Philox keys are fit's own (DETECT_BAL_KEY, DETECT_JOB_BASE + t).
`backend="ref"` is literally that loop.  `backend="hip"` computes the same
arrays with one fused forest_fit over all folds and three grouped launches
(ops/hip/holdout.hip) over all held-out rows.

Two prediction rules are counted, per project and pooled, as [FP, FN, TP]
(true negatives skipped, as in engine/metrics):
  argmax       pred = acc1 > acc0, the rule of detect and scores (ties 0);
  threshold k  pred = proba >= t_k with proba = acc1 / n_trees in fp64 and
               t_k = k / (K - 1), k = 0 .. K-1.
Every output is an integer or an fp64 value from a pinned operation order,
so the two backends agree exactly.
"""

import json
import os

import numpy as np

from ..configgrid import MODEL_AXIS, resolve
from ..constants import HOLDOUT_FILE
from ..dataset.tests_io import load_feat_lab_proj, load_tests
from ..models.forest_ref import Tree, canonicalize_tree
from ..preprocess import fit_preprocessing, transform_preprocessing
from .detector import (
    DETECT_BAL_KEY, DETECT_JOB_BASE, FPAD, _resolve_backend,
    assemble_detector, detect, encode_inputs, fit_detector, pack_nodes,
)
from .metrics import get_prf

MAX_THRESHOLDS = 256


def make_thresholds(n_thresholds):
    """t_k = k / (K - 1) as float64 [K]; a single threshold is 0."""
    K = int(n_thresholds)
    if not 1 <= K <= MAX_THRESHOLDS:
        raise ValueError(f"n_thresholds must be in 1..{MAX_THRESHOLDS}")
    return np.arange(K, dtype=np.float64) / max(K - 1, 1)


def counts_ref(proba, pred, labels, seg_off, thresholds):
    """numpy counts: (curve int32 [G + 1, K, 3], argmax int32 [G + 1, 3]),
    columns FP, FN, TP, row G pooled over all rows."""
    proba = np.asarray(proba, dtype=np.float64)
    pred = np.asarray(pred).astype(bool)
    y = np.asarray(labels).astype(bool)
    G, K = len(seg_off) - 1, len(thresholds)
    curve = np.zeros((G + 1, K, 3), dtype=np.int32)
    argmax = np.zeros((G + 1, 3), dtype=np.int32)

    def triple(p, t):
        return [int((p & ~t).sum()), int((~p & t).sum()), int((p & t).sum())]

    bounds = [(seg_off[g], seg_off[g + 1]) for g in range(G)]
    for g, (a, b) in enumerate(bounds + [(0, len(y))]):
        argmax[g] = triple(pred[a:b], y[a:b])
        for k, t in enumerate(thresholds):
            curve[g, k] = triple(proba[a:b] >= t, y[a:b])
    return curve, argmax


def curve_prf(curve):
    """[[FP, FN, TP]] * K -> [[P, R, F]] * K (None on zero denominators)."""
    return [list(get_prf(*(int(v) for v in row))) for row in curve]


def best_f1_threshold(curve, thresholds):
    """(k, t_k, F1) of the threshold with the largest F1; the lowest
    threshold wins ties.  None when no threshold has an F1.

    Descriptive only: the threshold is chosen on the held-out data it is
    scored on, so its F1 is an upper bound, not an estimate of what a
    threshold fixed in advance would reach."""
    best = None
    for k, (_, _, f) in enumerate(curve_prf(curve)):
        if f is not None and (best is None or f > best[2]):
            best = (k, float(thresholds[k]), f)
    return best


def _project_rows(tests):
    names = list(tests)
    seg_off = np.zeros(len(names) + 1, dtype=np.int32)
    seg_off[1:] = np.cumsum([len(tests[p]) for p in names])
    return names, seg_off


def _oof_ref(keys, tests, names, seed, n_trees):
    detectors, parts = [], []
    for held in names:
        train = {p: rows for p, rows in tests.items() if p != held}
        det = fit_detector(keys, tests=train, seed=seed, backend="ref",
                           n_trees=n_trees)
        parts.append(detect(det, tests={held: tests[held]}, backend="ref"))
        detectors.append(det)
    oof = {name: np.concatenate([p[name] for p in parts])
           for name in ("proba", "pred", "projects", "nodeids")}
    return detectors, oof


def _fold_chunks(fold_samples, n_trees):
    """Consecutive runs of folds whose job-sample total (rows x trees)
    stays within FLAKE16_FUSE_MAX_S, the gate of hip_cell.evaluate_group;
    a fold above the gate goes alone."""
    fuse_max = int(os.environ.get("FLAKE16_FUSE_MAX_S", str(1 << 26)))
    chunks, total = [[]], 0
    for g, n in enumerate(fold_samples):
        s = int(n) * n_trees
        if chunks[-1] and total + s > fuse_max:
            chunks.append([])
            total = 0
        chunks[-1].append(g)
        total += s
    return chunks


def _fit_folds_hip(tests, flaky_label, feature_set, preproc, balancing,
                   model, n_trees, seed, timer=None):
    """Per fold: host preprocessing fit, device cuts and balancing (the
    steps of detector._fit_trees_hip); then every fold's trees from one
    forest_fit per chunk of folds.  Returns per fold (params, cuts, trees)
    with the trees still in the device allocator's numbering."""
    import torch

    from ..ops.backend import get_ops
    from .hip_cell import SweepContext, _device_cuts, _pad16

    tick = timer or (lambda name: None)
    ops = get_ops()
    ctx = SweepContext(tests={}, seed=seed)
    device = ctx.device
    F = len(feature_set)

    # The training matrix is loaded the way fit_detector loads it, not
    # sliced out of the full one: numpy's column reductions add in an
    # order that follows the memory layout, and the fitted means must
    # match fit_detector's to the last bit.
    params, X32s = [], []
    for held in tests:
        train = {p: rows for p, rows in tests.items() if p != held}
        feats, labels_b, _ = load_feat_lab_proj(flaky_label, feature_set,
                                                tests=train)
        p = fit_preprocessing(feats, preproc)
        params.append(p)
        X32s.append((transform_preprocessing(feats, p).astype(np.float32),
                     labels_b.astype(np.uint8)))
    tick("host_preprocessing")

    cuts, fold_codes, fold_labels = [], [], []
    for X, y in X32s:
        X32 = _pad16(torch.from_numpy(np.ascontiguousarray(X)).to(device))
        cuts_dev, cut_off_dev = _device_cuts(X32[:, :F], F)
        Xb, yb = ctx._balance_dev(X32, y, balancing, DETECT_BAL_KEY)
        fold_codes.append(ops.bin_codes(Xb, cuts_dev, cut_off_dev, F))
        fold_labels.append(torch.from_numpy(yb).to(device))
        flat, off = cuts_dev.cpu().numpy(), cut_off_dev.cpu().numpy()
        cuts.append([flat[off[f]:off[f + 1]] for f in range(F)])
    tick("cuts_balancing")

    max_features = F if model["kind"] == "decision_tree" else max(
        1, int(np.sqrt(F)))
    n_rows = [int(y.shape[0]) for y in fold_labels]
    trees = []
    for chunk in _fold_chunks(n_rows, n_trees):
        n = np.array([n_rows[g] for g in chunk], dtype=np.int64)
        base = np.concatenate(([0], np.cumsum(n)[:-1]))
        i32 = lambda a: torch.from_numpy(a.astype(np.int32))
        nfeat, nsplit, nleft, ncnt0, ncnt1, j_node_off, node_alloc = \
            ops.forest_fit(
                torch.cat([fold_codes[g] for g in chunk]).contiguous(),
                torch.cat([fold_labels[g] for g in chunk]).contiguous(),
                i32(np.repeat(base, n_trees)).to(device),
                i32(np.repeat(n, n_trees)),
                i32(DETECT_JOB_BASE
                    + np.tile(np.arange(n_trees), len(chunk))).to(device),
                F, max_features, model["bootstrap"],
                model["kind"] == "extra_trees", seed)
        nfeat, nsplit, nleft = (a.cpu().numpy()
                                for a in (nfeat, nsplit, nleft))
        ncnt0, ncnt1 = ncnt0.cpu().numpy(), ncnt1.cpu().numpy()
        start = j_node_off.cpu().numpy()
        count = node_alloc.cpu().numpy()
        for i in range(len(chunk)):
            fold_trees = []
            for j in range(i * n_trees, (i + 1) * n_trees):
                s = slice(int(start[j]), int(start[j]) + int(count[j]))
                left = nleft[s]      # meaningful at internal nodes only
                fold_trees.append(Tree(
                    nfeat[s], nsplit[s],
                    np.zeros(count[j], dtype=np.float32), left, left + 1,
                    ncnt0[s].astype(np.float64),
                    ncnt1[s].astype(np.float64)))
            trees.append(fold_trees)
    tick("forest_fit")
    return list(zip(params, cuts, trees))


def grouped_inputs(detectors, X, seg_off, device=None):
    """Tensors for grouped_acc: detector g serves rows
    seg_off[g]:seg_off[g+1] of X.  The raw rows and the concatenated packed
    forest go to the device; parameters, cuts and offsets stay on the host,
    where the ops validate them."""
    import torch

    device = device or torch.device("cuda")
    first = detectors[0]
    F, n_trees = first.n_features, first.n_trees
    for d in detectors:
        if (d.n_features, d.n_trees, d.preproc) != (F, n_trees,
                                                    first.preproc):
            raise ValueError("grouped evaluation needs one configuration")
    X64 = np.zeros((X.shape[0], FPAD), dtype=np.float64)
    X64[:, :F] = X
    enc = [encode_inputs(d) for d in detectors]
    stack = lambda i: torch.from_numpy(np.stack([e[i] for e in enc]))

    node_base = np.concatenate(
        ([0], np.cumsum([len(d.feat) for d in detectors]))).astype(np.int64)
    nodes, roots = [], []
    for d, b in zip(detectors, node_base):
        packed = pack_nodes(d).copy()
        packed[d.feat >= 0, 0] += np.int32(b)    # child ids become global
        nodes.append(packed)
        roots.append(d.tree_off[:-1] + b)
    roots.append(node_base[-1:])
    return {
        "X64": torch.from_numpy(X64).to(device),
        "seg_off": torch.from_numpy(np.ascontiguousarray(seg_off,
                                                         dtype=np.int32)),
        "mean": stack(0), "scale": stack(1), "pca_mean": stack(2),
        "W": stack(3), "has_pca": first.preproc == "scale+pca",
        "cuts": torch.from_numpy(np.concatenate(
            [d.cuts for d in detectors]).astype(np.float32)),
        "cut_off": torch.from_numpy(np.stack(
            [d.cut_off for d in detectors]).astype(np.int32)),
        "F": F,
        "tree_off": torch.from_numpy(
            np.concatenate(roots).astype(np.int64)).to(device),
        "nodes": torch.from_numpy(np.concatenate(nodes)).to(device),
        "n_trees": n_trees,
    }


def grouped_acc(ops, d):
    """Encode and (acc0, acc1) float64 [M, 2] for all groups: 2 launches."""
    codes = ops.holdout_encode(d["X64"], d["seg_off"], d["mean"], d["scale"],
                               d["pca_mean"], d["W"], d["has_pca"],
                               d["cuts"], d["cut_off"], d["F"])
    return ops.holdout_proba(codes, d["seg_off"], d["tree_off"], d["nodes"],
                             d["n_trees"])


def grouped_eval(ops, d, labels_dev, thresholds):
    """The evaluation hot path: three launches whatever the group count.
    Returns device tensors (acc, curve, argmax)."""
    acc = grouped_acc(ops, d)
    curve, argmax = ops.threshold_counts(acc, labels_dev, d["seg_off"],
                                         d["n_trees"], thresholds)
    return acc, curve, argmax


def holdout(keys, tests=None, tests_file=None, seed=0, backend="auto",
            n_trees=None, n_thresholds=101, keep_detectors=False,
            timer=None):
    """Leave-one-project-out evaluation of configuration `keys`.

    Returns {"config_keys", "seed", "n_trees", "thresholds" float64 [K],
    "projects": {proj: {"n_train", "n_test", "n_flaky", "argmax": [FP, FN,
    TP, P, R, F], "curve": [[FP, FN, TP]] * K}}, "total": the same fields
    pooled over all held-out rows, "oof": the out-of-fold {"proba", "pred",
    "projects", "nodeids"} arrays in file order, as detect returns them},
    plus "detectors": the G fold Detectors when keep_detectors is set.

    timer, when given, is called with a phase name as each phase of the
    device backend ends (scripts/time_holdout.py)."""
    backend = _resolve_backend(backend)
    keys = tuple(keys)
    flaky_label, feature_set, preproc, balancing, _ = resolve(keys)
    model = MODEL_AXIS[keys[4]]
    n_trees = int(model["n_estimators"] if n_trees is None else n_trees)
    if n_trees < 1:
        raise ValueError("n_trees must be >= 1")
    thresholds = make_thresholds(n_thresholds)
    if tests is None:
        tests = load_tests(tests_file)
    if len(tests) < 2:
        raise ValueError("holdout needs at least two projects")
    names, seg_off = _project_rows(tests)
    features, labels_b, projects = load_feat_lab_proj(
        flaky_label, feature_set, tests=tests)
    labels = labels_b.astype(np.uint8)
    N = len(labels)

    if backend == "ref":
        detectors, oof = _oof_ref(keys, tests, names, seed, n_trees)
        curve, argmax = counts_ref(oof["proba"], oof["pred"], labels,
                                   seg_off, thresholds)
    else:
        import torch

        from ..ops.backend import get_ops

        if not np.isfinite(features).all():
            raise ValueError("detect: non-finite feature value")
        folds = _fit_folds_hip(tests, flaky_label, feature_set, preproc,
                               balancing, model, n_trees, seed, timer)
        detectors = [
            assemble_detector(
                keys, flaky_label, feature_set, params, cuts,
                [canonicalize_tree(t) for t in trees], n_trees, seed,
                N - int(seg_off[g + 1] - seg_off[g]))
            for g, (params, cuts, trees) in enumerate(folds)]
        if timer:
            timer("assemble")
        d = grouped_inputs(detectors, features, seg_off)
        acc, curve, argmax = grouped_eval(
            get_ops(), d, torch.from_numpy(labels).to(d["X64"].device),
            torch.from_numpy(thresholds))
        acc = acc.cpu().numpy()
        curve, argmax = curve.cpu().numpy(), argmax.cpu().numpy()
        oof = {"proba": acc[:, 1] / n_trees,
               "pred": (acc[:, 1] > acc[:, 0]).astype(np.uint8),
               "projects": projects.astype(str),
               "nodeids": np.array(
                   [nid for rows in tests.values() for nid in rows],
                   dtype=str)}
        if timer:
            timer("grouped_evaluation")

    def entry(g, n_test, n_flaky):
        fp, fn, tp = (int(v) for v in argmax[g])
        return {"n_train": N - n_test, "n_test": n_test, "n_flaky": n_flaky,
                "argmax": [fp, fn, tp, *get_prf(fp, fn, tp)],
                "curve": [[int(v) for v in row] for row in curve[g]]}

    res = {
        "config_keys": keys, "seed": int(seed), "n_trees": n_trees,
        "thresholds": thresholds,
        "projects": {
            p: entry(g, int(seg_off[g + 1] - seg_off[g]),
                     int(labels[seg_off[g]:seg_off[g + 1]].sum()))
            for g, p in enumerate(names)},
        "total": entry(len(names), N, int(labels.sum())),
        "oof": oof,
    }
    # pooled: every row is held out exactly once, nothing is trained on all
    res["total"]["n_train"] = None
    if keep_detectors:
        res["detectors"] = detectors
    return res


def write_holdout(keys, tests=None, tests_file=None, out_file=HOLDOUT_FILE,
                  detections_file=None, **kwargs):
    """holdout() written as JSON: the result without the per-test arrays
    and detectors, None as null.  With detections_file, the out-of-fold
    {proj: {nodeid: [proba, pred]}} goes there in the detections.json
    format."""
    res = holdout(keys, tests=tests, tests_file=tests_file, **kwargs)
    doc = {k: v for k, v in res.items() if k not in ("oof", "detectors")}
    doc["config_keys"] = list(res["config_keys"])
    doc["thresholds"] = [float(t) for t in res["thresholds"]]
    with open(out_file, "w") as fd:
        json.dump(doc, fd, indent=4)
    if detections_file:
        oof, out = res["oof"], {}
        for proj, nid, p, y in zip(oof["projects"], oof["nodeids"],
                                   oof["proba"], oof["pred"]):
            out.setdefault(str(proj), {})[str(nid)] = [float(p), int(y)]
        with open(detections_file, "w") as fd:
            json.dump(out, fd, indent=4)
    return res
