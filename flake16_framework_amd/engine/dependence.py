"""dependence: partial-dependence and ICE curves for a saved detector.

`importance` names the features detection quality hangs on; this stage
answers the question that follows: how does the flaky probability move as
one feature moves, and does it move the same way in every project?  It is
defined through `detect` alone: set one raw column of every test to a grid
value, classify again, average.

Definition.  For one Detector and a tests.json-shaped file (labels and
req_runs are ignored) with projects p_0 .. p_{G-1} in file order, project
g owning rows seg_off[g]:seg_off[g+1] of the raw fp64 matrix
X = load_rows(...) [M, F], position f of detector.feature_cols being raw
column c:

  grid         computed on the host in numpy, shared by both backends.
               With grid=V (2..64) position f gets
                 s     = np.sort(X[:, f])
                 lo    = (M - 1) * 5 // 100
                 hi    = (M - 1) - lo
                 idx_k = lo + (k * (hi - lo)) // (V - 1),  k = 0 .. V-1
                 grid_f = np.unique(s[idx])
               ascending, and shorter than V when the column has few
               distinct values.  Or grids={raw column id: ascending finite
               values} names 1..64 values for some of the detector's
               columns.
  jobs         the flat list of (f, value) pairs, feature-major; J <= 1024
  job (f, v)   X'[i, f] = v for every row i, on the RAW rows (before
               scaling or PCA); then (acc0, acc1) is exactly what detect
               computes on X'
  rule         argmax: acc1 > acc0 (ties 0), or threshold t:
               acc1 / n_trees >= t; one rule per call
  per job, and for the unmodified rows (the baseline):
  flagged[g]   int32 count of rows predicted flaky, pooled at index G
  S[g]         the fp64 sum of acc1 over project g in this pinned order:
                 1. cut the project's rows into consecutive blocks of 64
                    from seg_off[g]; the last block may be shorter
                 2. within a block put the rows' acc1 into v[0..63], 0.0
                    past the last row, and apply v = v[0::2] + v[1::2] six
                    times; B = v[0]
                 3. S[g] = 0.0 + B_first + B_next + ..., sequentially over
                    the project's blocks in ascending order
                 4. S[G] = 0.0 + S[0] + S[1] + ..., sequentially over the
                    projects in ascending order
  mean_proba   S / float(n_trees * n_rows), computed in Python on the host
               for both backends; None for a project without rows
  ICE          only when requested: acc1 / n_trees per (row, job)

Every output is an integer or fp64 arithmetic in a fixed order, so the two
backends agree bit for bit.  `backend="ref"` is literally the loop above;
`backend="hip"` computes all jobs in one fused launch
(ops/hip/dependence.hip), whose wave reduction is the tree of step 2.
"""

import json

import numpy as np

from ..constants import DEPENDENCE_FILE, FEATURE_NAMES
from ..dataset.tests_io import load_tests
from .detector import _acc_ref, _resolve_backend, load_rows

BLOCK_ROWS = 64
MAX_GRID = 64
MAX_JOBS = 1024


def make_grids(X, grid=20):
    """One ascending float64 grid per column of X (see the module
    docstring): V order statistics between the 5th and the 95th
    percentile position, duplicates dropped."""
    X = np.asarray(X, dtype=np.float64)
    V = int(grid)
    if not 2 <= V <= MAX_GRID:
        raise ValueError(f"grid must be in 2..{MAX_GRID}")
    M = X.shape[0]
    if M < 1:
        raise ValueError("make_grids needs at least one row")
    lo = (M - 1) * 5 // 100
    hi = (M - 1) - lo
    idx = np.array([lo + (k * (hi - lo)) // (V - 1) for k in range(V)])
    return [np.unique(np.sort(X[:, f])[idx]) for f in range(X.shape[1])]


def _explicit_grids(detector, grids):
    """{raw column id: values} -> [(position f, float64 values)] in
    ascending f."""
    cols = [int(c) for c in detector.feature_cols]
    if not grids:
        raise ValueError("dependence: grids names no column")
    out = {}
    for c, values in grids.items():
        c = int(c)
        if c not in cols:
            raise ValueError(f"dependence: grids names column {c}, which "
                             "the detector does not use")
        v = np.asarray(values, dtype=np.float64)
        if v.ndim != 1 or not 1 <= len(v) <= MAX_GRID:
            raise ValueError(f"dependence: column {c} needs 1..{MAX_GRID} "
                             "grid values")
        if not np.isfinite(v).all() or (np.diff(v) <= 0).any():
            raise ValueError(f"dependence: the grid of column {c} must be "
                             "finite and ascending")
        if cols.index(c) in out:
            raise ValueError(f"dependence: column {c} is named twice")
        out[cols.index(c)] = v
    return sorted(out.items())


def block_sums(acc1):
    """Definition steps 1 and 2 for the rows of one project: the pairwise
    sum of every block of 64 consecutive values."""
    n = len(acc1)
    v = np.zeros((-(-n // BLOCK_ROWS), BLOCK_ROWS), dtype=np.float64)
    v.reshape(-1)[:n] = acc1
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def pinned_sums(acc1, seg_off):
    """float64 [G + 1]: definition steps 1 to 4."""
    G = len(seg_off) - 1
    S = np.zeros(G + 1, dtype=np.float64)
    for g in range(G):
        s = 0.0
        for B in block_sums(acc1[int(seg_off[g]):int(seg_off[g + 1])]):
            s = s + float(B)
        S[g] = s
    total = 0.0
    for g in range(G):
        total = total + float(S[g])
    S[G] = total
    return S


def _flag_counts(acc0, acc1, n_trees, seg_off, threshold):
    pred = (acc1 > acc0 if threshold is None
            else acc1 / n_trees >= threshold)
    G = len(seg_off) - 1
    out = np.zeros(G + 1, dtype=np.int32)
    for g in range(G):
        out[g] = pred[int(seg_off[g]):int(seg_off[g + 1])].sum()
    out[G] = pred.sum()
    return out


def _run_ref(detector, X, seg_off, job_col, job_val, threshold, want_ice):
    J, G = len(job_col), len(seg_off) - 1
    S = np.zeros((J + 1, G + 1), dtype=np.float64)
    flagged = np.zeros((J + 1, G + 1), dtype=np.int32)
    ice = np.zeros((J, len(X)), dtype=np.float64) if want_ice else None
    for j in range(J + 1):
        Xp = X
        if j < J:
            Xp = X.copy()
            Xp[:, job_col[j]] = job_val[j]
        acc0, acc1 = _acc_ref(detector, Xp)
        S[j] = pinned_sums(acc1, seg_off)
        flagged[j] = _flag_counts(acc0, acc1, detector.n_trees, seg_off,
                                  threshold)
        if want_ice and j < J:
            ice[j] = acc1
    return S, flagged, ice


def partial_dependence(ops, d, job_col, job_val, threshold=None,
                       want_ice=False):
    """The device hot path on the tensors of holdout.grouped_inputs (one
    detector): every job in one fused launch after two launches for the
    unmodified rows, and one small launch for the sequential sums.
    job_col (int32) and job_val (float64) are CPU tensors.  Returns device
    tensors (S [J + 1, G + 1], flagged [J + 1, G + 1], ice [J, M] of acc1
    or an empty tensor); row J is the baseline."""
    return ops.partial_dependence(
        d["X64"], d["seg_off"], job_col, job_val, d["mean"], d["scale"],
        d["pca_mean"], d["W"], d["has_pca"], d["cuts"], d["cut_off"],
        d["F"], d["tree_off"], d["nodes"], d["n_trees"],
        -1.0 if threshold is None else float(threshold), bool(want_ice))


def _run_hip(detector, X, seg_off, job_col, job_val, threshold, want_ice):
    import torch

    from ..ops.backend import get_ops
    from .holdout import grouped_inputs

    d = grouped_inputs([detector], X, seg_off)
    S, flagged, ice = partial_dependence(
        get_ops(), d, torch.from_numpy(job_col), torch.from_numpy(job_val),
        threshold, want_ice)
    return (S.cpu().numpy(), flagged.cpu().numpy(),
            ice.cpu().numpy() if want_ice else None)


def dependence(detector, tests=None, tests_file=None, grid=20, grids=None,
               threshold=None, ice=False, backend="auto"):
    """Partial-dependence curves of every input of `detector` (or of the
    columns `grids` names) on a tests.json-shaped file.

    Returns {"config_keys", "rule" ("argmax" or "threshold"), "threshold"
    (None under argmax), "n_tests", "baseline": {"mean_proba", "flagged",
    "projects": {proj: [mean_proba, flagged]}}, "features": {FEATURE_NAME:
    {"grid": [...], "mean_proba": [...], "flagged": [...], "range": max -
    min of mean_proba, "projects": {proj: {"mean_proba": [...], "flagged":
    [...]}}}}}; with ice=True also "ice", float64 [M, J] probabilities,
    and "jobs", [[raw column, value], ...]."""
    backend = _resolve_backend(backend)
    detector.validate()
    if threshold is not None:
        threshold = float(threshold)
        if not 0.0 <= threshold <= 1.0:
            raise ValueError("threshold must be in [0, 1]")
    if tests is None:
        tests = load_tests(tests_file)
    names = list(tests)
    seg_off = np.zeros(len(names) + 1, dtype=np.int32)
    seg_off[1:] = np.cumsum([len(tests[p]) for p in names])
    if seg_off[-1] == 0:
        raise ValueError("dependence needs at least one test")
    X, _, _ = load_rows(detector, tests, None)

    if grids is not None:
        per_feature = _explicit_grids(detector, grids)
    else:
        per_feature = list(enumerate(make_grids(X, grid)))
    job_col = np.array([f for f, v in per_feature for _ in v],
                       dtype=np.int32)
    job_val = np.array([x for _, v in per_feature for x in v],
                       dtype=np.float64)
    J = len(job_col)
    if not 1 <= J <= MAX_JOBS:
        raise ValueError(f"dependence: between 1 and {MAX_JOBS} jobs")

    run = _run_hip if backend == "hip" else _run_ref
    S, flagged, acc1 = run(detector, X, seg_off, job_col, job_val,
                           threshold, bool(ice))

    G, n_trees = len(names), detector.n_trees
    n_rows = [int(seg_off[g + 1] - seg_off[g]) for g in range(G)]
    n_rows.append(int(seg_off[G]))

    def mean(j, g):
        if n_rows[g] == 0:
            return None
        return float(S[j, g]) / float(n_trees * n_rows[g])

    cols = [int(c) for c in detector.feature_cols]
    features, j0 = {}, 0
    for f, values in per_feature:
        js = range(j0, j0 + len(values))
        j0 += len(values)
        pooled = [mean(j, G) for j in js]
        features[FEATURE_NAMES[cols[f]]] = {
            "grid": [float(v) for v in values],
            "mean_proba": pooled,
            "flagged": [int(flagged[j, G]) for j in js],
            "range": max(pooled) - min(pooled),
            "projects": {p: {"mean_proba": [mean(j, g) for j in js],
                             "flagged": [int(flagged[j, g]) for j in js]}
                         for g, p in enumerate(names)},
        }
    res = {
        "config_keys": tuple(detector.config_keys),
        "rule": "argmax" if threshold is None else "threshold",
        "threshold": threshold,
        "n_tests": n_rows[G],
        "baseline": {"mean_proba": mean(J, G),
                     "flagged": int(flagged[J, G]),
                     "projects": {p: [mean(J, g), int(flagged[J, g])]
                                  for g, p in enumerate(names)}},
        "features": features,
    }
    if ice:
        res["ice"] = np.ascontiguousarray((acc1 / n_trees).T)
        res["jobs"] = [[cols[f], float(v)]
                       for f, v in zip(job_col, job_val)]
    return res


def write_dependence(detector, tests=None, tests_file=None,
                     out_file=DEPENDENCE_FILE, ice_out=None, **kwargs):
    """dependence() written as JSON, None as null.  With ice_out the ICE
    matrix float64 [M, J] is saved there as .npy; it is not part of the
    JSON file."""
    if ice_out:
        kwargs["ice"] = True
    res = dependence(detector, tests=tests, tests_file=tests_file, **kwargs)
    doc = {k: v for k, v in res.items() if k not in ("ice", "jobs")}
    doc["config_keys"] = list(res["config_keys"])
    with open(out_file, "w") as fd:
        json.dump(doc, fd, indent=4)
    if ice_out:
        with open(ice_out, "wb") as fd:
            np.save(fd, res["ice"])
    return res
