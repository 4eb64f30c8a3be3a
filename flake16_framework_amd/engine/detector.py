"""fit / detect: one configuration fitted, saved, and applied to new tests.

The scores stage ranks the 216 configurations and the shap stage explains
two of them; this module USES one.  `fit_detector` trains a configuration
on a tests.json and keeps everything needed to classify tests that were
not in it: the preprocessing parameters, the bin cuts and the forest.
`detect` applies a saved detector to another tests.json and returns a
flakiness probability per test.

Contract: given one detector, `detect` returns bit-identical probabilities
on the numpy and the device backend, and for the same training file the
two backends fit array-for-array equal detectors.  That rests on
  - preprocessing fitted on the host in fp64 for BOTH backends, applied
    with a pinned arithmetic order (preprocess.transform_preprocessing;
    the device fit in hip_cell.view_for reduces in another order, so it
    is deliberately not used here);
  - the forest builder's existing bit-parity (models/forest_ref.py);
  - canonical breadth-first node numbering (forest_ref.canonicalize_tree),
    which removes the device allocator's scheduling order;
  - the PREDICT_TREE_BLOCK summation association shared with `scores`.

Philox keys: DETECT_BAL_KEY / DETECT_JOB_BASE sit above the scores and
shap ranges (see engine/shap_stage.py) and fit the device's int32 keys.
"""

import json
from dataclasses import dataclass, fields

import numpy as np

from ..balance import apply_balancing
from ..configgrid import MODEL_AXIS, resolve
from ..constants import DETECTIONS_FILE
from ..dataset.tests_io import load_feat_lab_proj, load_tests
from ..models.binning import bin_codes, compute_bin_cuts
from ..models.forest_ref import (
    LEAF, Tree, accumulate_proba, canonicalize_tree, fit_forest,
    params_for_model,
)
from ..preprocess import fit_preprocessing, transform_preprocessing

FORMAT_VERSION = 1
DETECT_BAL_KEY = 1 << 22
DETECT_JOB_BASE = 1 << 23

FPAD = 16
MAX_CUTS = 255

_SPEC_TO_NAME = {None: "none", "scale": "scale", "scale+pca": "scale+pca"}
_NAME_TO_SPEC = {v: k for k, v in _SPEC_TO_NAME.items()}


@dataclass
class Detector:
    """A fitted configuration.  Every field is a scalar, a tuple of str or
    a numpy array; trees are concatenated in canonical numbering, tree t
    owning nodes tree_off[t]:tree_off[t+1] with tree-local child ids."""
    version: int
    config_keys: tuple        # the five display keys (configgrid axes)
    flaky_label: int
    feature_cols: np.ndarray  # int32[F] columns of the 16-feature row
    preproc: object           # None | "scale" | "scale+pca"
    mean: np.ndarray          # float64[F]   (identity when unused)
    scale: np.ndarray         # float64[F]
    pca_mean: np.ndarray      # float64[F]
    W: np.ndarray             # float64[F, F]
    cuts: np.ndarray          # float32, all features' cuts back to back
    cut_off: np.ndarray       # int32[17]; features >= F own no cuts
    tree_off: np.ndarray      # int64[T + 1]
    feat: np.ndarray          # int32, -1 = leaf
    split: np.ndarray         # int32 split bin (code <= split goes left)
    left: np.ndarray          # int32 left child, right = left + 1; -1 leaf
    cnt0: np.ndarray          # float32 class counts at the node
    cnt1: np.ndarray
    n_trees: int
    seed: int
    n_train: int

    @property
    def n_features(self):
        return len(self.feature_cols)

    def arrays(self):
        """Field name -> numpy array: the artifact's exact content."""
        out = {}
        for fld in fields(self):
            v = getattr(self, fld.name)
            if fld.name == "preproc":
                v = _SPEC_TO_NAME[v]
            out[fld.name] = np.asarray(v)
        return out

    def preprocessing_params(self):
        return {"spec": self.preproc, "mean": self.mean, "scale": self.scale,
                "pca_mean": self.pca_mean, "W": self.W}

    def cut_list(self):
        return [self.cuts[self.cut_off[f]:self.cut_off[f + 1]]
                for f in range(self.n_features)]

    def trees(self):
        """forest_ref.Tree views of the stored trees (counts as fp64)."""
        out = []
        for t in range(self.n_trees):
            s = slice(self.tree_off[t], self.tree_off[t + 1])
            left = self.left[s]
            out.append(Tree(
                self.feat[s], self.split[s],
                np.zeros(len(left), dtype=np.float32), left,
                np.where(left >= 0, left + 1, -1).astype(np.int32),
                self.cnt0[s].astype(np.float64),
                self.cnt1[s].astype(np.float64)))
        return out

    def validate(self):
        """Raise ValueError unless every index a traversal follows is in
        range: the device kernels walk these arrays unchecked."""
        def need(ok, what):
            if not ok:
                raise ValueError(f"detector: {what}")

        F, T = self.n_features, int(self.n_trees)
        need(1 <= F <= FPAD, "feature count out of range")
        need(self.preproc in _SPEC_TO_NAME, "unknown preprocessing spec")
        for name in ("mean", "scale", "pca_mean"):
            need(getattr(self, name).shape == (F,), f"{name} shape")
        need(self.W.shape == (F, F), "W shape")
        off = self.cut_off
        need(off.shape == (FPAD + 1,) and off[0] == 0, "cut offsets")
        n_cut = np.diff(off)
        need((n_cut >= 0).all() and (n_cut <= MAX_CUTS).all()
             and (n_cut[F:] == 0).all() and off[-1] == len(self.cuts),
             "cut offsets")
        toff = self.tree_off
        n_nodes = len(self.feat)
        need(T >= 1 and toff.shape == (T + 1,) and toff[0] == 0
             and toff[-1] == n_nodes and (np.diff(toff) >= 1).all(),
             "tree offsets")
        for name in ("split", "left", "cnt0", "cnt1"):
            need(len(getattr(self, name)) == n_nodes, f"{name} length")
        size = np.repeat(np.diff(toff), np.diff(toff))
        local = np.arange(n_nodes) - np.repeat(toff[:-1], np.diff(toff))
        internal = self.feat != LEAF
        need(((self.feat >= LEAF) & (self.feat < F)).all(), "feature id")
        need(((self.split >= 0) & (self.split <= MAX_CUTS)).all(),
             "split bin")
        # children come after their parent, so every walk terminates
        need(((self.left > local) & (self.left + 1 < size))[internal].all(),
             "child id")
        need((self.left[~internal] == -1).all(), "leaf child id")
        # the packed record tells leaves from internal nodes by cnt0's
        # sign bit, so -0.0 is refused as well
        need((self.cnt0 >= 0).all() and (self.cnt1 >= 0).all()
             and not np.signbit(self.cnt0).any()
             and np.isfinite(self.cnt0 + self.cnt1).all()
             and (self.cnt0 + self.cnt1 > 0)[~internal].all(),
             "class counts")

    def save(self, path):
        with open(path, "wb") as fd:
            np.savez(fd, **self.arrays())

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "version" not in z.files:
                raise ValueError("detector: missing field version")
            version = int(z["version"])
            if version != FORMAT_VERSION:
                raise ValueError(
                    f"detector: unknown format version {version}")
            data = {}
            for fld in fields(cls):
                if fld.name not in z.files:
                    raise ValueError(f"detector: missing field {fld.name}")
                data[fld.name] = z[fld.name]
        name = str(data["preproc"])
        if name not in _NAME_TO_SPEC:
            raise ValueError(f"detector: unknown preprocessing {name}")
        data["preproc"] = _NAME_TO_SPEC[name]
        data["config_keys"] = tuple(str(k) for k in data["config_keys"])
        for name in ("version", "flaky_label", "n_trees", "seed", "n_train"):
            data[name] = int(data[name])
        det = cls(**data)
        det.validate()
        return det


def _resolve_backend(backend):
    if backend == "auto":
        from .scores import _auto_backend
        backend = _auto_backend()
    if backend not in ("hip", "ref"):
        raise ValueError(backend)
    return backend


def assemble_detector(config_keys, flaky_label, feature_set, params, cuts,
                      trees, n_trees, seed, n_train):
    """Canonical trees + fitted parameters + per-feature cut arrays ->
    validated Detector."""
    cut_off = np.zeros(FPAD + 1, dtype=np.int32)
    cut_off[1:] = np.cumsum(
        [len(c) for c in cuts] + [0] * (FPAD - len(cuts)))
    cat = lambda name, dt: np.concatenate(
        [getattr(t, name) for t in trees]).astype(dt)
    det = Detector(
        version=FORMAT_VERSION,
        config_keys=tuple(config_keys),
        flaky_label=int(flaky_label),
        feature_cols=np.array(feature_set, dtype=np.int32),
        preproc=params["spec"],
        mean=np.asarray(params["mean"], dtype=np.float64),
        scale=np.asarray(params["scale"], dtype=np.float64),
        pca_mean=np.asarray(params["pca_mean"], dtype=np.float64),
        W=np.asarray(params["W"], dtype=np.float64),
        cuts=(np.concatenate(cuts) if cuts else np.zeros(0)).astype(
            np.float32),
        cut_off=cut_off,
        tree_off=np.concatenate(
            ([0], np.cumsum([t.n_nodes for t in trees]))).astype(np.int64),
        feat=cat("feature", np.int32),
        split=cat("split_bin", np.int32),
        left=cat("left", np.int32),
        cnt0=cat("count0", np.float32),
        cnt1=cat("count1", np.float32),
        n_trees=int(n_trees), seed=int(seed), n_train=int(n_train))
    det.validate()
    return det


def _fit_trees_ref(X, labels, balancing, model, n_trees, seed):
    cuts = compute_bin_cuts(X)
    Xb, yb = apply_balancing(X, labels, balancing, seed, DETECT_BAL_KEY)
    codes_b = bin_codes(Xb, cuts)
    fparams = params_for_model(model, seed=seed)
    fparams.n_trees = n_trees
    forest = fit_forest(codes_b, yb, fparams, job_base=DETECT_JOB_BASE,
                        cuts=cuts)
    return cuts, forest.trees


def _fit_trees_hip(X, labels, balancing, model, n_trees, seed, tests):
    import torch

    from ..ops.backend import get_ops
    from .hip_cell import SweepContext, _device_cuts, _pad16

    ops = get_ops()
    ctx = SweepContext(tests=tests, seed=seed)
    device = ctx.device
    F = X.shape[1]

    X32 = _pad16(torch.from_numpy(np.ascontiguousarray(X)).to(device))
    cuts_dev, cut_off_dev = _device_cuts(X32[:, :F], F)
    Xb, yb = ctx._balance_dev(X32, labels, balancing, DETECT_BAL_KEY)
    codes_b = ops.bin_codes(Xb, cuts_dev, cut_off_dev, F)

    max_features = F if model["kind"] == "decision_tree" else max(
        1, int(np.sqrt(F)))
    J = n_trees
    j_row_off = torch.zeros(J, dtype=torch.int32, device=device)
    j_n = torch.full((J,), len(yb), dtype=torch.int32, device=device)
    j_key = torch.arange(DETECT_JOB_BASE, DETECT_JOB_BASE + J,
                         dtype=torch.int32, device=device)
    nfeat, nsplit, nleft, ncnt0, ncnt1, j_node_off, node_alloc = \
        ops.forest_fit(codes_b, torch.from_numpy(yb).to(device), j_row_off,
                       j_n, j_key, F, max_features, model["bootstrap"],
                       model["kind"] == "extra_trees", seed)

    flat = cuts_dev.cpu().numpy()
    off = cut_off_dev.cpu().numpy()
    cuts = [flat[off[f]:off[f + 1]] for f in range(F)]

    nfeat, nsplit, nleft = (a.cpu().numpy() for a in (nfeat, nsplit, nleft))
    ncnt0, ncnt1 = ncnt0.cpu().numpy(), ncnt1.cpu().numpy()
    base = j_node_off.cpu().numpy()
    count = node_alloc.cpu().numpy()
    trees = []
    for t in range(J):
        s = slice(int(base[t]), int(base[t]) + int(count[t]))
        left = nleft[s]      # meaningful at internal nodes only
        trees.append(Tree(
            nfeat[s], nsplit[s], np.zeros(count[t], dtype=np.float32),
            left, left + 1, ncnt0[s].astype(np.float64),
            ncnt1[s].astype(np.float64)))
    return cuts, trees


def fit_detector(config_keys, tests=None, tests_file=None, seed=0,
                 backend="auto", n_trees=None):
    """Fit `config_keys` on a whole tests.json and return the Detector.

    n_trees overrides the model axis's n_estimators (tests, quick runs);
    the value used is stored in the artifact."""
    backend = _resolve_backend(backend)
    config_keys = tuple(config_keys)
    flaky_label, feature_set, preproc, balancing, _ = resolve(config_keys)
    model = MODEL_AXIS[config_keys[4]]
    n_trees = int(model["n_estimators"] if n_trees is None else n_trees)
    if n_trees < 1:
        raise ValueError("n_trees must be >= 1")
    if tests is None:
        tests = load_tests(tests_file)

    features, labels_b, _ = load_feat_lab_proj(flaky_label, feature_set,
                                               tests=tests)
    labels = labels_b.astype(np.uint8)
    params = fit_preprocessing(features, preproc)
    X = transform_preprocessing(features, params).astype(np.float32)

    if backend == "hip":
        cuts, trees = _fit_trees_hip(X, labels, balancing, model, n_trees,
                                     seed, tests)
    else:
        cuts, trees = _fit_trees_ref(X, labels, balancing, model, n_trees,
                                     seed)
    trees = [canonicalize_tree(t) for t in trees]
    return assemble_detector(config_keys, flaky_label, feature_set, params,
                             cuts, trees, n_trees, seed, len(labels))


def pack_nodes(detector):
    """int32 [n_nodes, 2] inference records (layout: ops/hip/detector_steps.h).
    Child ids become global so a walk needs only the tree's root id."""
    d = detector
    sizes = np.diff(d.tree_off)
    base = np.repeat(d.tree_off[:-1], sizes)
    internal = d.feat != LEAF
    child = ((d.left + base).astype(np.uint32) | np.uint32(0x80000000))
    word1 = ((d.split.astype(np.uint32) << np.uint32(8))
             | d.feat.astype(np.uint32))
    packed = np.empty((len(d.feat), 2), dtype=np.uint32)
    packed[:, 0] = np.where(internal, child, d.cnt0.view(np.uint32))
    packed[:, 1] = np.where(internal, word1, d.cnt1.view(np.uint32))
    return packed.view(np.int32)


def load_rows(detector, tests, tests_file):
    if tests is None:
        tests = load_tests(tests_file)
    rows, projects, nodeids = [], [], []
    for proj, tests_proj in tests.items():
        for nid, (_, _, *features_nid) in tests_proj.items():
            projects.append(proj)
            nodeids.append(nid)
            rows.append(features_nid)
    X = np.array(rows, dtype=np.float64).reshape(len(rows), -1)
    X = X[:, detector.feature_cols]
    if not np.isfinite(X).all():
        raise ValueError("detect: non-finite feature value")
    return X, np.array(projects, dtype=str), np.array(nodeids, dtype=str)


def _acc_ref(detector, X):
    T = transform_preprocessing(X, detector.preprocessing_params())
    codes = bin_codes(T.astype(np.float32), detector.cut_list())
    return accumulate_proba(detector.trees(), codes)


def encode_inputs(detector):
    """The detector's preprocessing padded to the kernel's 16-wide layout
    (mean 0 / scale 1 / zero loadings in the padding)."""
    F = detector.n_features
    mean, pca_mean = np.zeros(FPAD), np.zeros(FPAD)
    scale = np.ones(FPAD)
    W = np.zeros((FPAD, FPAD))
    mean[:F], scale[:F] = detector.mean, detector.scale
    pca_mean[:F] = detector.pca_mean
    W[:F, :F] = detector.W
    return mean, scale, pca_mean, W


def device_inputs(detector, X, device=None):
    """Tensors for device_acc: the raw rows and the packed forest on the
    device, the few KB of preprocessing parameters and cuts on the host
    (the op validates the cut offsets there)."""
    import torch

    device = device or torch.device("cuda")
    F = detector.n_features
    X64 = np.zeros((X.shape[0], FPAD), dtype=np.float64)
    X64[:, :F] = X
    mean, scale, pca_mean, W = (torch.from_numpy(a)
                                for a in encode_inputs(detector))
    return {
        "X64": torch.from_numpy(X64).to(device),
        "mean": mean, "scale": scale, "pca_mean": pca_mean, "W": W,
        "has_pca": detector.preproc == "scale+pca",
        "cuts": torch.from_numpy(np.ascontiguousarray(detector.cuts)),
        "cut_off": torch.from_numpy(np.ascontiguousarray(detector.cut_off)),
        "F": F,
        "tree_off": torch.from_numpy(detector.tree_off).to(device),
        "nodes": torch.from_numpy(pack_nodes(detector)).to(device),
        "n_trees": detector.n_trees,
    }


def device_acc(ops, d):
    """The device hot path: encode, then (acc0, acc1) as float64 [M, 2]."""
    codes = ops.detect_encode(d["X64"], d["mean"], d["scale"], d["pca_mean"],
                              d["W"], d["has_pca"], d["cuts"], d["cut_off"],
                              d["F"])
    return ops.forest_proba(codes, d["tree_off"], d["nodes"], d["n_trees"])


def _acc_hip(detector, X):
    from ..ops.backend import get_ops

    acc = device_acc(get_ops(), device_inputs(detector, X)).cpu().numpy()
    return acc[:, 0], acc[:, 1]


def detect(detector, tests=None, tests_file=None, backend="auto"):
    """Classify every test of a tests.json (file iteration order).

    Rows use the tests.json layout [req_runs, label, f0..f15]; the first
    two columns are ignored.  Returns {"proba": float64[M] probability of
    the detector's flaky class, "pred": uint8[M] (ties -> 0, as in the
    scores stage), "projects", "nodeids"}."""
    backend = _resolve_backend(backend)
    detector.validate()
    X, projects, nodeids = load_rows(detector, tests, tests_file)
    if len(X) == 0:
        acc0 = acc1 = np.zeros(0)
    elif backend == "hip":
        acc0, acc1 = _acc_hip(detector, X)
    else:
        acc0, acc1 = _acc_ref(detector, X)
    return {"proba": acc1 / detector.n_trees,
            "pred": (acc1 > acc0).astype(np.uint8),
            "projects": projects, "nodeids": nodeids}


def write_detections(detector, tests=None, tests_file=None,
                     out_file=DETECTIONS_FILE, backend="auto"):
    """detect() written as {proj: {nodeid: [proba, pred]}} JSON."""
    res = detect(detector, tests=tests, tests_file=tests_file,
                 backend=backend)
    out = {}
    for proj, nid, p, y in zip(res["projects"], res["nodeids"],
                               res["proba"], res["pred"]):
        out.setdefault(str(proj), {})[str(nid)] = [float(p), int(y)]
    with open(out_file, "w") as fd:
        json.dump(out, fd, indent=4)
    return res
