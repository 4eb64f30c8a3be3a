"""Preprocessing: StandardScaler and PCA (full), reference implementations.

Semantics follow the reference grid (experiment.py:84-85):
  "Scaling" = StandardScaler().fit_transform
  "PCA"     = Pipeline(StandardScaler -> PCA(n_components=None, random_state=0))
and the reference's (leakage-style, deliberately preserved) protocol of
fitting on the FULL dataset before the CV split (experiment.py:452-453).

sklearn parity notes:
  - StandardScaler: population std (ddof=0); zero-variance columns divide
    by 1.0 (sklearn's _handle_zeros_in_scale).
  - PCA on an N x F (F<=16) matrix: full SVD; components are eigenvectors of
    the covariance; sklearn's deterministic svd_flip sign convention is
    applied (sign of the largest-|u| entry per component).  Sign choice
    cannot change tree splits (bins mirror with the sign), so metric parity
    is sign-independent; golden tests compare |values|.

The device path implements the same math as HIP kernels (ops/hip/pca.hip);
those are validated against this module within fp tolerance.
"""

import numpy as np


def scaler_fit_transform(X):
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0)
    var = X.var(axis=0)
    scale = np.sqrt(var)
    scale[scale == 0.0] = 1.0
    return (X - mean) / scale


def pca_fit_transform(X):
    """Full PCA via SVD of the centered matrix (input is pre-scaled)."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    u, s, vt = np.linalg.svd(Xc, full_matrices=False)
    # svd_flip: largest-|u| entry of each component made positive.
    max_rows = np.argmax(np.abs(u), axis=0)
    signs = np.sign(u[max_rows, range(u.shape[1])])
    signs[signs == 0.0] = 1.0
    return (u * s) * signs


def apply_preprocessing(X, spec):
    """spec: None | 'scale' | 'scale+pca' (configgrid.PREPROCESSING_AXIS)."""
    if spec is None:
        return np.asarray(X, dtype=np.float64)
    if spec == "scale":
        return scaler_fit_transform(X)
    if spec == "scale+pca":
        return pca_fit_transform(scaler_fit_transform(X))
    raise ValueError(spec)


# ---------------------------------------------------------------------------
# Saved-parameter preprocessing (fit once, transform any matrix).
#
# The functions above return only the transformed training matrix; a saved
# detector (engine/detector.py) has to apply the SAME transform to tests it
# has never seen, so the fit is kept.  The fit always runs here, on the host
# in fp64, for both backends.  The transform's arithmetic order is pinned so
# the device kernels (ops/hip/detector_steps.h) reproduce it bit for bit.
# ---------------------------------------------------------------------------
def fit_preprocessing(X, spec):
    """Fit `spec` (None | 'scale' | 'scale+pca') on X.

    Returns {"spec", "mean", "scale", "pca_mean", "W"}: float64 arrays of
    F / F / F / F x F entries.  Stages the spec does not use hold the
    identity (mean 0, scale 1, W = I), so every field is always present.
    W[f, k] is the loading of input column f on component k with the
    svd_flip sign (pca_fit_transform's rule) already folded in.
    """
    if spec not in (None, "scale", "scale+pca"):
        raise ValueError(spec)
    X = np.asarray(X, dtype=np.float64)
    F = X.shape[1]
    params = {"spec": spec, "mean": np.zeros(F), "scale": np.ones(F),
              "pca_mean": np.zeros(F), "W": np.eye(F)}
    if spec is None:
        return params

    mean = X.mean(axis=0)
    scale = np.sqrt(X.var(axis=0))
    scale[scale == 0.0] = 1.0
    params["mean"], params["scale"] = mean, scale
    if spec == "scale":
        return params

    Z = (X - mean) / scale
    pca_mean = Z.mean(axis=0)
    u, _, vt = np.linalg.svd(Z - pca_mean, full_matrices=False)
    max_rows = np.argmax(np.abs(u), axis=0)
    signs = np.sign(u[max_rows, range(u.shape[1])])
    signs[signs == 0.0] = 1.0
    W = np.zeros((F, F))
    W[:, :vt.shape[0]] = (vt * signs[:, None]).T
    params["pca_mean"], params["W"] = pca_mean, W
    return params


def transform_preprocessing(X, params):
    """Apply fitted `params` to X (any number of rows) -> float64 matrix.

    Scale is (X - mean) / scale.  The PCA projection
    T[:, k] = sum_f (Z[:, f] - pca_mean[f]) * W[f, k] is accumulated
    sequentially in ascending f from 0.0 with separate multiply and add
    (elementwise column updates, not `@`): BLAS would pick its own
    summation order and fused multiply-adds.
    """
    X = np.asarray(X, dtype=np.float64)
    spec = params["spec"]
    if spec is None:
        return X
    Z = (X - params["mean"]) / params["scale"]
    if spec == "scale":
        return Z
    if spec != "scale+pca":
        raise ValueError(spec)
    pca_mean, W = params["pca_mean"], params["W"]
    T = np.zeros_like(Z)
    for f in range(Z.shape[1]):
        d = Z[:, f] - pca_mean[f]
        for k in range(Z.shape[1]):
            T[:, k] = T[:, k] + d * W[f, k]
    return T
