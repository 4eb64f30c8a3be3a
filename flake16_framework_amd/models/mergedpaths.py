"""Merged root->leaf paths of a saved detector, for its TreeSHAP.

Path-dependent TreeSHAP treats a feature that splits several times on one
root->leaf path as ONE path element: the recursion (models/treeshap_ref.py)
unwinds the earlier occurrence and re-extends with the product of the cover
ratios and the conjunction of the branch tests.  A detector has at most 16
model inputs, so after merging every path has at most 16 elements whatever
the tree depth, and the merged element is the same for every row:

  feature   the model input
  lo, hi    the element is hot for a row iff lo < code[feature] <= hi;
            -1 / 255 to begin with, a left edge at split s sets
            hi = min(hi, s), a right edge sets lo = max(lo, s)
  z         product of cover[child] / cover[parent] over the path's edges on
            that feature, multiplied in root->leaf order (fp64,
            cover = (double)cnt0 + (double)cnt1)

Elements are listed in order of first appearance on the path.  The table is
a CSR over all leaves of all trees: trees in order, leaves in ascending
canonical node id within a tree.  engine/explain.py holds the arithmetic
that consumes it (numpy) and ops/hip/detector_shap.hip the kernel.
"""

from dataclasses import dataclass

import numpy as np

from .forest_ref import LEAF

FPAD = 16
_ABSENT = FPAD            # order slot of a feature not on the path
MAX_ELEMENTS = (1 << 31) - 1


@dataclass
class MergedPaths:
    tree_leaf_off: np.ndarray   # int32[T + 1] leaf range of every tree
    leaf_tree: np.ndarray       # int32[L]
    leaf_node: np.ndarray       # int64[L] tree-local canonical node id
    leaf_value: np.ndarray      # float64[L] cnt1 / (cnt0 + cnt1)
    leaf_off: np.ndarray        # int32[L + 1] CSR into the element arrays
    feature: np.ndarray         # uint8[E]
    lo: np.ndarray              # int16[E]
    hi: np.ndarray              # int16[E]
    z: np.ndarray               # float64[E]

    @property
    def n_leaves(self):
        return len(self.leaf_tree)

    @property
    def n_elements(self):
        return len(self.feature)

    def elements(self, leaf):
        """[(feature, lo, hi, z)] of one leaf, table order."""
        s = slice(self.leaf_off[leaf], self.leaf_off[leaf + 1])
        return list(zip(self.feature[s].tolist(), self.lo[s].tolist(),
                        self.hi[s].tolist(), self.z[s].tolist()))


def _check_element_count(n):
    if n > MAX_ELEMENTS:
        raise ValueError(
            f"explain: {n} path elements do not fit the int32 offsets")


def build_merged_paths(detector):
    """MergedPaths of `detector` (engine.detector.Detector, validated).

    Raises ValueError if a node reachable from a root has cover <= 0 (its
    cover ratio would be 0 or undefined, and z divides later), if a node is
    reached along two paths, or if the element count overflows int32."""
    d = detector
    T = int(d.n_trees)
    toff = d.tree_off.astype(np.int64)
    n_nodes = len(d.feat)
    feat = d.feat.astype(np.int64)
    cover = d.cnt0.astype(np.float64) + d.cnt1.astype(np.float64)
    base = np.repeat(toff[:-1], np.diff(toff))
    left = d.left.astype(np.int64) + base         # global ids

    lo = np.full((n_nodes, FPAD), -1, dtype=np.int16)
    hi = np.full((n_nodes, FPAD), 255, dtype=np.int16)
    z = np.ones((n_nodes, FPAD), dtype=np.float64)
    order = np.full((n_nodes, FPAD), _ABSENT, dtype=np.int8)
    count = np.zeros(n_nodes, dtype=np.int8)
    visits = np.zeros(n_nodes, dtype=np.int64)

    # level-synchronous walk down from the roots; a child's state is its
    # parent's with one feature's element narrowed / scaled
    frontier = toff[:-1].copy()
    while len(frontier):
        np.add.at(visits, frontier, 1)
        if not (cover[frontier] > 0).all():
            raise ValueError("explain: a reachable node has zero cover")
        parents = frontier[feat[frontier] != LEAF]
        if not len(parents):
            break
        f = feat[parents]
        s = d.split[parents].astype(np.int16)
        nxt = []
        for side in (0, 1):
            child = left[parents] + side
            lo[child], hi[child] = lo[parents], hi[parents]
            z[child], order[child] = z[parents], order[parents]
            if side == 0:
                hi[child, f] = np.minimum(hi[parents, f], s)
            else:
                lo[child, f] = np.maximum(lo[parents, f], s)
            z[child, f] = z[parents, f] * (cover[child] / cover[parents])
            new = order[parents, f] == _ABSENT
            order[child, f] = np.where(new, count[parents],
                                       order[parents, f])
            count[child] = count[parents] + new
            nxt.append(child)
        frontier = np.concatenate(nxt)
    if (visits > 1).any():
        raise ValueError("explain: a node is reachable along two paths")

    leaves = np.flatnonzero((visits == 1) & (feat == LEAF))   # ascending
    leaf_tree = (np.searchsorted(toff, leaves, side="right") - 1)
    n_el = count[leaves].astype(np.int64)
    _check_element_count(int(n_el.sum()))
    leaf_off = np.zeros(len(leaves) + 1, dtype=np.int64)
    leaf_off[1:] = np.cumsum(n_el)

    # features of a leaf sorted by first appearance; absent ones sort last
    by_order = np.argsort(order[leaves], axis=1, kind="stable")
    keep = np.arange(FPAD)[None, :] < n_el[:, None]
    rows = np.repeat(leaves, n_el)
    cols = by_order[keep]
    tree_leaf_off = np.searchsorted(leaf_tree, np.arange(T + 1))
    return MergedPaths(
        tree_leaf_off=tree_leaf_off.astype(np.int32),
        leaf_tree=leaf_tree.astype(np.int32),
        leaf_node=leaves - toff[leaf_tree],
        leaf_value=(d.cnt1[leaves].astype(np.float64) / cover[leaves]),
        leaf_off=leaf_off.astype(np.int32),
        feature=cols.astype(np.uint8),
        lo=lo[rows, cols], hi=hi[rows, cols], z=z[rows, cols])
