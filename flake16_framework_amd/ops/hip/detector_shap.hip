// TreeSHAP and SHAP interaction values of a saved detector over merged
// leaf paths, gfx950.
//
//   detector_shap_tree_kernel<PAIRS>  one thread per (row, tree[, g]): the
//                                     tree's class-1 sums per feature;
//                                     PAIRS = false for the attributions,
//                                     true for the pairs (g, f) with the
//                                     conditioned feature g = blockIdx.z
//   detector_shap_combine_kernel      one thread per (row, feature): tree
//                                     sums -> phi
//   detector_interact_combine_kernel  one thread per (row, g): tree sums ->
//                                     Phi[g, :] off the diagonal, then the
//                                     diagonal from phi
//
// The path table (models/mergedpaths.py) holds, per leaf, at most FPAD
// elements: every repeated feature of the root->leaf path is merged into
// one (interval, cover-ratio product).  So the recursion's UNWIND never
// runs along a path, and the per-(leaf, row) state is 17 fp64 weights and
// a 16-bit hot mask, kept in registers: every loop over a path position
// is fully unrolled with a wave-uniform predicate, so w[] and acc[] are
// only ever indexed by constants.  Lane = row; the tree and g come from
// blockIdx and the leaf loop is uniform, so the table is read with scalar
// loads.  A feature appears at most once in a merged path, so conditioning
// on g is "drop its element c from the path": the position of g in the
// leaf is wave-uniform too, and a leaf without g is skipped by the whole
// wave.
//
// Bit-parity contract (host side: engine/explain.py and
// engine/interact.py, which pin the order of every operation; all fp64,
// contraction off).  This is its one statement.
//   EXTEND      w[i+1] += po * w[i] * (i+1) / (l+1)
//               w[i]    = pz * w[i] * (l-i) / (l+1)         left to right
//   unwound sum as models/treeshap_ref._unwound_sum, hot and cold form
//   term        unwound_sum * (o - z) * v
//   tree sum    from 0.0, leaves ascending, elements in table order
//   phi[f]      tree sums added sequentially within blocks of
//               PREDICT_TREE_BLOCK trees from 0.0, blocks ascending (the
//               association of forest_proba), / n_trees
// po is 0.0 or 1.0: the cold lanes skip their first line (it would add
// po * ... = 0.0), which is exact for finite weights.
// Interactions: as above, on the reduced path r_0..r_{n-2} (table order
// without c), and then
//   contribution to (g, f_k)   term_k * (o_c - z_c)
//   Phi[g, f], f != g          as phi[f], then * 0.5
//   Phi[g, g]                  phi[g] - s, s = Phi[g, f] added for f
//                              ascending without g, from 0.0
// Entries with g >= F or f >= F are 0.0: the op zero-fills the output and
// no element names such a feature.
//
// Packed element (elem_code, int32): feature | (lo + 1) << 8 | hi << 20,
// hot iff lo < code[feature] <= hi.

#pragma once

#include "detector_steps.h"

#pragma clang fp contract(off)

#define EXPLAIN_BLK 256

// partial layout: [tree][g][feature][row of the chunk] with gridDim.z
// slots g (one when !PAIRS), so a wave's store of one feature is 512
// contiguous bytes.
template <bool PAIRS>
__global__ __launch_bounds__(EXPLAIN_BLK) void detector_shap_tree_kernel(
    const uint8_t* __restrict__ codes,        // [M, FPAD]
    const int* __restrict__ tree_leaf_off,    // [T + 1]
    const int* __restrict__ leaf_off,         // [L + 1]
    const double* __restrict__ leaf_val,      // [L]
    const int* __restrict__ elem_code,        // [E] packed, see above
    const double* __restrict__ elem_z,        // [E]
    int row0, int m_chunk,
    double* __restrict__ partial /* [T, gridDim.z, FPAD, m_chunk] */) {
    const int t = blockIdx.y;
    const int g = PAIRS ? blockIdx.z : 0;
    const int r = blockIdx.x * EXPLAIN_BLK + threadIdx.x;
    // lanes past the chunk redo its last row and store nothing, which
    // keeps every loop below wave-uniform
    const int row = row0 + min(r, m_chunk - 1);
    const RowCodes rc = load_codes(codes, (size_t)row);

    double acc[FPAD];
#pragma unroll
    for (int f = 0; f < FPAD; ++f) acc[f] = 0.0;

    const int leaf_end = tree_leaf_off[t + 1];
    for (int leaf = tree_leaf_off[t]; leaf < leaf_end; ++leaf) {
        const int e0 = leaf_off[leaf];
        const int n_all = min(leaf_off[leaf + 1] - e0, FPAD);

        // position of g in the leaf; with it alone there is no pair
        int c = -1;
        if (PAIRS) {
            for (int k = 0; k < n_all; ++k)
                if ((elem_code[e0 + k] & 0xFF) == g) c = k;
            if (c < 0 || n_all < 2) continue;
        }
        const int n = PAIRS ? n_all - 1 : n_all;    // (reduced) path
        // table index of path element k: c is stepped over
        const auto at = [&](int k) { return e0 + k + (PAIRS && k >= c); };
        const double v = leaf_val[leaf];

        // bit k of hot: path element k
        uint32_t hot = 0u;
        bool oc = false;
        for (int k = 0; k < n_all; ++k) {
            const int ec = elem_code[e0 + k];
            const int code = code_of(rc, ec & 0xFF);
            const int lo1 = (ec >> 8) & 0x1FF, hi = (ec >> 20) & 0xFF;
            const bool h = code >= lo1 && code <= hi;
            if (PAIRS && k == c) oc = h;
            else hot |= (uint32_t)h << (k - (PAIRS && k > c));
        }
        // o_c - z_c; without PAIRS nothing reads cond, c or oc
        const double cond = PAIRS ? (oc ? 1.0 : 0.0) - elem_z[e0 + c] : 0.0;

        // EXTEND from the sentinel (w[0] = 1) with each element; l is the
        // path length before the element, sentinel included
        double w[FPAD + 1];
        w[0] = 1.0;
#pragma unroll
        for (int i = 1; i <= FPAD; ++i) w[i] = 0.0;
        for (int k = 0; k < n; ++k) {
            const int l = k + 1;
            const double pz = elem_z[at(k)];
            const bool po = (hot >> k) & 1u;
            const double l1 = (double)(l + 1);
#pragma unroll
            for (int i = FPAD - 1; i >= 0; --i) {
                if (i < l) {
                    const double wi = w[i];
                    if (po) w[i + 1] += wi * (double)(i + 1) / l1;
                    w[i] = pz * wi * (double)(l - i) / l1;
                }
            }
        }

        // one term per element; the path has n + 1 entries
        const double len = (double)(n + 1);
        double w_top = w[0];
#pragma unroll
        for (int i = 1; i <= FPAD; ++i) w_top = (i == n) ? w[i] : w_top;
        for (int k = 0; k < n; ++k) {
            const double z = elem_z[at(k)];
            const int f = elem_code[at(k)] & 0xFF;
            const bool po = (hot >> k) & 1u;
            double total = 0.0;
            if (po) {
                double nx = w_top;
#pragma unroll
                for (int j = FPAD - 1; j >= 0; --j) {
                    if (j < n) {
                        const double tj = nx * len / (double)(j + 1);
                        total += tj;
                        nx = w[j] - tj * z * (double)(n - j) / len;
                    }
                }
            } else {
#pragma unroll
                for (int j = FPAD - 1; j >= 0; --j) {
                    if (j < n)
                        total += w[j] * len / (z * (double)(n - j));
                }
            }
            double term = total * ((po ? 1.0 : 0.0) - z) * v;
            if (PAIRS) term = term * cond;
#pragma unroll
            for (int h = 0; h < FPAD; ++h)
                if (h == f) acc[h] += term;
        }
    }

    if (r < m_chunk) {
        const size_t base = ((size_t)t * (PAIRS ? gridDim.z : 1) + g) * FPAD;
#pragma unroll
        for (int f = 0; f < FPAD; ++f)
            partial[(base + f) * m_chunk + r] = acc[f];
    }
}

// p[t * stride], t = 0..n_trees-1, in the association of forest_proba:
// added sequentially within blocks of PREDICT_TREE_BLOCK trees from 0.0,
// the block sums added to 0.0 in ascending order.
__device__ __forceinline__ double blocked_tree_sum(
    const double* __restrict__ p, size_t stride, int n_trees) {
    double total = 0.0;
    for (int t0 = 0; t0 < n_trees; t0 += PREDICT_TREE_BLOCK) {
        const int t1 = min(n_trees, t0 + PREDICT_TREE_BLOCK);
        double blk = 0.0;
        for (int t = t0; t < t1; ++t) blk += p[t * stride];
        total += blk;
    }
    return total;
}

// One thread per (row, feature), rows fastest across lanes.
__global__ __launch_bounds__(EXPLAIN_BLK) void detector_shap_combine_kernel(
    const double* __restrict__ partial,       // [T, FPAD, m_chunk]
    int row0, int m_chunk, int n_trees,
    double* __restrict__ phi /* [M, FPAD] */) {
    const int r = blockIdx.x * EXPLAIN_BLK + threadIdx.x;
    const int f = blockIdx.y;
    if (r >= m_chunk) return;
    const double total = blocked_tree_sum(
        partial + (size_t)f * m_chunk + r, (size_t)FPAD * m_chunk, n_trees);
    phi[(size_t)(row0 + r) * FPAD + f] = total / (double)n_trees;
}

// One thread per (row, g), rows fastest across lanes.  out is zero-filled
// by the caller; row g of the row's matrix is written for g < F only.
__global__ __launch_bounds__(EXPLAIN_BLK) void
detector_interact_combine_kernel(
    const double* __restrict__ partial,       // [T, F, FPAD, m_chunk]
    const double* __restrict__ phi,           // [M, FPAD]
    int row0, int m_chunk, int n_trees,
    double* __restrict__ out /* [M, FPAD, FPAD] */) {
    const int r = blockIdx.x * EXPLAIN_BLK + threadIdx.x;
    const int g = blockIdx.y, F = gridDim.y;
    if (r >= m_chunk) return;
    double* o = out + ((size_t)(row0 + r) * FPAD + g) * FPAD;
    double s = 0.0;
    for (int f = 0; f < F; ++f) {
        if (f == g) continue;
        const double total = blocked_tree_sum(
            partial + ((size_t)g * FPAD + f) * m_chunk + r,
            (size_t)F * FPAD * m_chunk, n_trees);
        const double v = total / (double)n_trees * 0.5;
        o[f] = v;
        s += v;
    }
    o[g] = phi[(size_t)(row0 + r) * FPAD + g] - s;
}
