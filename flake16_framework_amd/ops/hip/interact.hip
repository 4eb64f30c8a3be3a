// SHAP interaction values of a saved detector over merged leaf paths,
// gfx950.
//
//   detector_interact_tree_kernel     one thread per (row, tree, conditioned
//                                     feature g): the tree's sums for the
//                                     pairs (g, f), f = 0..FPAD-1
//   detector_interact_combine_kernel  one thread per (row, g): tree sums ->
//                                     Phi[g, :], off the diagonal in the
//                                     association of forest_proba, then the
//                                     diagonal from phi
//
// A feature appears at most once in a merged path (models/mergedpaths.py),
// so conditioning on g is "drop its element c from the path": the tree
// kernel is detector_shap_tree_kernel (explain.hip) run on the path without
// c, every term scaled by (o_c - z_c).  The state per (leaf, row) stays 17
// fp64 weights and the hot mask, w[] and acc[] indexed by constants only.
// Lane = row; tree and g come from blockIdx, so the leaf loop, the position
// of g in the leaf and every table read are wave-uniform, and a leaf
// without g is skipped by the whole wave.
//
// Bit-parity contract (host side: engine/interact.py; all fp64, contraction
// off).  With the reduced path r_0..r_{n-2} (table order without c):
//   EXTEND, unwound sum and term   as explain.hip, on the reduced path
//   contribution to (g, f_k)       term_k * (o_c - z_c)
//   tree sum                       from 0.0, leaves ascending, reduced
//                                  elements in table order
//   Phi[g, f], f != g              tree sums in blocks of PREDICT_TREE_BLOCK
//                                  as detector_shap_combine_kernel,
//                                  / n_trees, * 0.5
//   Phi[g, g]                      phi[g] - s, s = Phi[g, f] added for f
//                                  ascending without g, from 0.0
// Entries with g >= F or f >= F are 0.0: the op zero-fills the output and
// no element names such a feature.

#pragma once

#include "explain.hip"

#pragma clang fp contract(off)

// partial layout: [tree][g][f][row of the chunk]
__global__ __launch_bounds__(EXPLAIN_BLK) void detector_interact_tree_kernel(
    const uint8_t* __restrict__ codes,        // [M, FPAD]
    const int* __restrict__ tree_leaf_off,    // [T + 1]
    const int* __restrict__ leaf_off,         // [L + 1]
    const double* __restrict__ leaf_val,      // [L]
    const int* __restrict__ elem_code,        // [E] packed as in explain.hip
    const double* __restrict__ elem_z,        // [E]
    int row0, int m_chunk,
    double* __restrict__ partial /* [T, F, FPAD, m_chunk], F = gridDim.z */) {
    const int t = blockIdx.y;
    const int g = blockIdx.z;
    const int r = blockIdx.x * EXPLAIN_BLK + threadIdx.x;
    // lanes past the chunk redo its last row and store nothing, which
    // keeps every loop below wave-uniform
    const int row = row0 + min(r, m_chunk - 1);

    const uint4 cw = *(const uint4*)(codes + (size_t)row * FPAD);
    const uint64_t c_lo = (uint64_t)cw.x | ((uint64_t)cw.y << 32);
    const uint64_t c_hi = (uint64_t)cw.z | ((uint64_t)cw.w << 32);

    double acc[FPAD];
#pragma unroll
    for (int f = 0; f < FPAD; ++f) acc[f] = 0.0;

    const int leaf_end = tree_leaf_off[t + 1];
    for (int leaf = tree_leaf_off[t]; leaf < leaf_end; ++leaf) {
        const int e0 = leaf_off[leaf];
        const int n_all = min(leaf_off[leaf + 1] - e0, FPAD);

        // position of g in the leaf; with it alone there is no pair
        int c = -1;
        for (int k = 0; k < n_all; ++k)
            if ((elem_code[e0 + k] & 0xFF) == g) c = k;
        if (c < 0 || n_all < 2) continue;
        const int n = n_all - 1;              // reduced path
        const double v = leaf_val[leaf];

        // bit k' of hot: reduced element k', which is table element
        // k' + (k' >= c)
        uint32_t hot = 0u;
        bool oc = false;
        for (int k = 0; k < n_all; ++k) {
            const int ec = elem_code[e0 + k];
            const int f = ec & 0xFF;
            const int code =
                (int)(((f & 8 ? c_hi : c_lo) >> ((f & 7) * 8)) & 0xFF);
            const int lo1 = (ec >> 8) & 0x1FF, hi = (ec >> 20) & 0xFF;
            const bool h = code >= lo1 && code <= hi;
            if (k == c) oc = h;
            else hot |= (uint32_t)h << (k - (k > c));
        }
        const double cond = (oc ? 1.0 : 0.0) - elem_z[e0 + c];

        double w[FPAD + 1];
        w[0] = 1.0;
#pragma unroll
        for (int i = 1; i <= FPAD; ++i) w[i] = 0.0;
        for (int k = 0; k < n; ++k) {
            const int l = k + 1;
            const double pz = elem_z[e0 + k + (k >= c)];
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

        const double len = (double)(n + 1);
        double w_top = w[0];
#pragma unroll
        for (int i = 1; i <= FPAD; ++i) w_top = (i == n) ? w[i] : w_top;
        for (int k = 0; k < n; ++k) {
            const int e = e0 + k + (k >= c);
            const double z = elem_z[e];
            const int f = elem_code[e] & 0xFF;
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
            const double term = total * ((po ? 1.0 : 0.0) - z) * v * cond;
#pragma unroll
            for (int h = 0; h < FPAD; ++h)
                if (h == f) acc[h] += term;
        }
    }

    if (r < m_chunk) {
        const size_t base = ((size_t)t * gridDim.z + g) * FPAD;
#pragma unroll
        for (int f = 0; f < FPAD; ++f)
            partial[(base + f) * m_chunk + r] = acc[f];
    }
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
        double total = 0.0;
        for (int t0 = 0; t0 < n_trees; t0 += PREDICT_TREE_BLOCK) {
            const int t1 = min(n_trees, t0 + PREDICT_TREE_BLOCK);
            double blk = 0.0;
            for (int t = t0; t < t1; ++t)
                blk += partial[(((size_t)t * F + g) * FPAD + f) * m_chunk + r];
            total += blk;
        }
        const double v = total / (double)n_trees * 0.5;
        o[f] = v;
        s += v;
    }
    o[g] = phi[(size_t)(row0 + r) * FPAD + g] - s;
}
