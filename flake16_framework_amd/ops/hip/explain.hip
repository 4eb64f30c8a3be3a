// TreeSHAP of a saved detector over merged leaf paths, gfx950.
//
//   detector_shap_tree_kernel     one thread per (row, tree): the tree's
//                                 class-1 attribution sums for the row
//   detector_shap_combine_kernel  tree sums -> phi, in the association of
//                                 forest_proba (blocks of PREDICT_TREE_BLOCK)
//
// The path table (models/mergedpaths.py) holds, per leaf, at most FPAD
// elements: every repeated feature of the root->leaf path is merged into
// one (interval, cover-ratio product).  So the recursion's UNWIND never
// runs along a path, and the per-(leaf, row) state is 17 fp64 weights and
// a 16-bit hot mask, kept in registers: every loop over a path position
// is fully unrolled with a wave-uniform predicate, so w[] is only ever
// indexed by constants.  Lane = row; the tree comes from blockIdx.y and
// the leaf loop is uniform, so the table is read with scalar loads.
//
// Bit-parity contract (host side: engine/explain.py, which pins the order
// of every operation; all fp64, contraction off):
//   EXTEND      w[i+1] += po * w[i] * (i+1) / (l+1)
//               w[i]    = pz * w[i] * (l-i) / (l+1)         left to right
//   unwound sum as models/treeshap_ref._unwound_sum, hot and cold form
//   term        unwound_sum * (o - z) * v
//   tree sum    from 0.0, leaves ascending, elements in table order
// po is 0.0 or 1.0: the cold lanes skip their first line (it would add
// po * ... = 0.0), which is exact for finite weights.
//
// Packed element (elem_code, int32): feature | (lo + 1) << 8 | hi << 20,
// hot iff lo < code[feature] <= hi.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

#ifndef FPAD
#define FPAD 16
#endif
#ifndef PREDICT_TREE_BLOCK
#define PREDICT_TREE_BLOCK 10
#endif

#define EXPLAIN_BLK 256

// partial layout: [tree][feature][row of the chunk], so a wave's store of
// one feature is 512 contiguous bytes.
__global__ __launch_bounds__(EXPLAIN_BLK) void detector_shap_tree_kernel(
    const uint8_t* __restrict__ codes,        // [M, FPAD]
    const int* __restrict__ tree_leaf_off,    // [T + 1]
    const int* __restrict__ leaf_off,         // [L + 1]
    const double* __restrict__ leaf_val,      // [L]
    const int* __restrict__ elem_code,        // [E] packed, see above
    const double* __restrict__ elem_z,        // [E]
    int row0, int m_chunk,
    double* __restrict__ partial /* [T, FPAD, m_chunk] */) {
    const int t = blockIdx.y;
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
        const int n = min(leaf_off[leaf + 1] - e0, FPAD);
        const double v = leaf_val[leaf];

        uint32_t hot = 0u;
        for (int k = 0; k < n; ++k) {
            const int ec = elem_code[e0 + k];
            const int f = ec & 0xFF;
            const int code =
                (int)(((f & 8 ? c_hi : c_lo) >> ((f & 7) * 8)) & 0xFF);
            const int lo1 = (ec >> 8) & 0x1FF, hi = (ec >> 20) & 0xFF;
            hot |= (uint32_t)(code >= lo1 && code <= hi) << k;
        }

        // EXTEND from the sentinel (w[0] = 1) with each element; l is the
        // path length before the element, sentinel included
        double w[FPAD + 1];
        w[0] = 1.0;
#pragma unroll
        for (int i = 1; i <= FPAD; ++i) w[i] = 0.0;
        for (int k = 0; k < n; ++k) {
            const int l = k + 1;
            const double pz = elem_z[e0 + k];
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
            const double z = elem_z[e0 + k];
            const int f = elem_code[e0 + k] & 0xFF;
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
            const double term = total * ((po ? 1.0 : 0.0) - z) * v;
#pragma unroll
            for (int g = 0; g < FPAD; ++g)
                if (g == f) acc[g] += term;
        }
    }

    if (r < m_chunk) {
#pragma unroll
        for (int f = 0; f < FPAD; ++f)
            partial[((size_t)t * FPAD + f) * m_chunk + r] = acc[f];
    }
}

// One thread per (row, feature), rows fastest across lanes: tree sums
// added sequentially within blocks of PREDICT_TREE_BLOCK trees from 0.0,
// blocks in ascending order, the total divided by n_trees.
__global__ __launch_bounds__(EXPLAIN_BLK) void detector_shap_combine_kernel(
    const double* __restrict__ partial,       // [T, FPAD, m_chunk]
    int row0, int m_chunk, int n_trees,
    double* __restrict__ phi /* [M, FPAD] */) {
    const int r = blockIdx.x * EXPLAIN_BLK + threadIdx.x;
    const int f = blockIdx.y;
    if (r >= m_chunk) return;
    double total = 0.0;
    for (int t0 = 0; t0 < n_trees; t0 += PREDICT_TREE_BLOCK) {
        const int t1 = min(n_trees, t0 + PREDICT_TREE_BLOCK);
        double blk = 0.0;
        for (int t = t0; t < t1; ++t)
            blk += partial[((size_t)t * FPAD + f) * m_chunk + r];
        total += blk;
    }
    phi[(size_t)(row0 + r) * FPAD + f] = total / (double)n_trees;
}
