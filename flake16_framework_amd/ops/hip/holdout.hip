// Grouped evaluation kernels for leave-one-project-out runs
// (engine/holdout.py), gfx950.
//
// Rows arrive sorted by group; group g owns rows seg_off[g]:seg_off[g+1]
// and its own preprocessing parameters, cuts and forest.  Every kernel is
// launched over a host-built block table, one int4 per block:
//     x = group, y = first row, z = one past the block's last row
// so a block serves exactly one group, groups without rows get no block,
// and nothing is gathered per row.
//
//   holdout_encode_kernel     detect_encode_kernel's body with the block's
//                             group choosing parameters and cuts
//   holdout_proba_kernel      forest_proba in one launch: a wave per tree
//                             block, partial sums combined through LDS in
//                             ascending tree-block order
//   threshold_counts_kernel   per-group and pooled [FP, FN, TP] under the
//                             argmax rule and under proba >= t_k for K
//                             thresholds, integer atomics only
//
// Bit-parity contract: that of detector_steps.h, per group.
// holdout_encode is detect_encode on the group's slice; holdout_proba adds
// the tree-block sums in ascending order; threshold_counts forms
// proba = acc1 / (double)n_trees and counts with integers, so no result
// depends on scheduling.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detector_steps.h"

#pragma clang fp contract(off)

#define HOLDOUT_PROBA_ROWS 64     // rows per block: one per lane
#define HOLDOUT_PROBA_WAVES (DETECT_BLK / HOLDOUT_PROBA_ROWS)
#define HOLDOUT_MAX_K 256         // thresholds per call: one per thread

// One thread per row, DETECT_BLK rows per block; the group's parameters
// and cuts are staged once.  The waves-per-SIMD hint dates from the
// kernel's own copy of the encode body, which needed it to stay at 5 waves.
// With the shared body the kernel reaches 5 waves without it (81 VGPRs
// against 92 with it); it is kept only because the kernel without it has
// not been timed.
__global__ __launch_bounds__(DETECT_BLK)
__attribute__((amdgpu_waves_per_eu(5, 5))) void holdout_encode_kernel(
    const double* __restrict__ X,          // [M, FPAD] raw, zero-padded
    const int4* __restrict__ blk_tab,      // [gridDim.x]
    const double* __restrict__ mean,       // [G, FPAD]
    const double* __restrict__ scale,      // [G, FPAD]
    const double* __restrict__ pca_mean,   // [G, FPAD]
    const double* __restrict__ W,          // [G, FPAD, FPAD], W[g][f][k]
    int has_pca,
    const float* __restrict__ cuts,        // flat, all groups back to back
    const int* __restrict__ cut_off,       // [G, FPAD + 1] group-local
    const int* __restrict__ cut_base,      // [G] group's first cut
    int F,
    uint8_t* __restrict__ codes /* [M, FPAD] */) {
    __shared__ DetectorLds s;
    const int4 blk = blk_tab[blockIdx.x];
    const int g = blk.x;
    stage_detector(s, mean + g * FPAD, scale + g * FPAD,
                   pca_mean + g * FPAD, W + (size_t)g * FPAD * FPAD,
                   cuts + cut_base[g], cut_off + g * (FPAD + 1));

    const int row = blk.y + threadIdx.x;
    if (row >= blk.z) return;
    store_codes(codes, row,
                encode_row(s, X + (size_t)row * FPAD, has_pca, F));
}

// HOLDOUT_PROBA_ROWS rows per block, one per lane; wave w walks tree
// blocks w, w + WAVES, ... of the group's forest, so a wave reads one
// tree's root at a time as forest_proba_partial_kernel does.  After each
// round wave 0 adds that round's partial sums in ascending tree-block
// order, which is forest_proba_combine_kernel's order.
__global__ __launch_bounds__(DETECT_BLK) void holdout_proba_kernel(
    const uint8_t* __restrict__ codes,     // [M, FPAD]
    const int4* __restrict__ blk_tab,      // [gridDim.x]
    const long* __restrict__ tree_off,     // [G * n_trees + 1] root ids
    const int2* __restrict__ nodes,        // packed records, all groups
    int n_trees, int n_blocks,
    double2* __restrict__ acc /* [M] */) {
    __shared__ double2 s_part[HOLDOUT_PROBA_WAVES][HOLDOUT_PROBA_ROWS];

    const int lane = threadIdx.x % HOLDOUT_PROBA_ROWS;
    const int wave = threadIdx.x / HOLDOUT_PROBA_ROWS;
    const int4 blk = blk_tab[blockIdx.x];
    const long* roots = tree_off + (size_t)blk.x * n_trees;
    const int row = blk.y + lane;
    const bool live = row < blk.z;

    RowCodes c = {0, 0};
    if (live) c = load_codes(codes, row);

    double tot0 = 0.0, tot1 = 0.0;
    for (int tb0 = 0; tb0 < n_blocks; tb0 += HOLDOUT_PROBA_WAVES) {
        const int tb = tb0 + wave;
        double2 part = make_double2(0.0, 0.0);
        if (live && tb < n_blocks)
            part = tree_block_sums(nodes, roots, tb, n_trees, c);
        s_part[wave][lane] = part;
        __syncthreads();
        if (wave == 0) {
            const int nw = min(HOLDOUT_PROBA_WAVES, n_blocks - tb0);
            for (int w = 0; w < nw; ++w) {
                const double2 p = s_part[w][lane];
                tot0 += p.x;
                tot1 += p.y;
            }
        }
        __syncthreads();
    }
    if (wave == 0 && live) acc[row] = make_double2(tot0, tot1);
}

// One thread per row, DETECT_BLK rows per block.  A row falls into bin
// b = #{k : t_k <= proba} of its label's LDS histogram; it is predicted
// flaky at threshold k iff b > k, so FP[k] and TP[k] are suffix sums of
// the two histograms over bins k + 1 .. K (bin 0 is predicted flaky
// nowhere and only counts towards the block's positives).  Thread k then
// adds the block's [FP, FN, TP] at threshold k to its group's row and to
// the pooled row G.
__global__ __launch_bounds__(DETECT_BLK) void threshold_counts_kernel(
    const double2* __restrict__ acc,       // [M] (acc0, acc1)
    const uint8_t* __restrict__ labels,    // [M]
    const int4* __restrict__ blk_tab,      // [gridDim.x]
    const double* __restrict__ thresholds, // [K] ascending
    int K, int n_trees, int G,
    int* __restrict__ curve,               // [G + 1, K, 3] zeroed
    int* __restrict__ argmax /* [G + 1, 3] zeroed */) {
    __shared__ double s_thr[HOLDOUT_MAX_K];
    __shared__ int s_hist[2][HOLDOUT_MAX_K];   // bins 1 .. K
    __shared__ int s_zero[2];                  // bin 0
    __shared__ int s_arg[3];

    const int tid = threadIdx.x;
    const int4 blk = blk_tab[blockIdx.x];
    if (tid < K) s_thr[tid] = thresholds[tid];
    s_hist[0][tid] = 0;                    // DETECT_BLK == HOLDOUT_MAX_K
    s_hist[1][tid] = 0;
    if (tid < 2) s_zero[tid] = 0;
    if (tid < 3) s_arg[tid] = 0;
    __syncthreads();

    const int row = blk.y + tid;
    if (row < blk.z) {
        const double2 a = acc[row];
        const int y = labels[row] != 0;
        const double proba = a.y / (double)n_trees;
        int lo = 0, hi = K;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_thr[mid] <= proba) lo = mid + 1; else hi = mid;
        }
        atomicAdd(lo ? &s_hist[y][lo - 1] : &s_zero[y], 1);
        const int k = 2 * y + (a.y > a.x) - 1;   // -1: true negative
        if (k >= 0) atomicAdd(&s_arg[k], 1);
    }
    __syncthreads();

    // inclusive suffix sums: s_hist[l][k] = #{rows of label l, b > k}
    for (int off = 1; off < HOLDOUT_MAX_K; off <<= 1) {
        const bool in = tid + off < HOLDOUT_MAX_K;
        const int v0 = s_hist[0][tid] + (in ? s_hist[0][tid + off] : 0);
        const int v1 = s_hist[1][tid] + (in ? s_hist[1][tid + off] : 0);
        __syncthreads();
        s_hist[0][tid] = v0;
        s_hist[1][tid] = v1;
        __syncthreads();
    }

    if (tid < K) {
        const int fp = s_hist[0][tid];
        const int tp = s_hist[1][tid];
        const int fn = s_zero[1] + s_hist[1][0] - tp;
        int* grp = curve + ((size_t)blk.x * K + tid) * 3;
        int* all = curve + ((size_t)G * K + tid) * 3;
        if (fp) { atomicAdd(grp + 0, fp); atomicAdd(all + 0, fp); }
        if (fn) { atomicAdd(grp + 1, fn); atomicAdd(all + 1, fn); }
        if (tp) { atomicAdd(grp + 2, tp); atomicAdd(all + 2, tp); }
    }
    if (tid < 3 && s_arg[tid]) {
        atomicAdd(argmax + blk.x * 3 + tid, s_arg[tid]);
        atomicAdd(argmax + G * 3 + tid, s_arg[tid]);
    }
}
