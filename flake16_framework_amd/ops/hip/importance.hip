// Permutation-importance kernel (engine/importance.py), gfx950.
//
// Job (j, r) replaces the raw columns of mask_j in every row by those of
// row perm_r[row] (a row of the same group), classifies the row again and
// counts [FP, FN, TP] per group and pooled.  One launch serves all J * R
// jobs: nothing of size J * R * M (rows, codes or sums) exists in memory.
//
//   permuted_counts_kernel   block = 64 rows of one group (the int4 block
//                            table of holdout.hip, w = the group's
//                            detector), lane = row, wave = job, striding
//                            over the jobs of the block's blockIdx.y share.
//                            Per (row, job): gather the masked columns of
//                            the source row, encode in registers, walk the
//                            detector's forest, apply the rule, count.
//
// The unpermuted rows are encoded and summed once per call by
// holdout_encode_kernel and holdout_proba_kernel; this kernel reads their
// codes and (acc0, acc1) per row, keeps them in registers across its jobs
// and counts the baseline from them (blockIdx.y == 0, wave 0).  The
// block's parameters and cuts are staged into LDS once.
//
// Bit-parity contract: that of detector_steps.h for codes, sums and the
// rule, and
//   - counts are integers: a wave holds all of its block's rows for a job,
//     so a cell's block total is a popcount of a ballot, added with one
//     integer atomic per non-zero cell to the group's row and to the pooled
//     row.  No floating-point atomics.
// Two shortcuts, both exact: without a projection only the masked columns
// are searched again (the other code bytes are the baseline's), and a row
// whose 16 codes equal its baseline codes takes the baseline's sums.
//
// The kernel follows perm unchecked: the host op refuses a table with an
// entry outside the row's own group before anything is launched.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detector_steps.h"

#pragma clang fp contract(off)

#define IMPORTANCE_ROWS 64        // rows per block: one per lane
#define IMPORTANCE_WAVES (DETECT_BLK / IMPORTANCE_ROWS)

template <bool HAS_PCA>
__global__ __launch_bounds__(DETECT_BLK) void permuted_counts_kernel(
    const double* __restrict__ X,          // [M, FPAD] raw, zero-padded
    const uint8_t* __restrict__ labels,    // [M]
    const int4* __restrict__ blk_tab,      // [gridDim.x] w = detector
    const uint8_t* __restrict__ base_codes,    // [M, FPAD]
    const double2* __restrict__ base_acc,  // [M]
    const int* __restrict__ perm,          // [R, M] source rows
    const int* __restrict__ masks,         // [J] column masks
    const double* __restrict__ mean,       // [D, FPAD]
    const double* __restrict__ scale,      // [D, FPAD]
    const double* __restrict__ pca_mean,   // [D, FPAD]
    const double* __restrict__ W,          // [D, FPAD, FPAD], W[d][f][k]
    const float* __restrict__ cuts,        // flat, all detectors
    const int* __restrict__ cut_off,       // [D, FPAD + 1] detector-local
    const int* __restrict__ cut_base,      // [D] detector's first cut
    int F,
    const long* __restrict__ tree_off,     // [D * n_trees + 1] root ids
    const int2* __restrict__ nodes,        // packed records, all detectors
    int n_trees, int n_blocks, int n_jobs, int R, int M, int G,
    double threshold,                      // < 0: argmax rule
    int* __restrict__ counts,              // [J, R, G + 1, 3] zeroed
    int* __restrict__ baseline /* [G + 1, 3] zeroed */) {
    // s_own is placed on a 16-byte boundary: 8 B of padding follow the
    // 18,824 B of s
    __shared__ DetectorLds s;
    __shared__ double s_own[HAS_PCA ? FPAD * IMPORTANCE_ROWS : 1];

    const int tid = threadIdx.x;
    const int lane = tid % IMPORTANCE_ROWS;
    const int wave = __builtin_amdgcn_readfirstlane(tid / IMPORTANCE_ROWS);
    const int4 blk = blk_tab[blockIdx.x];
    const int g = blk.x, d = blk.w;
    stage_detector(s, mean + d * FPAD, scale + d * FPAD,
                   pca_mean + d * FPAD, W + (size_t)d * FPAD * FPAD,
                   cuts + cut_base[d], cut_off + d * (FPAD + 1));

    // lanes past the block's last row repeat it and are left out of the
    // counts, so every lane reads valid rows and the wave never diverges
    // on liveness
    const bool live = blk.y + lane < blk.z;
    const int row = live ? blk.y + lane : blk.z - 1;
    const int y = labels[row] != 0;
    const RowCodes b_codes = load_codes(base_codes, row);
    const double2 b_acc = base_acc[row];
    const long* roots = tree_off + (size_t)d * n_trees;

    // with a projection every code depends on every column: the rows'
    // own centred values z[f] - pca_mean[f] are kept in LDS, column-major
    // (the block's waves share their rows; wave w fills columns 4w..4w+3)
    if (HAS_PCA) {
        for (int f = wave * (FPAD / IMPORTANCE_WAVES);
             f < (wave + 1) * (FPAD / IMPORTANCE_WAVES); ++f)
            s_own[f * IMPORTANCE_ROWS + lane] =
                scaled(s, f, X[(size_t)row * FPAD + f]) - s.pmean[f];
        __syncthreads();
    }

    if (blockIdx.y == 0 && wave == 0) {
        const bool pred = predicted(b_acc, n_trees, threshold);
        const int fp = __popcll(__ballot(live && pred && !y));
        const int fn = __popcll(__ballot(live && !pred && y));
        const int tp = __popcll(__ballot(live && pred && y));
        if (lane < 3) {
            const int n = lane == 0 ? fp : lane == 1 ? fn : tp;
            if (n) {
                atomicAdd(baseline + g * 3 + lane, n);
                atomicAdd(baseline + G * 3 + lane, n);
            }
        }
    }

    for (int job = blockIdx.y * IMPORTANCE_WAVES + wave; job < n_jobs;
         job += gridDim.y * IMPORTANCE_WAVES) {
        const int mask = masks[job / R];
        const double* xs =
            X + (size_t)perm[(size_t)(job % R) * M + row] * FPAD;

        // f and the mask are wave-uniform: the column loops stay rolled
        // so that one column's load, division and search are live at a
        // time
        RowCodes c;
        if (HAS_PCA) {
            double t[FPAD];
#pragma unroll
            for (int k = 0; k < FPAD; ++k) t[k] = 0.0;
#pragma unroll 1
            for (int f = 0; f < F; ++f) {
                double dv;
                if (mask >> f & 1)
                    dv = scaled(s, f, xs[f]) - s.pmean[f];
                else
                    dv = s_own[f * IMPORTANCE_ROWS + lane];
#pragma unroll
                for (int k = 0; k < FPAD; ++k)
                    t[k] = t[k] + dv * s.W[f * FPAD + k];
            }
            c = search_codes(s, t, F);
        } else {
            c = b_codes;
#pragma unroll 1
            for (int m = mask; m; m &= m - 1) {
                const int f = __builtin_ctz(m);
                c = with_code(c, f, cut_code(s, f, scaled(s, f, xs[f])));
            }
        }

        const double2 acc = same_codes(c, b_codes)
            ? b_acc : forest_sums(nodes, roots, n_trees, n_blocks, c);
        const bool pred = predicted(acc, n_trees, threshold);
        const int fp = __popcll(__ballot(live && pred && !y));
        const int fn = __popcll(__ballot(live && !pred && y));
        const int tp = __popcll(__ballot(live && pred && y));
        if (lane < 3) {
            const int n = lane == 0 ? fp : lane == 1 ? fn : tp;
            if (n) {
                int* out = counts + (size_t)job * (G + 1) * 3;
                atomicAdd(out + g * 3 + lane, n);
                atomicAdd(out + G * 3 + lane, n);
            }
        }
    }
}

// Both forms are instantiated here, so that compiling this file alone with
// -Rpass-analysis=kernel-resource-usage reports them
// (profiles/importance.md).
#define PERMUTED_COUNTS_INSTANCE(HAS_PCA)                                   \
    template __global__ void permuted_counts_kernel<HAS_PCA>(               \
        const double*, const uint8_t*, const int4*, const uint8_t*,         \
        const double2*, const int*, const int*, const double*,              \
        const double*, const double*, const double*, const float*,          \
        const int*, const int*, int, const long*, const int2*, int, int,    \
        int, int, int, int, double, int*, int*)
PERMUTED_COUNTS_INSTANCE(false);
PERMUTED_COUNTS_INSTANCE(true);
#undef PERMUTED_COUNTS_INSTANCE
