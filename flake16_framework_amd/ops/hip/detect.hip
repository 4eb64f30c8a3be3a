// Inference kernels for a saved detector (engine/detector.py), gfx950.
//
//   detect_encode_kernel   raw fp64 feature rows -> uint8 bin codes, one
//                          pass: scale, optional PCA projection, fp32
//                          cast, binary search of the feature's cuts
//   forest_proba_partial_kernel / forest_proba_combine_kernel
//                          per-row (acc0, acc1) class-probability sums
//                          over a packed inference forest
//
// The steps, the packed node format and the bit-parity contract are in
// detector_steps.h.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detector_steps.h"

#pragma clang fp contract(off)

// One thread per row.  Parameters and cuts are staged into LDS once per
// block.
__global__ __launch_bounds__(DETECT_BLK) void detect_encode_kernel(
    const double* __restrict__ X,          // [M, FPAD] raw, zero-padded
    const double* __restrict__ mean,       // [FPAD]
    const double* __restrict__ scale,      // [FPAD]
    const double* __restrict__ pca_mean,   // [FPAD]
    const double* __restrict__ W,          // [FPAD, FPAD], W[f][k]
    int has_pca,
    const float* __restrict__ cuts,        // flat, cut_off[FPAD] entries
    const int* __restrict__ cut_off,       // [FPAD + 1]
    int M, int F,
    uint8_t* __restrict__ codes /* [M, FPAD] */) {
    __shared__ DetectorLds s;
    stage_detector(s, mean, scale, pca_mean, W, cuts, cut_off);

    const long row = (long)blockIdx.x * DETECT_BLK + threadIdx.x;
    if (row >= M) return;
    store_codes(codes, row,
                encode_row(s, X + (size_t)row * FPAD, has_pca, F));
}

// Stage 1: one thread per (row, block of PREDICT_TREE_BLOCK trees), rows
// fastest across lanes so a wave walks the same trees.  The row's 16 code
// bytes live in two 64-bit registers; the walk is one 8-byte node load
// per level.  Partial sums leave with plain stores.
__global__ __launch_bounds__(DETECT_BLK) void forest_proba_partial_kernel(
    const uint8_t* __restrict__ codes,     // [M, FPAD]
    const long* __restrict__ tree_off,     // [T + 1] root ids
    const int2* __restrict__ nodes,        // packed records
    int M, int n_trees, int n_blocks,
    double2* __restrict__ partial /* [n_blocks, M] */) {
    const long idx = (long)blockIdx.x * DETECT_BLK + threadIdx.x;
    if (idx >= (long)M * n_blocks) return;
    const int row = (int)(idx % M);
    const int tb = (int)(idx / M);
    partial[(size_t)tb * M + row] = tree_block_sums(
        nodes, tree_off, tb, n_trees, load_codes(codes, row));
}

// Stage 2: one thread per row, tree blocks added in ascending order.
__global__ __launch_bounds__(DETECT_BLK) void forest_proba_combine_kernel(
    const double2* __restrict__ partial, int M, int n_blocks,
    double2* __restrict__ acc /* [M] */) {
    const long row = (long)blockIdx.x * DETECT_BLK + threadIdx.x;
    if (row >= M) return;
    double acc0 = 0.0, acc1 = 0.0;
    for (int tb = 0; tb < n_blocks; ++tb) {
        const double2 p = partial[(size_t)tb * M + row];
        acc0 += p.x;
        acc1 += p.y;
    }
    acc[row] = make_double2(acc0, acc1);
}
