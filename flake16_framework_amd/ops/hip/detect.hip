// Inference kernels for a saved detector (engine/detector.py), gfx950.
//
//   detect_encode_kernel   raw fp64 feature rows -> uint8 bin codes, one
//                          pass: scale, optional PCA projection, fp32
//                          cast, binary search of the feature's cuts
//   forest_proba_partial_kernel / forest_proba_combine_kernel
//                          per-row (acc0, acc1) class-probability sums
//                          over a packed inference forest
//
// Bit-parity contract (host side: preprocess.transform_preprocessing,
// models/binning.bin_codes, models/forest_ref.accumulate_proba):
//   - z[f] = (x[f] - mean[f]) / scale[f]                       (fp64)
//   - t[k] = sum over ascending f of (z[f] - pca_mean[f]) * W[f][k],
//     from 0.0, separate multiply and add — contraction must stay off
//     (the build passes -ffp-contract=off; the pragma below pins it for
//     this file whatever the command line says)
//   - code = #{cut <= (float)value}
//   - tree probabilities summed sequentially within blocks of
//     PREDICT_TREE_BLOCK trees, blocks added in ascending order.
//
// Packed node (8 bytes, one load per tree level):
//   internal  x = 0x80000000 | id of the left child (global, into the
//                 packed array; the right child is the next record)
//             y = split_bin << 8 | feature
//   leaf      x, y = bit patterns of the fp32 class counts cnt0, cnt1
// Counts are non-negative, so the sign bit of x tells the kinds apart.

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

#define DETECT_BLK 256
#define DETECT_MAX_CUTS 255   // per feature: codes are uint8

// One thread per row.  Parameters and cuts are staged into LDS once per
// block (2432 B of doubles + <= 16320 B of cuts + the offset table); the
// projection reads them wave-uniformly (LDS broadcast).
__global__ __launch_bounds__(DETECT_BLK) void detect_encode_kernel(
    const double* __restrict__ X,          // [M, FPAD] raw, zero-padded
    const double* __restrict__ mean,       // [FPAD]
    const double* __restrict__ scale,      // [FPAD]
    const double* __restrict__ pca_mean,   // [FPAD]
    const double* __restrict__ W,          // [FPAD, FPAD], W[f][k]
    int has_pca,
    const float* __restrict__ cuts,        // flat, n_cuts entries
    const int* __restrict__ cut_off,       // [FPAD + 1]
    int n_cuts, int M, int F,
    uint8_t* __restrict__ codes /* [M, FPAD] */) {
    __shared__ double s_mean[FPAD], s_scale[FPAD], s_pmean[FPAD];
    __shared__ double s_W[FPAD * FPAD];
    __shared__ float s_cuts[FPAD * DETECT_MAX_CUTS];
    __shared__ int s_off[FPAD + 1];

    const int tid = threadIdx.x;
    if (tid < FPAD) {
        s_mean[tid] = mean[tid];
        s_scale[tid] = scale[tid];
        s_pmean[tid] = pca_mean[tid];
    }
    if (tid <= FPAD) s_off[tid] = cut_off[tid];
    s_W[tid] = W[tid];                     // DETECT_BLK == FPAD * FPAD
    for (int i = tid; i < n_cuts; i += DETECT_BLK) s_cuts[i] = cuts[i];
    __syncthreads();

    const long row = (long)blockIdx.x * DETECT_BLK + tid;
    if (row >= M) return;

    double v[FPAD];
    const double2* xr = (const double2*)(X + (size_t)row * FPAD);
#pragma unroll
    for (int f = 0; f < FPAD; f += 2) {
        const double2 x2 = xr[f >> 1];
        v[f] = (x2.x - s_mean[f]) / s_scale[f];
        v[f + 1] = (x2.y - s_mean[f + 1]) / s_scale[f + 1];
    }

    if (has_pca) {
        double t[FPAD];
#pragma unroll
        for (int k = 0; k < FPAD; ++k) t[k] = 0.0;
#pragma unroll
        for (int f = 0; f < FPAD; ++f) {
            if (f < F) {
                const double d = v[f] - s_pmean[f];
#pragma unroll
                for (int k = 0; k < FPAD; ++k)
                    t[k] = t[k] + d * s_W[f * FPAD + k];
            }
        }
#pragma unroll
        for (int k = 0; k < FPAD; ++k) v[k] = t[k];
    }

    uint32_t out[FPAD / 4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int f = 0; f < FPAD; ++f) {
        if (f < F) {
            const float x = (float)v[f];
            const float* c = s_cuts + s_off[f];
            int lo = 0, hi = s_off[f + 1] - s_off[f];
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (c[mid] <= x) lo = mid + 1; else hi = mid;
            }
            out[f >> 2] |= (uint32_t)lo << ((f & 3) * 8);
        }
    }
    *(uint4*)(codes + (size_t)row * FPAD) =
        make_uint4(out[0], out[1], out[2], out[3]);
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

    const uint4 cw = *(const uint4*)(codes + (size_t)row * FPAD);
    const uint64_t c_lo = (uint64_t)cw.x | ((uint64_t)cw.y << 32);
    const uint64_t c_hi = (uint64_t)cw.z | ((uint64_t)cw.w << 32);

    const int t0 = tb * PREDICT_TREE_BLOCK;
    const int t1 = min(n_trees, t0 + PREDICT_TREE_BLOCK);
    double acc0 = 0.0, acc1 = 0.0;
    for (int t = t0; t < t1; ++t) {
        int2 nd = nodes[tree_off[t]];
        while (nd.x < 0) {
            const int f = nd.y & 0xFF;
            const int code =
                (int)(((f & 8 ? c_hi : c_lo) >> ((f & 7) * 8)) & 0xFF);
            nd = nodes[(nd.x & 0x7FFFFFFF) + (code > (nd.y >> 8))];
        }
        const double c0 = (double)__int_as_float(nd.x);
        const double c1 = (double)__int_as_float(nd.y);
        const double tot = c0 + c1;
        acc0 += c0 / tot;
        acc1 += c1 / tot;
    }
    partial[(size_t)tb * M + row] = make_double2(acc0, acc1);
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
