// The per-row steps every saved-detector kernel shares (detect.hip,
// holdout.hip, importance.hip, dependence.hip, similar.hip), gfx950:
// staging a detector's parameters and cuts into LDS, encoding a row,
// walking a packed tree, summing a forest, applying the decision rule.
//
// Bit-parity contract (host side: preprocess.transform_preprocessing,
// models/binning.bin_codes, models/forest_ref.accumulate_proba).  This is
// its one statement; the kernels refer to it.
//   - z[f] = (x[f] - mean[f]) / scale[f]                       (fp64)
//   - t[k] = sum over ascending f of (z[f] - pca_mean[f]) * W[f][k],
//     from 0.0, separate multiply and add — contraction must stay off
//     (the build passes -ffp-contract=off; the pragma below pins it for
//     every file that includes this one, whatever the command line says)
//   - code = #{cut <= (float)value}
//   - per-tree c / (c0 + c1) summed sequentially from 0.0 within blocks of
//     PREDICT_TREE_BLOCK trees, block sums added to 0.0 in ascending order
//   - proba = acc1 / (double)n_trees, the host's single division; the
//     argmax rule is acc1 > acc0 (ties: not flaky).
//
// Packed node (8 bytes, one load per tree level):
//   internal  x = 0x80000000 | id of the left child (global, into the
//                 packed array; the right child is the next record)
//             y = split_bin << 8 | feature
//   leaf      x, y = bit patterns of the fp32 class counts cnt0, cnt1
// Counts are non-negative, so the sign bit of x tells the kinds apart.
//
// Codes: a row's FPAD code bytes, feature f in byte f, are 16 contiguous
// bytes in memory and two 64-bit registers (RowCodes) in a kernel.

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

// One detector's parameters and cuts in LDS: 2432 B of doubles, <= 16320 B
// of cuts and the offset table.  The projection reads them wave-uniformly
// (LDS broadcast).  The struct is 8-aligned, so it ends in 4 B of padding.
struct DetectorLds {
    double mean[FPAD], scale[FPAD], pmean[FPAD];
    double W[FPAD * FPAD];                 // W[f][k]
    float cuts[FPAD * DETECT_MAX_CUTS];    // detector-local, back to back
    int off[FPAD + 1];                     // feature f: off[f] .. off[f + 1]
};

// Called by all DETECT_BLK threads of a block, with the base pointers
// already offset to the block's detector; ends in the barrier.  The caller
// (module.hip) has checked the offsets against DETECT_MAX_CUTS.
__device__ __forceinline__ void stage_detector(
    DetectorLds& s, const double* __restrict__ mean,
    const double* __restrict__ scale, const double* __restrict__ pca_mean,
    const double* __restrict__ W, const float* __restrict__ cuts,
    const int* __restrict__ cut_off) {
    static_assert(DETECT_BLK == FPAD * FPAD, "one thread per entry of W");
    const int tid = threadIdx.x;
    if (tid < FPAD) {
        s.mean[tid] = mean[tid];
        s.scale[tid] = scale[tid];
        s.pmean[tid] = pca_mean[tid];
    }
    if (tid <= FPAD) s.off[tid] = cut_off[tid];
    s.W[tid] = W[tid];
    const int n_cuts = cut_off[FPAD];
    for (int i = tid; i < n_cuts; i += DETECT_BLK) s.cuts[i] = cuts[i];
    __syncthreads();
}

__device__ __forceinline__ double scaled(const DetectorLds& s, int f,
                                         double x) {
    return (x - s.mean[f]) / s.scale[f];
}

// #{cut of feature f <= (float)value}
__device__ __forceinline__ uint32_t cut_code(const DetectorLds& s, int f,
                                             double value) {
    const float x = (float)value;
    const float* c = s.cuts + s.off[f];
    int lo = 0, hi = s.off[f + 1] - s.off[f];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return (uint32_t)lo;
}

struct RowCodes {
    uint64_t lo, hi;                       // features 0..7, 8..15
};

__device__ __forceinline__ RowCodes load_codes(
    const uint8_t* __restrict__ codes /* [M, FPAD] */, size_t row) {
    const uint4 cw = *(const uint4*)(codes + row * FPAD);
    return {(uint64_t)cw.x | ((uint64_t)cw.y << 32),
            (uint64_t)cw.z | ((uint64_t)cw.w << 32)};
}

__device__ __forceinline__ void store_codes(
    uint8_t* __restrict__ codes /* [M, FPAD] */, size_t row, RowCodes c) {
    *(uint4*)(codes + row * FPAD) =
        make_uint4((uint32_t)c.lo, (uint32_t)(c.lo >> 32), (uint32_t)c.hi,
                   (uint32_t)(c.hi >> 32));
}

__device__ __forceinline__ int code_of(RowCodes c, int f) {
    return (int)(((f & 8 ? c.hi : c.lo) >> ((f & 7) * 8)) & 0xFF);
}

// c with feature f's byte replaced by code
__device__ __forceinline__ RowCodes with_code(RowCodes c, int f,
                                              uint64_t code) {
    const int sh = (f & 7) * 8;
    const uint64_t keep = ~(0xFFull << sh);
    if (f & 8) c.hi = (c.hi & keep) | code << sh;
    else c.lo = (c.lo & keep) | code << sh;
    return c;
}

__device__ __forceinline__ bool same_codes(RowCodes a, RowCodes b) {
    return a.lo == b.lo && a.hi == b.hi;
}

// The codes of the first F of a row's values (scaled, or projected).
__device__ __forceinline__ RowCodes search_codes(const DetectorLds& s,
                                                 const double* v, int F) {
    RowCodes c = {0, 0};
#pragma unroll
    for (int f = 0; f < FPAD; ++f)
        if (f < F) c = with_code(c, f, cut_code(s, f, v[f]));
    return c;
}

// Scale, optionally project, cast, search, pack: one raw row to its codes.
__device__ __forceinline__ RowCodes encode_row(
    const DetectorLds& s, const double* __restrict__ x /* [FPAD] */,
    int has_pca, int F) {
    double v[FPAD];
    const double2* xr = (const double2*)x;
#pragma unroll
    for (int f = 0; f < FPAD; f += 2) {
        const double2 x2 = xr[f >> 1];
        v[f] = scaled(s, f, x2.x);
        v[f + 1] = scaled(s, f + 1, x2.y);
    }
    if (has_pca) {
        double t[FPAD];
#pragma unroll
        for (int k = 0; k < FPAD; ++k) t[k] = 0.0;
#pragma unroll
        for (int f = 0; f < FPAD; ++f) {
            if (f < F) {
                const double d = v[f] - s.pmean[f];
#pragma unroll
                for (int k = 0; k < FPAD; ++k)
                    t[k] = t[k] + d * s.W[f * FPAD + k];
            }
        }
#pragma unroll
        for (int k = 0; k < FPAD; ++k) v[k] = t[k];
    }
    return search_codes(s, v, F);
}

// Walks the tree rooted at record `root` to the row's leaf: one 8-byte
// load per level.  Returns the leaf record and its id.
__device__ __forceinline__ int2 tree_leaf(const int2* __restrict__ nodes,
                                          long root, RowCodes c, int& id) {
    id = (int)root;
    int2 nd = nodes[root];
    while (nd.x < 0) {
        id = (nd.x & 0x7FFFFFFF) + (code_of(c, nd.y & 0xFF) > (nd.y >> 8));
        nd = nodes[id];
    }
    return nd;
}

__device__ __forceinline__ int2 tree_leaf(const int2* __restrict__ nodes,
                                          long root, RowCodes c) {
    int id;
    return tree_leaf(nodes, root, c, id);
}

// (acc0, acc1) over tree block tb: trees tb * PREDICT_TREE_BLOCK .. of the
// forest whose root ids start at roots[0], summed sequentially from 0.0.
__device__ __forceinline__ double2 tree_block_sums(
    const int2* __restrict__ nodes, const long* __restrict__ roots, int tb,
    int n_trees, RowCodes c) {
    const int t0 = tb * PREDICT_TREE_BLOCK;
    const int t1 = min(n_trees, t0 + PREDICT_TREE_BLOCK);
    double acc0 = 0.0, acc1 = 0.0;
    for (int t = t0; t < t1; ++t) {
        const int2 nd = tree_leaf(nodes, roots[t], c);
        const double c0 = (double)__int_as_float(nd.x);
        const double c1 = (double)__int_as_float(nd.y);
        const double tot = c0 + c1;
        acc0 += c0 / tot;
        acc1 += c1 / tot;
    }
    return make_double2(acc0, acc1);
}

// (acc0, acc1) over the whole forest: the block sums added to 0.0 in
// ascending order.
__device__ __forceinline__ double2 forest_sums(
    const int2* __restrict__ nodes, const long* __restrict__ roots,
    int n_trees, int n_blocks, RowCodes c) {
    double tot0 = 0.0, tot1 = 0.0;
    for (int tb = 0; tb < n_blocks; ++tb) {
        const double2 p = tree_block_sums(nodes, roots, tb, n_trees, c);
        tot0 += p.x;
        tot1 += p.y;
    }
    return make_double2(tot0, tot1);
}

// threshold < 0: the argmax rule; otherwise proba >= threshold.
__device__ __forceinline__ bool predicted(double2 acc, int n_trees,
                                          double threshold) {
    return threshold < 0.0 ? acc.y > acc.x
                           : acc.y / (double)n_trees >= threshold;
}
