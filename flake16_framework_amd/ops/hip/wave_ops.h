// Wave-level primitives that stay in registers (gfx9 / CDNA DPP).
//
// The subtree builders reduce and broadcast small values many times per
// tree node.  __shfl* lowers to ds_bpermute_b32 — an LDS round trip with a
// full lgkmcnt wait per step — so a 6-step butterfly costs six dependent
// LDS latencies.  The helpers here use DPP row shifts / row broadcasts and
// v_readlane instead: pure VALU, no memory counter.
//
// EVERY primitive assumes a FULLY ACTIVE 64-lane wave (EXEC all ones):
// DPP reads of inactive lanes are undefined.  All call sites are
// wave-uniform code of the forest kernels (forest.hip) and of the
// partial-dependence kernel (dependence.hip).
//
// Reduction shape (wave_reduce): row_shr:1,2,4,8 leave each 16-lane row's
// reduction in its lane 15; row_bcast:15 folds row 0 into row 1 and row 2
// into row 3; row_bcast:31 folds lane 31 into rows 2-3; lane 63 then holds
// the reduction over all 64 lanes and is read back with v_readlane, so the
// result is wave-uniform (an SGPR).  update_dpp is called with old = v:
// a lane whose DPP source does not exist combines with itself.  Only lane
// 63 is read, and every value on lane 63's dependency chain came from a
// lane that had a source, so this is exact for non-idempotent operators
// (sum) too.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "philox.h"

#define WAVE_DPP_ROW_SHR1 0x111
#define WAVE_DPP_ROW_SHR2 0x112
#define WAVE_DPP_ROW_SHR4 0x114
#define WAVE_DPP_ROW_SHR8 0x118
#define WAVE_DPP_ROW_BCAST15 0x142
#define WAVE_DPP_ROW_BCAST31 0x143

template <int CTRL>
__device__ __forceinline__ int wave_dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}

// v_readlane with a wave-uniform lane: replaces __shfl(x, uniform).
__device__ __forceinline__ int wave_bcast(int v, int lane) {
    return __builtin_amdgcn_readlane(v, lane);
}
__device__ __forceinline__ uint32_t wave_bcast(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

template <class Op>
__device__ __forceinline__ int wave_reduce(int v, Op op) {
    v = op(v, wave_dpp_i32<WAVE_DPP_ROW_SHR1>(v));
    v = op(v, wave_dpp_i32<WAVE_DPP_ROW_SHR2>(v));
    v = op(v, wave_dpp_i32<WAVE_DPP_ROW_SHR4>(v));
    v = op(v, wave_dpp_i32<WAVE_DPP_ROW_SHR8>(v));
    v = op(v, wave_dpp_i32<WAVE_DPP_ROW_BCAST15>(v));
    v = op(v, wave_dpp_i32<WAVE_DPP_ROW_BCAST31>(v));
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
    return wave_reduce(v, [](int a, int b) { return a + b; });
}
__device__ __forceinline__ int wave_min_i32(int v) {
    return wave_reduce(v, [](int a, int b) { return a < b ? a : b; });
}
__device__ __forceinline__ int wave_max_i32(int v) {
    return wave_reduce(v, [](int a, int b) { return a > b ? a : b; });
}

// fp64 sum of one value per lane with a PINNED association, wave-uniform.
// The double travels as two 32-bit DPP moves (as in wave_argmax_step).
//
// The result is bit for bit the pairwise tree
//     v = v[0::2] + v[1::2]      six times over v[0..63], result v[0]
// that numpy evaluates (engine/dependence.py).  Follow lane 63's
// dependency chain, writing T_k[i] for the sum over lanes i-2^k+1 .. i:
//   row_shr:1    lane 2i+1  = own v[2i+1] + lower v[2i]        tree level 1
//   row_shr:2    lane 4i+3  = own T_1[4i+3] + lower T_1[4i+1]  level 2
//   row_shr:4    lane 8i+7  = own T_2[8i+7] + lower T_2[8i+3]  level 3
//   row_shr:8    lane 16i+15 = own T_3 + lower T_3[16i+7]      level 4
//   row_bcast:15 lanes 31, 63 = own T_4 + lane 15 / 47's T_4   level 5
//   row_bcast:31 lane 63 = own T_5[63] + lane 31's T_5         level 6
// so every add on the chain joins the two adjacent aligned halves of a
// tree node, upper half as the first operand: `own + lower`, where numpy
// adds `lower + upper`.  IEEE fp64 addition of non-NaN values is
// commutative, so the two have the same bits.  Lanes off the chain (those
// without a DPP source add their own value, old = v) are never read.
template <int CTRL>
__device__ __forceinline__ double wave_dpp_f64(double v) {
    return __hiloint2double(wave_dpp_i32<CTRL>(__double2hiint(v)),
                            wave_dpp_i32<CTRL>(__double2loint(v)));
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    v = v + wave_dpp_f64<WAVE_DPP_ROW_SHR1>(v);
    v = v + wave_dpp_f64<WAVE_DPP_ROW_SHR2>(v);
    v = v + wave_dpp_f64<WAVE_DPP_ROW_SHR4>(v);
    v = v + wave_dpp_f64<WAVE_DPP_ROW_SHR8>(v);
    v = v + wave_dpp_f64<WAVE_DPP_ROW_BCAST15>(v);
    v = v + wave_dpp_f64<WAVE_DPP_ROW_BCAST31>(v);
    return __hiloint2double(
        __builtin_amdgcn_readlane(__double2hiint(v), 63),
        __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// Inclusive prefix sum over the 64 lanes (lane i gets v_0 + ... + v_i).
// Lanes without a DPP source, and rows masked off, add old = 0: row_shr
// 1/2/4/8 scan each 16-lane row, row_bcast:15 adds the total of row 0 to
// row 1 and of row 2 to row 3 (row_mask 0xA), row_bcast:31 adds the total
// of rows 0-1 to rows 2-3 (row_mask 0xC).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int wave_dpp_or0_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ int wave_scan_incl_i32(int v) {
    v += wave_dpp_or0_i32<WAVE_DPP_ROW_SHR1, 0xF>(v);
    v += wave_dpp_or0_i32<WAVE_DPP_ROW_SHR2, 0xF>(v);
    v += wave_dpp_or0_i32<WAVE_DPP_ROW_SHR4, 0xF>(v);
    v += wave_dpp_or0_i32<WAVE_DPP_ROW_SHR8, 0xF>(v);
    v += wave_dpp_or0_i32<WAVE_DPP_ROW_BCAST15, 0xA>(v);
    v += wave_dpp_or0_i32<WAVE_DPP_ROW_BCAST31, 0xC>(v);
    return v;
}

// Two independent u16 lanes per dword (v_pk_min_u16 / v_pk_max_u16).
typedef uint16_t wave_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pkmin_u16x2(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(
        __builtin_bit_cast(wave_u16x2, a), __builtin_bit_cast(wave_u16x2, b)));
}
__device__ __forceinline__ uint32_t pkmax_u16x2(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(
        __builtin_bit_cast(wave_u16x2, a), __builtin_bit_cast(wave_u16x2, b)));
}
__device__ __forceinline__ uint32_t wave_pkmin_u16x2(uint32_t v) {
    return (uint32_t)wave_reduce((int)v, [](int a, int b) {
        return (int)pkmin_u16x2((uint32_t)a, (uint32_t)b);
    });
}
__device__ __forceinline__ uint32_t wave_pkmax_u16x2(uint32_t v) {
    return (uint32_t)wave_reduce((int)v, [](int a, int b) {
        return (int)pkmax_u16x2((uint32_t)a, (uint32_t)b);
    });
}

// Argmax over (fp64 score, bin, left count) triples, one per lane; the
// winning triple is returned wave-uniform in (s, b, nl).
//
// Both comparators are total orders over the values that occur, so the
// selected triple does not depend on the order in which lanes are combined
// (the DPP tree combines in a different order than the __shfl_down tree
// it replaces):
//   mid   other wins if  os > s || (os == s && ob != -1 && (b == -1 || ob < b))
//         invalid entries are (-1.0, -1); valid scores are positive with
//         bin >= 0, so among equal scores both are valid (lower bin wins)
//         or both invalid (identical).
//   small other wins if  os > s || (os == s && ob < b)
//         invalid entries are (-1e300, INT_MAX); valid scores are positive
//         with bin <= 255.
// Equal (score, bin) pairs come from the same threshold and carry the same
// left count, so which copy survives is immaterial.
// The double travels as two 32-bit DPP moves.
struct ArgmaxMidCmp {
    __device__ __forceinline__ bool operator()(double os, int ob, double s,
                                               int b) const {
        return os > s || (os == s && ob != -1 && (b == -1 || ob < b));
    }
};
struct ArgmaxSmallCmp {
    __device__ __forceinline__ bool operator()(double os, int ob, double s,
                                               int b) const {
        return os > s || (os == s && ob < b);
    }
};

template <int CTRL, class Cmp>
__device__ __forceinline__ void wave_argmax_step(double& s, int& b, int& nl,
                                                 Cmp other_wins) {
    const int lo = __double2loint(s), hi = __double2hiint(s);
    const double os = __hiloint2double(wave_dpp_i32<CTRL>(hi),
                                       wave_dpp_i32<CTRL>(lo));
    const int ob = wave_dpp_i32<CTRL>(b);
    const int onl = wave_dpp_i32<CTRL>(nl);
    if (other_wins(os, ob, s, b)) { s = os; b = ob; nl = onl; }
}

template <class Cmp>
__device__ __forceinline__ void wave_argmax(double& s, int& b, int& nl,
                                            Cmp cmp) {
    wave_argmax_step<WAVE_DPP_ROW_SHR1>(s, b, nl, cmp);
    wave_argmax_step<WAVE_DPP_ROW_SHR2>(s, b, nl, cmp);
    wave_argmax_step<WAVE_DPP_ROW_SHR4>(s, b, nl, cmp);
    wave_argmax_step<WAVE_DPP_ROW_SHR8>(s, b, nl, cmp);
    wave_argmax_step<WAVE_DPP_ROW_BCAST15>(s, b, nl, cmp);
    wave_argmax_step<WAVE_DPP_ROW_BCAST31>(s, b, nl, cmp);
    const int lo = __builtin_amdgcn_readlane(__double2loint(s), 63);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(s), 63);
    s = __hiloint2double(hi, lo);
    b = __builtin_amdgcn_readlane(b, 63);
    nl = __builtin_amdgcn_readlane(nl, 63);
}
__device__ __forceinline__ void wave_argmax_mid(double& s, int& b, int& nl) {
    wave_argmax(s, b, nl, ArgmaxMidCmp());
}
__device__ __forceinline__ void wave_argmax_small(double& s, int& b, int& nl) {
    wave_argmax(s, b, nl, ArgmaxSmallCmp());
}

// Fisher-Yates feature permutation in one 64-bit register of sixteen 4-bit
// entries: perm[k] = (P >> 4*k) & 15.  u_mine is lane i's FEATSEL draw
// (lanes >= F - 1 are ignored).  Lane i < F-1 computes its own swap target
// j_i = i + bounded(u_i, F - i) — a draw does not depend on the swaps
// before it — and the swaps then run wave-uniformly on j_i fetched with
// v_readlane.  No LDS, no lane-0 section; F = 1 does no swap.  The swap
// sequence is exactly forest_ref's, so the permutation is identical.
__device__ __forceinline__ uint64_t feature_perm(uint32_t u_mine, int F) {
    const int lane = threadIdx.x & 63;
    int j_mine = lane;
    if (lane < F - 1)
        j_mine = lane + (int)philox_bounded(u_mine, (uint32_t)(F - lane));
    uint64_t P = 0xFEDCBA9876543210ULL;
    for (int i = 0; i < F - 1; ++i) {
        const int j = __builtin_amdgcn_readlane(j_mine, i);
        const uint64_t x = ((P >> (4 * i)) ^ (P >> (4 * j))) & 15ULL;
        P ^= (x << (4 * i)) ^ (x << (4 * j));
    }
    return P;
}

__device__ __forceinline__ int perm_at(uint64_t P, int k) {
    return (int)((P >> (4 * k)) & 15ULL);
}
