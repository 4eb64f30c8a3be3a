// Forest proximity for a saved detector (engine/similar.py), gfx950.
//
//   forest_leaves_kernel    the tree walk of detector_steps.h, one
//                           thread per (row, tree); writes the tree-local
//                           canonical id of the leaf reached
//   prox_wide_kernel        raises a flag if an id does not fit 16 bits
//   prox_pack_kernel        row-major int32 ids -> the internal layout
//   proximity_topk_kernel   per (query, corpus chunk) the first k corpus
//                           rows under (larger shared, lower index)
//   proximity_merge_kernel  the chunks' lists merged under the same order
//
// Every value is an integer and the order is total, so the result does not
// depend on the tiling, on the chunking or on the merge; the numpy form is
// engine/similar.py (backend="ref").  No atomics, no waiting on other
// workgroups, plain stores only.
//
// Internal layout.  A row of T ids becomes W dwords: two 16-bit ids per
// dword when every id of both matrices fits 16 bits (PACKED), one id per
// dword otherwise; W is padded with zero ids to a multiple of PROX_D, on
// both sides, so padding always compares equal and shared = T - mismatches.
// The corpus is stored [N, W]: a tile of PROX_TILE rows is staged into LDS
// and read back wave-uniformly (ds_read_b128, all lanes one address: a
// broadcast, no bank conflict).  The queries are stored transposed [W, M]:
// each lane owns one query and loads PROX_D dwords of it into registers
// with lane-consecutive addresses.
//
// Cost per corpus dword and lane: PACKED xor + packed min(.,1) + packed add
// = 3 VALU for two comparisons; full width compare + add-with-carry.  One
// 16-byte LDS broadcast feeds 12 VALU instructions of each wave, so the
// VALU issue rate is the bound, not the LDS read rate.
//
// Rows with more than PROX_D dwords are compared PROX_D dwords at a time:
// between the pieces a lane parks its running mismatch counts of the tile's
// rows in LDS (a slot only that lane touches).

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detector_steps.h"

#define PROX_BLK 256      // lanes = queries per workgroup
#define PROX_D 52         // dwords of a row compared per piece (registers)
#define PROX_TILE 32      // corpus rows per LDS tile
#define PROX_CHUNK 512    // least corpus rows per workgroup
#define PROX_MAX_K 16
#define PROX_MAX_T 65535  // parked counts are 16-bit

// One thread per (row, tree), rows fastest so a wave walks one tree.
__global__ __launch_bounds__(DETECT_BLK) void forest_leaves_kernel(
    const uint8_t* __restrict__ codes,     // [M, FPAD]
    const long* __restrict__ tree_off,     // [T + 1] root ids
    const int2* __restrict__ nodes,        // packed records
    int M, int n_trees,
    int* __restrict__ leaf /* [M, T] */) {
    const long idx = (long)blockIdx.x * DETECT_BLK + threadIdx.x;
    if (idx >= (long)M * n_trees) return;
    const int row = (int)(idx % M);
    const int t = (int)(idx / M);
    const int root = (int)tree_off[t];
    int id;
    tree_leaf(nodes, root, load_codes(codes, row), id);
    leaf[(size_t)row * n_trees + t] = id - root;
}

// flag[0] = 1 if any of the n ids is outside 0..65535.  Every writer
// stores the same value, so the plain store needs no ordering.
__global__ __launch_bounds__(PROX_BLK) void prox_wide_kernel(
    const int* __restrict__ ids, long n, int* __restrict__ flag) {
    const long stride = (long)gridDim.x * PROX_BLK;
    bool wide = false;
    for (long i = (long)blockIdx.x * PROX_BLK + threadIdx.x; i < n;
         i += stride)
        wide |= ((uint32_t)ids[i] >> 16) != 0u;
    if (wide) flag[0] = 1;
}

// out[r * sr + w * sw] = dword w of row r, w < W.  The corpus uses
// (sr, sw) = (W, 1), the queries (1, rows).  One thread per output dword,
// w fastest.
template <bool PACKED>
__global__ __launch_bounds__(PROX_BLK) void prox_pack_kernel(
    const int* __restrict__ ids,           // [rows, T]
    long rows, int T, int W, long sr, long sw,
    uint32_t* __restrict__ out) {
    const long i = (long)blockIdx.x * PROX_BLK + threadIdx.x;
    if (i >= rows * W) return;
    const long r = i / W;
    const int w = (int)(i % W);
    const int* src = ids + (size_t)r * T;
    uint32_t v = 0u;
    if (PACKED) {
        const int t = 2 * w;
        if (t < T) v = (uint32_t)src[t] & 0xFFFFu;
        if (t + 1 < T) v |= (uint32_t)src[t + 1] << 16;
    } else if (w < T) {
        v = (uint32_t)src[w];
    }
    out[(size_t)r * sr + (size_t)w * sw] = v;
}

// A sorted list of the K best (shared, idx) seen so far.  Candidates
// arrive in ascending idx, so a candidate never goes ahead of an entry
// with an equal count: the strict comparison IS the tie rule.  Empty
// slots hold shared = -1, below every real count.
template <int K>
struct ProxList {
    int sh[K], id[K];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < K; ++j) { sh[j] = -1; id[j] = -1; }
    }

    __device__ __forceinline__ void offer(int c, int i) {
        if (c <= sh[K - 1]) return;
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
            const bool above = j > 0 && c > sh[j > 0 ? j - 1 : 0];
            const bool here = !above && c > sh[j];
            const int psh = sh[j > 0 ? j - 1 : 0];
            const int pid = id[j > 0 ? j - 1 : 0];
            sh[j] = above ? psh : (here ? c : sh[j]);
            id[j] = above ? pid : (here ? i : id[j]);
        }
    }

    // the first k entries, `step` ints apart; an empty slot leaves as
    // (-1, 0)
    __device__ __forceinline__ void store(int* __restrict__ o_idx,
                                          int* __restrict__ o_sh, int k,
                                          size_t step) const {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) {
                o_idx[j * step] = id[j];
                o_sh[j * step] = sh[j] < 0 ? 0 : sh[j];
            }
    }
};

typedef unsigned short prox_u16x2 __attribute__((ext_vector_type(2)));

// Mismatching ids between one query dword and one corpus dword, added to
// acc: PACKED keeps two 16-bit counters (one per half, each <= PROX_D per
// piece), full width one counter.
template <bool PACKED>
__device__ __forceinline__ uint32_t prox_acc(uint32_t acc, uint32_t q,
                                             uint32_t c) {
    if (PACKED) {
        // Written as min(x, 1) in C++ the compiler turns each half into a
        // compare, a select and a repack (7 VALU per dword); the packed
        // minimum is one register-only instruction, so it is named here.
        uint32_t m;
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(m) : "v"(q ^ c),
            "v"(0x00010001u));
        return __builtin_bit_cast(
            uint32_t, (prox_u16x2)(__builtin_bit_cast(prox_u16x2, acc) +
                                   __builtin_bit_cast(prox_u16x2, m)));
    }
    return acc + (q != c ? 1u : 0u);
}

// grid = (query blocks, corpus chunks).  Lane q of block b owns query
// b * PROX_BLK + q and the corpus rows chunk * chunk_rows ... of its
// blockIdx.y.  With one chunk it writes its list to the outputs [M, k];
// with more, to the partial arrays [n_chunks, k, M], whose stores and
// loads (proximity_merge_kernel) are lane-consecutive.
// 4 waves per SIMD: K = 16 then fits 128 registers without scratch.
template <int K, bool PACKED>
__global__ __launch_bounds__(PROX_BLK, 4) void proximity_topk_kernel(
    const uint32_t* __restrict__ qT,       // [W, M]
    const uint32_t* __restrict__ cP,       // [N, W]
    const int* __restrict__ self_idx,      // [M]
    int M, int N, int T, int W, int chunk_rows, int k,
    int* __restrict__ out_idx,             // [M, k] or [n_chunks, k, M]
    int* __restrict__ out_sh) {
    __shared__ uint4 s_tile[PROX_TILE * (PROX_D / 4)];
    __shared__ unsigned short s_cnt[PROX_TILE * PROX_BLK];

    const int tid = threadIdx.x;
    const int query = blockIdx.x * PROX_BLK + tid;
    const bool live = query < M;
    const int qld = live ? query : M - 1;          // loads stay in range
    const int self = self_idx[qld];
    const int n_pieces = W / PROX_D;
    const int row0 = (int)((long)blockIdx.y * chunk_rows);  // < N by the grid
    const int row1 = (int)min((long)N, (long)row0 + chunk_rows);

    ProxList<K> best;
    best.clear();

    uint32_t qreg[PROX_D];
    for (int base = row0; base < row1; base += PROX_TILE) {
        const int rows = min(PROX_TILE, row1 - base);
        for (int p = 0; p < n_pieces; ++p) {
            __syncthreads();                       // the last tile is read
            for (int i = tid; i < rows * (PROX_D / 4); i += PROX_BLK) {
                const int r = i / (PROX_D / 4), d4 = i % (PROX_D / 4);
                s_tile[i] = *(const uint4*)(
                    cP + (size_t)(base + r) * W + p * PROX_D + 4 * d4);
            }
            if (n_pieces > 1 || base == row0) {
#pragma unroll
                for (int d = 0; d < PROX_D; ++d)
                    qreg[d] = qT[(size_t)(p * PROX_D + d) * M + qld];
            }
            __syncthreads();

            for (int r = 0; r < rows; ++r) {
                const uint4* row = s_tile + r * (PROX_D / 4);
                // PACKED: four independent chains; a 16-bit counter
                // holds at most PROX_D, so the plain sum carries nothing
                // across.  Full width keeps one chain: four would hold
                // four compare masks at a time and spill scalar registers.
                uint32_t a[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int d4 = 0; d4 < PROX_D / 4; ++d4) {
                    const uint4 c = row[d4];
                    const uint32_t cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        uint32_t& dst = a[PACKED ? e : 0];
                        dst = prox_acc<PACKED>(dst, qreg[4 * d4 + e], cv[e]);
                    }
                }
                const uint32_t acc = (a[0] + a[1]) + (a[2] + a[3]);
                int mism = PACKED ? (int)((acc & 0xFFFFu) + (acc >> 16))
                                  : (int)acc;
                if (n_pieces > 1) {
                    if (p > 0) mism += s_cnt[r * PROX_BLK + tid];
                    if (p + 1 < n_pieces) {
                        s_cnt[r * PROX_BLK + tid] = (unsigned short)mism;
                        continue;
                    }
                }
                const int cand = base + r;
                best.offer(cand == self ? -1 : T - mism, cand);
            }
        }
    }
    if (!live) return;
    if (gridDim.y == 1) {
        best.store(out_idx + (size_t)query * k, out_sh + (size_t)query * k,
                   k, 1);
    } else {
        const size_t slot = (size_t)blockIdx.y * k * M + query;
        best.store(out_idx + slot, out_sh + slot, k, (size_t)M);
    }
}

// One thread per query: the chunks' lists in ascending chunk order, each
// in its own order, offered to one list.  That is ascending idx among
// equal counts, which ProxList::offer relies on.
template <int K>
__global__ __launch_bounds__(PROX_BLK) void proximity_merge_kernel(
    const int* __restrict__ part_idx,      // [n_chunks, k, M]
    const int* __restrict__ part_sh,
    int M, int n_chunks, int k,
    int* __restrict__ out_idx,             // [M, k]
    int* __restrict__ out_sh) {
    const int query = blockIdx.x * PROX_BLK + threadIdx.x;
    if (query >= M) return;
    ProxList<K> best;
    best.clear();
    for (int e = 0; e < n_chunks * k; ++e) {
        const size_t at = (size_t)e * M + query;
        const int i = part_idx[at];
        if (i >= 0) best.offer(part_sh[at], i);
    }
    best.store(out_idx + (size_t)query * k, out_sh + (size_t)query * k, k,
               1);
}
