// Batched histogram-forest construction for MI355X (gfx950).
//
// One forest_fit call builds ALL trees of one grid cell (10 folds x
// n_estimators jobs) device-resident.  Work is tiered by node size:
//   > 2048 samples   level-synchronous work queue, one 256-thread
//                    workgroup per node, packed 16-bit LDS histograms
//                    (hist_split_kernel; a WIDE unpacked instantiation
//                    covers nodes >= 2^16) with parent-minus-smaller-child
//                    histogram-subtraction pools; Extra-Trees jobs use the
//                    histogram-free two-pass et_split_kernel instead
//   65..2048         mid_subtree_kernel: the block stages the node's code
//                    rows into LDS once and finishes the whole subtree
//                    internally (LDS histograms + LDS index partitions)
//   <= 64            small_subtree_kernel: one 64-lane wave finishes the
//                    subtree from register-resident samples with
//                    ballot/popcount counting
// Only the first tier is level-synchronous.  Mid and small subtrees are
// terminal, so the split kernels just append them to two queues that
// accumulate over the whole fit, each item tagged with the sample buffer
// (sidx_a / sidx_b) its range was partitioned into; the host launches
// mid_subtree_kernel then small_subtree_kernel once after the band is
// exhausted (mid first: it farms its <= 64 descendants into the small
// queue), or earlier if a queue passes its drain threshold.
// Split selection is fp64 (file compiled -ffp-contract=off) and all
// randomness is Philox keyed on (tag, node sample-range, draw), so trees
// are bit-identical to the numpy reference in models/forest_ref.py no
// matter how the device schedules the work.
//
// All tiers build a node from the same steps — node draws, fp64 split
// score, best bin of a histogram row, select in permutation order, commit,
// stable partition — and each step is written once, in the "Shared node
// steps" section above the kernels.  A change to a step belongs there.
//
// Reference semantics being implemented: sklearn 1.0.2 defaults for
// DecisionTree/RandomForest/ExtraTrees (see models/forest_ref.py docstring;
// reference experiment.py:96-98, 469, 473).

#include <hip/hip_runtime.h>
#include <cstdint>

#include "philox.h"
#include "wave_ops.h"

#define HBLK 256
#define FPAD 16          // codes row stride (bytes); F <= 16
#define LEAF_SENTINEL (-1)

struct WorkItem {
    int job;
    int node;       // job-local node id
    int start;      // job-local sidx range [start, end)
    int end;
    int depth;
    // Level-queue items: precomputed-histogram slot in pool[depth&1], or
    // -1.  Mid/small-queue items never carry a slot (route_child), so the
    // field holds their sample-buffer tag instead: 0 = sidx_a, 1 = sidx_b.
    int hist_slot;
};

struct ForestDev {
    const uint8_t* __restrict__ codes;    // [R, FPAD]
    const uint8_t* __restrict__ labels;   // [R]
    const int* __restrict__ j_row_off;    // [J] fold data base row
    const int* __restrict__ j_n;          // [J] samples per job
    const long* __restrict__ j_sidx_off;  // [J] base into sidx buffers
    const long* __restrict__ j_node_off;  // [J] base into node arrays
    const int* __restrict__ j_key;        // [J] philox k1 per job
    int* __restrict__ node_alloc;         // [J]
    int* __restrict__ nfeat;              // per node (LEAF_SENTINEL = leaf)
    int* __restrict__ nsplit;
    int* __restrict__ nleft;              // left child id; right = left + 1
    float* __restrict__ ncnt0;
    float* __restrict__ ncnt1;
    const int* __restrict__ sidx_cur;
    int* __restrict__ sidx_nxt;
    // Both sample-index buffers by tag: deferred mid/small items outlive
    // the level that routed them and name their buffer explicitly.
    int* sidx_a;
    int* sidx_b;
    const WorkItem* __restrict__ cur;
    const int* __restrict__ cur_count;
    WorkItem* __restrict__ nxt;
    int* __restrict__ nxt_count;
    int* __restrict__ err_flag;
    int F;
    // Per-job model spec (a fused fit batches a balance group's three
    // model cells: DT + RF + ET jobs in one build).
    const int* __restrict__ j_mf;        // [J] max_features
    const uint8_t* __restrict__ j_rand;  // [J] splitter: 1 = random (ET)
    uint32_t seed;
    int work_cap;
    // Histogram-subtraction pools: a splitting node >= hist_save_min
    // samples accumulates its SMALLER child's histogram itself and derives
    // the larger child's by subtraction (exact integer counts); both are
    // stored in pool[(depth+1)&1] and the children skip accumulation.
    uint32_t* __restrict__ hist_pool0;
    uint32_t* __restrict__ hist_pool1;
    int* __restrict__ pool_count;   // strided level-state slots (see host)
    int pool_cap;
    int hist_save_min;
    // Small-subtree routing: children with n <= SMALL_N go to this queue
    // and are finished wholesale by small_subtree_kernel (one wave builds
    // the whole subtree from register-resident samples).  small_count and
    // mid_count are fixed slots that accumulate over the whole fit; the
    // host drains and resets them (see forest_fit_impl).
    WorkItem* __restrict__ small;
    int* __restrict__ small_count;
    int small_cap;
    // Mid-subtree routing: children with SMALL_N < n <= MID_N are staged
    // into LDS by mid_subtree_kernel, which recurses internally (no level
    // round-trips) and farms its <=SMALL_N descendants to the small queue.
    WorkItem* __restrict__ mid;
    int* __restrict__ mid_count;
    int mid_cap;
    // mid_subtree_kernel mode: wave-parallel node processing (4 nodes in
    // flight per block) when max_features <= WAVE_CANDS; 0 = block-serial
    // DFS (DT, or FLAKE16_NO_WAVE_MID=1 for A/B runs).
    int wave_mid;
};

#define SMALL_N 64
#define MID_N 2048

// Three-way child routing: <=SMALL_N -> wave-subtree queue, <=MID_N ->
// LDS-staged mid-subtree queue, else next level.  Called by one thread.
// A split kernel partitions depth-d children into the buffer of parity
// d & 1 (root level 0 reads sidx_a), and no later level writes inside a
// deferred child's [start, end) — every partition stays inside the
// splitting node's own range and a job's node ranges are disjoint — so
// the tagged item stays valid until the host drains the queue.
__device__ __forceinline__ void route_child(const ForestDev& a,
                                            const WorkItem& w) {
    const int n = w.end - w.start;
    if (n <= SMALL_N) {
        const int i = atomicAdd(a.small_count, 1);
        if (i < a.small_cap)
            a.small[i] = {w.job, w.node, w.start, w.end, w.depth,
                          w.depth & 1};
        else atomicExch(a.err_flag, 1);
    } else if (n <= MID_N && w.hist_slot < 0) {
        const int i = atomicAdd(a.mid_count, 1);
        if (i < a.mid_cap)
            a.mid[i] = {w.job, w.node, w.start, w.end, w.depth,
                        w.depth & 1};
        else atomicExch(a.err_flag, 1);
    } else {
        const int i = atomicAdd(a.nxt_count, 1);
        if (i < a.work_cap) a.nxt[i] = w;
        else atomicExch(a.err_flag, 1);
    }
}

// ===========================================================================
// Shared node steps.
//
// The single copy of each step every tier runs to build a node.  Bit-parity
// with models/forest_ref.py rests on these: the operand order of
// split_score, the Philox counters, the lowest-bin and first-candidate tie
// rules, and the stable partition arithmetic.  The wave-level steps assume
// a fully active 64-lane wave in wave-uniform control flow (wave_ops.h).
// ===========================================================================

// Code of feature f from a 16-byte row.  Selects instead of indexing: a
// dynamically indexed private array is promoted to LDS (or scratch) by
// the compiler, which puts a store + load round trip on every sample.
__device__ __forceinline__ uint32_t code_byte(const uint4& cw, int f) {
    const int k = f >> 2;
    const uint32_t w = k == 0 ? cw.x : k == 1 ? cw.y : k == 2 ? cw.z : cw.w;
    return (w >> ((f & 3) * 8)) & 0xFFu;
}

// Packed histogram word -> (total, class-1) counts.
__device__ __forceinline__ uint2 unpack_counts(uint32_t v) {
    return uint2{v & 0xFFFFu, v >> 16};
}

// Sum of v over the block's 256 threads, returned to every thread.
__device__ __forceinline__ int block_sum_i32(int v, int* sh_wsum) {
    v = wave_sum_i32(v);
    if ((threadIdx.x & 63) == 0) sh_wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    const int t = sh_wsum[0] + sh_wsum[1] + sh_wsum[2] + sh_wsum[3];
    __syncthreads();
    return t;
}

// Split score of a node (n samples, c0 / c1 per class) whose left child
// takes nL samples, n1L of them class 1.  fp64 with integer operands; the
// operand order is forest_ref's (file compiled -ffp-contract=off).  The
// caller makes sure neither child is empty.
__device__ __forceinline__ double split_score(long nL, long n1L, int n,
                                              int c0, int c1) {
    const long n0L = nL - n1L, nR = n - nL;
    const long n1R = c1 - n1L, n0R = c0 - n0L;
    return (double)(n0L * n0L + n1L * n1L) / (double)nL
         + (double)(n0R * n0R + n1R * n1R) / (double)nR;
}

// The two per-node Philox draws, keyed on the node's job-relative sample
// range [s, e) and depth: lane i < FPAD holds draw i (the other lanes
// repeat draw 0 and are never read).
__device__ __forceinline__ uint32_t node_draws(
    uint32_t tag, const ForestDev& a, uint32_t key, int depth, int s, int e) {
    const int lane = threadIdx.x & 63;
    return philox_draw(tag | ((uint32_t)(depth & 0xFF) << 8), (uint32_t)s,
                       (uint32_t)e, (uint32_t)(lane < FPAD ? lane : 0),
                       a.seed, key);
}
// Feature permutation of the node (partial Fisher-Yates, wave_ops.h).
__device__ __forceinline__ uint64_t featsel_perm(
    const ForestDev& a, uint32_t key, int depth, int s, int e) {
    return feature_perm(node_draws(TAG_FEATSEL, a, key, depth, s, e), a.F);
}
// Extra-Trees threshold draws: lane f holds feature f's.
__device__ __forceinline__ uint32_t thresh_draws(
    const ForestDev& a, uint32_t key, int depth, int s, int e) {
    return node_draws(TAG_THRESH, a, key, depth, s, e);
}
// The drawn bin of feature f (wave-uniform) with occupied range [mn, mx].
__device__ __forceinline__ int et_bin(uint32_t thr_mine, int f, int mn,
                                      int mx) {
    return mn + (int)philox_bounded(wave_bcast(thr_mine, f),
                                    (uint32_t)(mx - mn));
}

// Best bin of one 256-bin histogram row, by one wave.  counts(b) returns
// bin b's (total, class-1) counts; lane l takes bins 4l..4l+3.  Returns,
// wave-uniform, the best (score, bin, left count) over the occupied bins
// in [bmin, bmax), the lowest bin winning ties, or bin = -1 if there is
// none.  Split scores only change at occupied bins, and the first bin of
// an equal-score run is occupied, so skipping empty bins preserves the
// argmax-first result.  PACKED_SCAN carries both prefix counts in one
// scan; it needs n < 2^15 (callers: n <= MID_N).
template <bool PACKED_SCAN, class CountsFn>
__device__ __forceinline__ void wave_best_bin(
    CountsFn counts, int bmin, int bmax, int n, int c0, int c1,
    double& best_s, int& best_b, int& best_nl) {
    const int lane = threadIdx.x & 63;
    int ln[4], l1[4];
    int tn = 0, t1 = 0;
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint2 v = counts(lane * 4 + k);
        ln[k] = (int)v.x;
        l1[k] = (int)v.y;
        tn += ln[k];
        t1 += l1[k];
    }
    int cn, c1f;   // exclusive prefix counts of this lane's first bin
    if (PACKED_SCAN) {
        const int sc = wave_scan_incl_i32(tn | (t1 << 16));
        cn = (sc & 0xFFFF) - tn;
        c1f = (sc >> 16) - t1;
    } else {
        cn = wave_scan_incl_i32(tn) - tn;
        c1f = wave_scan_incl_i32(t1) - t1;
    }
    best_s = -1.0;   // all real scores are > 0
    best_b = -1;
    best_nl = 0;
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = lane * 4 + k;
        cn += ln[k];
        c1f += l1[k];
        if (ln[k] == 0 || b < bmin || b >= bmax) continue;
        const double s = split_score(cn, c1f, n, c0, c1);
        if (s > best_s) { best_s = s; best_b = b; best_nl = cn; }
    }
    wave_argmax_mid(best_s, best_b, best_nl);
}

// The split chosen among a node's candidates.  Candidates are offered in
// permutation order and a later one must be strictly better, so the first
// of equal scores is kept; bin < 0 marks a candidate with no valid bin.
struct BestSplit {
    double score;
    int feat, bin, nL;   // feat = -1: no valid split (the node is a leaf)
};
__device__ __forceinline__ BestSplit no_split() {
    return {-1.0e300, -1, -1, 0};
}
__device__ __forceinline__ void offer_split(BestSplit& best, double score,
                                            int feat, int bin, int nL) {
    if (bin >= 0 && score > best.score) best = {score, feat, bin, nL};
}

// Turn `node` of `job` (node arrays at nbase) into a split on (feat, bin):
// allocate its two children (both start as leaves; right = left + 1) and
// return the left child's id.  Called by one thread.
__device__ __forceinline__ int commit_split(const ForestDev& a, int job,
                                            long nbase, int node, int feat,
                                            int bin) {
    const int l = atomicAdd(&a.node_alloc[job], 2);
    a.nfeat[nbase + l] = LEAF_SENTINEL;
    a.nfeat[nbase + l + 1] = LEAF_SENTINEL;
    a.nfeat[nbase + node] = feat;
    a.nsplit[nbase + node] = bin;
    a.nleft[nbase + node] = l;
    return l;
}

// Occupied-bin range [sh_bmin[f], sh_bmax[f]] of every feature's histogram
// row (total(f, b) = bin count), by the whole block: each thread scans one
// 16-bin segment of one feature.  Ends with a barrier.
template <class TotalFn>
__device__ __forceinline__ void block_bin_ranges(int F, TotalFn total,
                                                 int* sh_bmin, int* sh_bmax) {
    const int tid = threadIdx.x;
    if (tid < F) {
        sh_bmin[tid] = 256;
        sh_bmax[tid] = -1;
    }
    __syncthreads();
    const int f = tid >> 4;
    const int seg = (tid & 15) * 16;
    if (f < F) {
        int lo = 256, hi = -1;
        for (int b = seg; b < seg + 16; ++b)
            if (total(f, b)) {
                if (lo == 256) lo = b;
                hi = b;
            }
        if (hi >= 0) {
            atomicMin(&sh_bmin[f], lo);
            atomicMax(&sh_bmax[f], hi);
        }
    }
    __syncthreads();
}

// Feature permutation and candidate walk of a block-built node [s, e):
// wave 0 keeps the permutation in a register and walks it, taking
// non-constant features (sh_min[f] != sh_max[f]; a constant one is skipped
// and not counted) until max_features are found.  Fills sh_cand and, for
// the random splitter, each candidate's drawn bin in sh_cbin; returns the
// candidate count to every thread.  The per-feature ranges must be
// complete (barrier) on entry; ends with a barrier.
__device__ __forceinline__ int block_candidates(
    const ForestDev& a, uint32_t key, int depth, int s, int e,
    int max_features, bool random, const int* sh_min, const int* sh_max,
    int* sh_cand, int* sh_cbin, int* sh_ncand) {
    if (threadIdx.x < 64) {
        const uint64_t perm = featsel_perm(a, key, depth, s, e);
        const uint32_t thr_mine =
            random ? thresh_draws(a, key, depth, s, e) : 0u;
        int nc = 0;
        for (int i = 0; i < a.F && nc < max_features; ++i) {
            const int f = perm_at(perm, i);
            // every lane reads the same word: keep the walk scalar
            const int mn = __builtin_amdgcn_readfirstlane(sh_min[f]);
            const int mx = __builtin_amdgcn_readfirstlane(sh_max[f]);
            if (mn == mx) continue;
            const int b = random ? et_bin(thr_mine, f, mn, mx) : 0;
            if (threadIdx.x == 0) {
                sh_cand[nc] = f;
                if (random) sh_cbin[nc] = b;
            }
            ++nc;
        }
        if (threadIdx.x == 0) *sh_ncand = nc;
    }
    __syncthreads();
    return *sh_ncand;
}

// Stable partition of entries [start, end) by the whole block, 256-wide
// tiles: load(i, v) fetches entry i into v and returns whether it goes
// left; store(dst, v) places it.  Lefts are packed from `start`, rights
// from start + nL, both in source order.  Ranks come from wave ballots
// (valid lanes are a prefix of the tile, so cross-wave offsets are 4 LDS
// words); the running offsets are block-uniform and stay in registers.
// Two barriers per tile, the second after the tile's stores.
template <class LoadFn, class StoreFn>
__device__ __forceinline__ void block_partition(
    int start, int end, int nL, int* sh_wsum, LoadFn load, StoreFn store) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    int loff = 0, roff = 0;
    for (int base = start; base < end; base += HBLK) {
        const int i = base + tid;
        const bool valid = i < end;
        int v = 0;
        bool left = false;
        if (valid) left = load(i, v);
        const unsigned long long lm = __ballot(left);
        const int left_rank = __popcll(lm & ((1ULL << lane) - 1ULL));
        if (lane == 0) sh_wsum[wave] = __popcll(lm);
        __syncthreads();
        int lefts_before = left_rank;   // in this tile
        for (int ww = 0; ww < wave; ++ww) lefts_before += sh_wsum[ww];
        const int tile_left = sh_wsum[0] + sh_wsum[1] + sh_wsum[2]
                              + sh_wsum[3];
        const int tile_n = min(HBLK, end - base);
        if (valid)
            // rights before me = my tile index - lefts before me
            store(left ? start + loff + lefts_before
                       : start + nL + roff + (i - base) - lefts_before, v);
        __syncthreads();
        loff += tile_left;
        roff += tile_n - tile_left;
    }
}

// The level kernels' partition: sidx_cur -> sidx_nxt on code(feat) <= bin.
__device__ __forceinline__ void partition_samples(
    const ForestDev& a, const WorkItem& it, const BestSplit& best,
    int* sh_wsum) {
    const long sbase = a.j_sidx_off[it.job];
    block_partition(
        it.start, it.end, best.nL, sh_wsum,
        [&](int i, int& row) {
            row = a.sidx_cur[sbase + i];
            return a.codes[(size_t)row * FPAD + best.feat]
                   <= (uint32_t)best.bin;
        },
        [&](int dst, int row) { a.sidx_nxt[sbase + dst] = row; });
}

// ---------------------------------------------------------------------------
// Init: fill per-job sample indices (bootstrap or identity) and root items.
// Bootstrap draw i: bounded(philox(TAG_BOOTSTRAP, 0, 0, i), n)  — matches
// forest_ref.fit_forest.
// ---------------------------------------------------------------------------
__global__ void forest_init_kernel(
    const int* __restrict__ j_row_off, const int* __restrict__ j_n,
    const long* __restrict__ j_sidx_off, const int* __restrict__ j_key,
    const long* __restrict__ j_node_off, int* __restrict__ nfeat,
    int* __restrict__ node_alloc, int* __restrict__ sidx,
    WorkItem* __restrict__ work, const uint8_t* __restrict__ j_boot,
    uint32_t seed) {
    int job = blockIdx.x;
    int n = j_n[job];
    long off = j_sidx_off[job];
    int row0 = j_row_off[job];
    uint32_t key = (uint32_t)j_key[job];
    const int bootstrap = j_boot[job];

    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        int s;
        if (bootstrap) {
            uint32_t u = philox_draw(TAG_BOOTSTRAP, 0u, 0u, (uint32_t)i,
                                     seed, key);
            s = (int)philox_bounded(u, (uint32_t)n);
        } else {
            s = i;
        }
        sidx[off + i] = row0 + s;
    }
    if (threadIdx.x == 0) {
        node_alloc[job] = 1;
        nfeat[j_node_off[job]] = LEAF_SENTINEL;   // root starts as a leaf
        work[job] = {job, 0, 0, n, 0, -1};
    }
}

// ---------------------------------------------------------------------------
// The level kernel: histogram + split + partition, one workgroup per item.
// ---------------------------------------------------------------------------
// Histogram packing (WIDE = false): one uint32 per (feature, bin) with
// the total count in bits 0-15 and the class-1 count in bits 16-31 — one
// LDS atomic per (sample, feature) and 16 KiB LDS (double the resident
// blocks per CU).  Nodes with n >= 2^16 overflow the packing; the WIDE
// instantiation uses two unpacked count planes (32 KiB LDS, two atomics)
// and handles exactly those nodes — the two instantiations filter the
// same work queue by node size, so arbitrarily large training sets work
// (top levels wide, everything below packed).
template <bool WIDE>
__launch_bounds__(HBLK)
__global__ void hist_split_kernel(ForestDev a) {
    __shared__ uint32_t hist[FPAD * 256 * (WIDE ? 2 : 1)];
    __shared__ int sh_wsum[HBLK / 64];
    __shared__ int sh_bmin[FPAD], sh_bmax[FPAD];
    __shared__ int sh_cand[FPAD], sh_ncand;
    __shared__ double sh_score[FPAD];
    __shared__ int sh_bin[FPAD], sh_nL[FPAD];
    __shared__ BestSplit sh_best;
    __shared__ int sh_lid;                 // allocated left-child node id
    __shared__ int sh_accum_small;         // phase-8 plan flags
    __shared__ int sh_slot_small, sh_slot_large, sh_small_is_left;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n_items = *a.cur_count;

    for (int wi = blockIdx.x; wi < n_items; wi += gridDim.x) {
        WorkItem it = a.cur[wi];
        const int n = it.end - it.start;
        if ((n >= 65536) != WIDE) continue;   // size-class filter (uniform)
        if (a.j_rand[it.job]) continue;       // random-splitter: et_split's
        const long sbase = a.j_sidx_off[it.job];
        const long nbase = a.j_node_off[it.job];
        const uint32_t key = (uint32_t)a.j_key[it.job];
        const int F = a.F;

        // helpers: per-(feature, bin) total / class-1 counts
        auto h_n = [&](int f, int b) -> uint32_t {
            return WIDE ? hist[f * 256 + b] : (hist[f * 256 + b] & 0xFFFFu);
        };
        auto h_1 = [&](int f, int b) -> uint32_t {
            return WIDE ? hist[FPAD * 256 + f * 256 + b]
                        : (hist[f * 256 + b] >> 16);
        };

        // Phase 0/1: obtain the node histogram — either load the slot the
        // parent precomputed (subtraction scheme), or zero + accumulate.
        if (!WIDE && it.hist_slot >= 0) {
            const uint32_t* src =
                ((it.depth & 1) ? a.hist_pool1 : a.hist_pool0)
                + (size_t)it.hist_slot * (FPAD * 256);
            for (int i = tid; i < F * 64; i += HBLK)
                reinterpret_cast<uint4*>(hist)[i] =
                    reinterpret_cast<const uint4*>(src)[i];
        } else {
            const int zwords = F * 64 * (WIDE ? 2 : 1);
            for (int i = tid; i < zwords; i += HBLK)
                reinterpret_cast<uint4*>(hist)[i] = uint4{0, 0, 0, 0};
            __syncthreads();
            // One uint4 = the sample's 16 packed bin codes.
            for (int i = it.start + tid; i < it.end; i += HBLK) {
                int row = a.sidx_cur[sbase + i];
                uint4 cw = *reinterpret_cast<const uint4*>(
                    a.codes + (size_t)row * FPAD);
                uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
                const uint32_t lab = a.labels[row];
                const uint32_t inc = WIDE ? 1u : (1u | (lab << 16));
                for (int f = 0; f < F; ++f) {
                    uint32_t b = (w[f >> 2] >> ((f & 3) * 8)) & 0xFFu;
                    atomicAdd(&hist[f * 256 + b], inc);
                    if (WIDE && lab)
                        atomicAdd(&hist[FPAD * 256 + f * 256 + b], 1u);
                }
            }
        }
        __syncthreads();

        // Phase 2: class counts from the feature-0 histogram.
        const int c1 = block_sum_i32((int)h_1(0, tid), sh_wsum);
        const int c0 = n - c1;

        if (tid == 0) {
            a.ncnt0[nbase + it.node] = (float)c0;
            a.ncnt1[nbase + it.node] = (float)c1;
        }

        if (n < 2 || c0 == 0 || c1 == 0) {
            __syncthreads();
            continue;  // leaf (nfeat stays LEAF_SENTINEL)
        }

        // Phase 3: occupied-bin range per feature.
        block_bin_ranges(F, h_n, sh_bmin, sh_bmax);

        // Phase 4: feature permutation + candidate list.
        const int ncand = block_candidates(
            a, key, it.depth, it.start, it.end, a.j_mf[it.job], false,
            sh_bmin, sh_bmax, sh_cand, nullptr, &sh_ncand);
        if (ncand == 0) {
            __syncthreads();
            continue;  // all features constant: leaf
        }

        // Phase 5: evaluate candidates; wave w handles candidates w, w+4, ...
        // (two 32-bit scans: WIDE counts do not fit the packed one).
        for (int ci = wave; ci < ncand; ci += HBLK / 64) {
            const int f = sh_cand[ci];
            double best_s;
            int best_b, best_nl;
            wave_best_bin<false>(
                [&](int b) { return uint2{h_n(f, b), h_1(f, b)}; },
                sh_bmin[f], sh_bmax[f], n, c0, c1, best_s, best_b, best_nl);
            if (lane == 0) {
                sh_score[ci] = best_s;
                sh_bin[ci] = best_b;
                sh_nL[ci] = best_nl;
            }
        }
        __syncthreads();

        // Phase 6 (thread 0): select in permutation order and commit.
        if (tid == 0) {
            BestSplit best = no_split();
            for (int ci = 0; ci < ncand; ++ci)
                offer_split(best, sh_score[ci], sh_cand[ci], sh_bin[ci],
                            sh_nL[ci]);
            sh_best = best;
            if (best.feat >= 0)
                sh_lid = commit_split(a, it.job, nbase, it.node, best.feat,
                                      best.bin);
        }
        __syncthreads();

        const BestSplit best = sh_best;
        if (best.feat < 0) {
            __syncthreads();
            continue;  // no valid split: leaf
        }
        const int bf = best.feat, bb = best.bin, nL = best.nL;

        // Phase 7: stable partition into sidx_nxt.
        partition_samples(a, it, best, sh_wsum);

        // Phase 8: histogram-subtraction bookkeeping + child item push.
        // A big splitting node accumulates its SMALLER child's histogram
        // here (the children's samples are now contiguous in sidx_nxt) and
        // stores smaller + (parent - smaller) so both children skip their
        // accumulation.  Exact integer counts — results are unchanged.
        if (tid == 0) {
            // class-1 count of the left child (prefix over chosen feature)
            int n1L = 0;
            for (int b = 0; b <= bb; ++b)
                n1L += (int)h_1(bf, b);
            const int nR = n - nL;
            const int n1R = c1 - n1L;
            // only children that will run the histogram path need a slot
            const bool l_needs = nL > SMALL_N && n1L > 0 && n1L < nL;
            const bool r_needs = nR > SMALL_N && n1R > 0 && n1R < nR;
            sh_small_is_left = nL <= nR;
            const bool small_needs = sh_small_is_left ? l_needs : r_needs;
            const bool large_needs = sh_small_is_left ? r_needs : l_needs;

            sh_slot_small = sh_slot_large = -1;
            sh_accum_small = 0;
            // no pools on the WIDE path: packed 16-bit slots cannot hold
            // its counts (its children > 2048 re-accumulate)
            if (!WIDE && n >= a.hist_save_min &&
                (small_needs || large_needs)) {
                const int wp = (it.depth + 1) & 1;
                const int want = (small_needs ? 1 : 0) +
                                 (large_needs ? 1 : 0);
                int s = atomicAdd(&a.pool_count[wp * 4], want);
                if (s + want <= a.pool_cap) {
                    sh_accum_small = 1;
                    if (small_needs) sh_slot_small = s++;
                    if (large_needs) sh_slot_large = s;
                }
            }

            const int sl = sh_small_is_left ? sh_slot_small : sh_slot_large;
            const int sr = sh_small_is_left ? sh_slot_large : sh_slot_small;
            route_child(a, {it.job, sh_lid, it.start, it.start + nL,
                            it.depth + 1, sh_accum_small ? sl : -1});
            route_child(a, {it.job, sh_lid + 1, it.start + nL, it.end,
                            it.depth + 1, sh_accum_small ? sr : -1});
        }
        __syncthreads();

        if (sh_accum_small) {
            // stash the parent histogram in registers (16 words/thread)
            uint32_t stash[FPAD];
            #pragma unroll
            for (int r = 0; r < FPAD; ++r)
                stash[r] = (tid + r * HBLK < F * 256)
                               ? hist[tid + r * HBLK] : 0u;
            __syncthreads();

            for (int i = tid; i < F * 64; i += HBLK)
                reinterpret_cast<uint4*>(hist)[i] = uint4{0, 0, 0, 0};
            __syncthreads();

            const int s0 = sh_small_is_left ? it.start : it.start + nL;
            const int s1 = sh_small_is_left ? it.start + nL : it.end;
            for (int i = s0 + tid; i < s1; i += HBLK) {
                int row = a.sidx_nxt[sbase + i];
                uint4 cw = *reinterpret_cast<const uint4*>(
                    a.codes + (size_t)row * FPAD);
                uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
                const uint32_t inc = 1u | ((uint32_t)a.labels[row] << 16);
                for (int f = 0; f < F; ++f) {
                    uint32_t b = (w[f >> 2] >> ((f & 3) * 8)) & 0xFFu;
                    atomicAdd(&hist[f * 256 + b], inc);
                }
            }
            __syncthreads();

            uint32_t* wpool = ((it.depth + 1) & 1) ? a.hist_pool1
                                                   : a.hist_pool0;
            if (sh_slot_small >= 0) {
                uint32_t* dst = wpool + (size_t)sh_slot_small * (FPAD * 256);
                for (int i = tid; i < F * 256; i += HBLK)
                    dst[i] = hist[i];
            }
            if (sh_slot_large >= 0) {
                uint32_t* dst = wpool + (size_t)sh_slot_large * (FPAD * 256);
                #pragma unroll
                for (int r = 0; r < FPAD; ++r) {
                    const int i = tid + r * HBLK;
                    if (i < F * 256) dst[i] = stash[r] - hist[i];
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Extra-Trees level kernel: histogram-free.
//
// The random splitter needs only (a) per-feature occupied min/max codes to
// know constancy and the draw range, and (b) left counts at ONE drawn bin
// per candidate feature — two atomic-free passes over the node's samples
// instead of a 16-way-atomic histogram pass.  Scores, draws and
// tie-breaking are identical to the histogram path (same Philox counters,
// same fp64 expression), so trees are unchanged.  Used for all
// splitter_random jobs; the wave-subtree kernel handles their <=64 tails.
// ---------------------------------------------------------------------------
__launch_bounds__(HBLK)
__global__ void et_split_kernel(ForestDev a) {
    __shared__ int sh_wsum[HBLK / 64];
    __shared__ int sh_min[FPAD], sh_max[FPAD];
    __shared__ int sh_cand[FPAD], sh_cbin[FPAD], sh_ncand;
    __shared__ int sh_cnt[4][FPAD], sh_cnt1[4][FPAD];
    __shared__ BestSplit sh_best;
    __shared__ int sh_lid;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n_items = *a.cur_count;

    for (int wi = blockIdx.x; wi < n_items; wi += gridDim.x) {
        WorkItem it = a.cur[wi];
        const int n = it.end - it.start;
        if (!a.j_rand[it.job]) continue;     // best-splitter: hist_split's
        const long sbase = a.j_sidx_off[it.job];
        const long nbase = a.j_node_off[it.job];
        const uint32_t key = (uint32_t)a.j_key[it.job];
        const int F = a.F;

        if (tid < F) {
            sh_min[tid] = 256;
            sh_max[tid] = -1;
        }
        __syncthreads();

        // Pass 1: per-feature min/max + class-1 count.
        int lmin[FPAD], lmax[FPAD];
        #pragma unroll
        for (int f = 0; f < FPAD; ++f) { lmin[f] = 256; lmax[f] = -1; }
        int lc1 = 0;
        for (int i = it.start + tid; i < it.end; i += HBLK) {
            int row = a.sidx_cur[sbase + i];
            uint4 cw = *reinterpret_cast<const uint4*>(
                a.codes + (size_t)row * FPAD);
            uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
            lc1 += a.labels[row];
            for (int f = 0; f < F; ++f) {
                const int b = (int)((w[f >> 2] >> ((f & 3) * 8)) & 0xFFu);
                lmin[f] = min(lmin[f], b);
                lmax[f] = max(lmax[f], b);
            }
        }
        for (int f = 0; f < F; ++f) {
            const int mn = wave_min_i32(lmin[f]);
            const int mx = wave_max_i32(lmax[f]);
            if (lane == 0) {
                atomicMin(&sh_min[f], mn);
                atomicMax(&sh_max[f], mx);
            }
        }
        // (its barriers also complete sh_min / sh_max)
        const int c1 = block_sum_i32(lc1, sh_wsum);
        const int c0 = n - c1;

        if (tid == 0) {
            a.ncnt0[nbase + it.node] = (float)c0;
            a.ncnt1[nbase + it.node] = (float)c1;
        }
        if (n < 2 || c0 == 0 || c1 == 0) {
            __syncthreads();
            continue;
        }

        // Feature permutation, candidate list and each candidate's drawn bin.
        const int ncand = block_candidates(
            a, key, it.depth, it.start, it.end, a.j_mf[it.job], true,
            sh_min, sh_max, sh_cand, sh_cbin, &sh_ncand);
        if (ncand == 0) {
            __syncthreads();
            continue;
        }

        // Pass 2: left counts at each candidate's drawn bin.
        int cnt[FPAD], cnt1[FPAD];
        for (int ci = 0; ci < ncand; ++ci) { cnt[ci] = 0; cnt1[ci] = 0; }
        for (int i = it.start + tid; i < it.end; i += HBLK) {
            int row = a.sidx_cur[sbase + i];
            uint4 cw = *reinterpret_cast<const uint4*>(
                a.codes + (size_t)row * FPAD);
            uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
            const int lab = a.labels[row];
            for (int ci = 0; ci < ncand; ++ci) {
                const int f = sh_cand[ci];
                const int b = (int)((w[f >> 2] >> ((f & 3) * 8)) & 0xFFu);
                const int le = b <= sh_cbin[ci];
                cnt[ci] += le;
                cnt1[ci] += le & lab;
            }
        }
        for (int ci = 0; ci < ncand; ++ci) {
            const int c = wave_sum_i32(cnt[ci]);
            const int c1l = wave_sum_i32(cnt1[ci]);
            if (lane == 0) {
                sh_cnt[wave][ci] = c;
                sh_cnt1[wave][ci] = c1l;
            }
        }
        __syncthreads();

        // Select in permutation order and commit (thread 0).
        if (tid == 0) {
            BestSplit best = no_split();
            for (int ci = 0; ci < ncand; ++ci) {
                const long nL = sh_cnt[0][ci] + sh_cnt[1][ci]
                                + sh_cnt[2][ci] + sh_cnt[3][ci];
                const long n1L = sh_cnt1[0][ci] + sh_cnt1[1][ci]
                                 + sh_cnt1[2][ci] + sh_cnt1[3][ci];
                if (nL == 0 || nL == n) continue;
                offer_split(best, split_score(nL, n1L, n, c0, c1),
                            sh_cand[ci], sh_cbin[ci], (int)nL);
            }
            sh_best = best;
            if (best.feat >= 0)
                sh_lid = commit_split(a, it.job, nbase, it.node, best.feat,
                                      best.bin);
        }
        __syncthreads();

        const BestSplit best = sh_best;
        if (best.feat < 0) {
            __syncthreads();
            continue;
        }
        const int nL = best.nL;

        partition_samples(a, it, best, sh_wsum);

        // Push children (no histogram slots on the ET path).
        if (tid == 0) {
            route_child(a, {it.job, sh_lid, it.start, it.start + nL,
                            it.depth + 1, -1});
            route_child(a, {it.job, sh_lid + 1, it.start + nL, it.end,
                            it.depth + 1, -1});
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Mid-subtree builder: one BLOCK finishes the whole subtree of a node with
// SMALL_N < n <= MID_N samples from LDS-resident data.
//
// The node's code rows + labels are staged into LDS ONCE; the block then
// recurses (smaller-child-first DFS, stack in LDS) over its > SMALL_N
// descendants with LDS histograms and LDS index partitions — no level
// round-trips, no global gathers per level (PMC showed the level kernels
// 40-69% wait-bound on exactly those).  <= SMALL_N descendants are written
// back (final index arrangement -> sidx buffer) and pushed to the small
// queue for the wave kernel.  Split semantics, RNG counters (global
// job-relative (start,end) ranges) and fp64 scores are identical to
// hist_split_kernel — trees are bit-identical.
// Handles both splitters (best: prefix scan over bins; random: drawn bin).
// ---------------------------------------------------------------------------
struct MidFrame {
    short s, e;     // LOCAL sample range within the staged window
    int depth;
    int node;
};

// Block-serial DFS (DT / fallback) needs <= log2(MID_N)+2 entries; the
// wave-parallel mode (4 nodes in flight, breadth-ish order) can hold the
// whole >SMALL_N frontier of a MID_N subtree: live frames are disjoint
// ranges of > SMALL_N samples inside <= MID_N samples, so at most 31 of
// them exist at once; a full stack is a logic error and trips err_flag.
#define MID_STACK 96
#define WAVE_CANDS 4   // wave-parallel path: max_features <= 4 (RF / ET)

// m_idx / m_idx2 entries: local sample index (11 bits for MID_N = 2048)
// with the sample's label in bit 15, set once at staging, so no pass reads
// a separate label array.  Partitions move the entry whole; the write-back
// masks the bit.
#define MID_LAB_BIT 15
#define MID_IDX_MASK 0x7FFF

// A <= SMALL_N child of a mid item goes to the global small queue with its
// final global range and the mid item's buffer tag (the write-back lands
// in the mid root's buffer).  Called by one thread.
__device__ __forceinline__ void mid_farm_small(
    const ForestDev& a, const WorkItem& it, int s, int e, int depth,
    int node) {
    const int i = atomicAdd(a.small_count, 1);
    if (i < a.small_cap)
        a.small[i] = {it.job, node, it.start + s, it.start + e, depth,
                      it.hist_slot};
    else
        atomicExch(a.err_flag, 1);
}

// One 64-lane wave splits one node [ls, le) of the staged window and
// routes its children (shared LDS stack for > SMALL_N, global small queue
// otherwise).  Control flow is wave-uniform throughout; split semantics,
// Philox counters (global job-relative ranges) and fp64 scores are
// identical to the block-wide path — trees are bit-identical.  Requires
// max_features <= WAVE_CANDS (RF / ET; DT keeps the block path).
// whist: this wave's WAVE_CANDS*256-word LDS histogram region (RF only).
template <bool STAGED>
__device__ __forceinline__ void mid_wave_node(
    const ForestDev& a, const WorkItem& it, int ls, int le, int depth,
    int node, const uint4* m_codes, const int* m_rows, uint16_t* m_idx,
    uint16_t* m_idx2, uint32_t* whist, MidFrame* stack,
    int* sh_count) {
    // STAGED reads the LDS-staged code rows; the unstaged variant reads
    // them from L1/L2 through the m_rows map (half the LDS per block).
    // m_idx entries carry the sample's label in bit 15 (MID_LAB_BIT).
    auto code_at = [&](int o) -> uint4 {
        if (STAGED) return m_codes[o];
        return *reinterpret_cast<const uint4*>(
            a.codes + (size_t)m_rows[o] * FPAD);
    };
    const int lane = threadIdx.x & 63;
    const int n = le - ls;
    const long nbase = a.j_node_off[it.job];
    const uint32_t key = (uint32_t)a.j_key[it.job];
    const int F = a.F;
    const int max_features = a.j_mf[it.job];
    const int splitter_random = a.j_rand[it.job];
    const int gs = it.start + ls;   // global job-relative range (RNG id)
    const int ge = it.start + le;

    // Pass 1: per-feature occupied min/max + class-1 count.  Each code
    // word is unpacked into two u16 pairs, so one packed min and one
    // packed max cover two features: pmin[2k] holds features 4k (low
    // half) and 4k+2 (high half), pmin[2k+1] features 4k+1 and 4k+3.
    // Only the words that hold a feature < F are touched.
    const int nw = (F + 3) >> 2;
    uint32_t pmin[FPAD / 2], pmax[FPAD / 2];
    #pragma unroll
    for (int k = 0; k < FPAD / 2; ++k) { pmin[k] = 0x01000100u; pmax[k] = 0u; }
    int lc1 = 0;
    for (int i = ls + lane; i < le; i += 64) {
        const int ent = m_idx[i];
        const uint4 cw = code_at(ent & MID_IDX_MASK);
        const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
        lc1 += ent >> MID_LAB_BIT;
        #pragma unroll
        for (int k = 0; k < FPAD / 4; ++k) {
            if (k >= nw) break;
            const uint32_t ev = w[k] & 0x00FF00FFu;
            const uint32_t od = (w[k] >> 8) & 0x00FF00FFu;
            pmin[2 * k] = pkmin_u16x2(pmin[2 * k], ev);
            pmax[2 * k] = pkmax_u16x2(pmax[2 * k], ev);
            pmin[2 * k + 1] = pkmin_u16x2(pmin[2 * k + 1], od);
            pmax[2 * k + 1] = pkmax_u16x2(pmax[2 * k + 1], od);
        }
    }
    const int c1 = wave_sum_i32(lc1);
    const int c0 = n - c1;

    if (lane == 0) {
        a.ncnt0[nbase + node] = (float)c0;
        a.ncnt1[nbase + node] = (float)c1;
    }
    if (n < 2 || c0 == 0 || c1 == 0) return;   // leaf

    // Cross-lane reduction; the results are wave-uniform.  Lane f < 16
    // then keeps feature f's range as (min | max << 16) in rng_mine, so
    // the candidate walk fetches a range with one v_readlane and never
    // indexes a register array dynamically.
    uint32_t rng_mine = 0;
    #pragma unroll
    for (int k = 0; k < FPAD / 4; ++k) {
        if (k >= nw) break;
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t umin = wave_pkmin_u16x2(pmin[2 * k + h]);
            const uint32_t umax = wave_pkmax_u16x2(pmax[2 * k + h]);
            // low halves: feature 4k + h; high halves: feature 4k + h + 2
            if (lane == 4 * k + h)
                rng_mine = (umin & 0xFFFFu) | (umax << 16);
            if (lane == 4 * k + h + 2)
                rng_mine = (umin >> 16) | (umax & 0xFFFF0000u);
        }
    }

    // Feature permutation + candidate walk, wave-uniform in registers:
    // candidates, their ranges and (ET) drawn bins are packed 4 / 8 bits
    // per candidate (WAVE_CANDS = 4 candidates, values <= 255).
    const uint64_t perm = featsel_perm(a, key, depth, gs, ge);
    const uint32_t thr_mine =
        splitter_random ? thresh_draws(a, key, depth, gs, ge) : 0u;
    int ncand = 0;
    uint32_t cand_pk = 0, cbin_pk = 0, cmin_pk = 0, cmax_pk = 0;
    for (int i = 0; i < F && ncand < max_features; ++i) {
        const int f = perm_at(perm, i);
        const uint32_t r = wave_bcast(rng_mine, f);
        const int mn = (int)(r & 0xFFFFu), mx = (int)(r >> 16);
        if (mn == mx) continue;
        cand_pk |= (uint32_t)f << (4 * ncand);
        cmin_pk |= (uint32_t)mn << (8 * ncand);
        cmax_pk |= (uint32_t)mx << (8 * ncand);
        if (splitter_random)
            cbin_pk |= (uint32_t)et_bin(thr_mine, f, mn, mx) << (8 * ncand);
        ++ncand;
    }
    if (ncand == 0) return;   // all candidates constant: leaf

    BestSplit best = no_split();

    if (splitter_random) {
        // ET: counts at each candidate's drawn bin — histogram-free.  The
        // left count (low half) and its class-1 part (high half) share one
        // accumulator: n <= MID_N = 2048 fits 16 bits.
        int cnt[WAVE_CANDS];
        #pragma unroll
        for (int ci = 0; ci < WAVE_CANDS; ++ci) cnt[ci] = 0;
        for (int i = ls + lane; i < le; i += 64) {
            const int ent = m_idx[i];
            const uint4 cw = code_at(ent & MID_IDX_MASK);
            const int inc = 1 | ((ent >> MID_LAB_BIT) << 16);
            #pragma unroll
            for (int ci = 0; ci < WAVE_CANDS; ++ci) {
                if (ci >= ncand) break;
                const int f = (int)((cand_pk >> (4 * ci)) & 15u);
                const int b = (int)code_byte(cw, f);
                cnt[ci] += b <= (int)((cbin_pk >> (8 * ci)) & 0xFFu) ? inc : 0;
            }
        }
        #pragma unroll
        for (int ci = 0; ci < WAVE_CANDS; ++ci) {
            if (ci >= ncand) break;
            const uint2 t = unpack_counts((uint32_t)wave_sum_i32(cnt[ci]));
            const int nL = (int)t.x;
            if (nL == 0 || nL == n) continue;
            offer_split(best, split_score(nL, t.y, n, c0, c1),
                        (int)((cand_pk >> (4 * ci)) & 15u),
                        (int)((cbin_pk >> (8 * ci)) & 0xFFu), nL);
        }
    } else {
        // RF: candidate-only packed LDS histograms.
        for (int i = lane; i < ncand * 256; i += 64) whist[i] = 0;
        for (int i = ls + lane; i < le; i += 64) {
            const int ent = m_idx[i];
            const uint4 cw = code_at(ent & MID_IDX_MASK);
            const uint32_t inc = 1u | ((uint32_t)(ent >> MID_LAB_BIT) << 16);
            #pragma unroll
            for (int ci = 0; ci < WAVE_CANDS; ++ci) {
                if (ci >= ncand) break;
                const int f = (int)((cand_pk >> (4 * ci)) & 15u);
                const uint32_t b = code_byte(cw, f);
                atomicAdd(&whist[ci * 256 + b], inc);
            }
        }
        for (int ci = 0; ci < ncand; ++ci) {
            double cand_s;
            int cand_b, cand_nl;
            wave_best_bin<true>(
                [&](int b) { return unpack_counts(whist[ci * 256 + b]); },
                (int)((cmin_pk >> (8 * ci)) & 0xFFu),
                (int)((cmax_pk >> (8 * ci)) & 0xFFu), n, c0, c1,
                cand_s, cand_b, cand_nl);
            offer_split(best, cand_s, (int)((cand_pk >> (4 * ci)) & 15u),
                        cand_b, cand_nl);
        }
    }

    if (best.feat < 0) return;   // no valid split: leaf
    const int bf = best.feat, bb = best.bin, nL = best.nL;

    int lid = 0;
    if (lane == 0) lid = commit_split(a, it.job, nbase, node, bf, bb);
    lid = wave_bcast(lid, 0);

    // Stable partition of m_idx[ls, le) via this node's private m_idx2
    // range (sibling ranges are disjoint — no cross-wave aliasing).  The
    // entry moves whole: its label bit travels with the index.
    int lo = 0, ro = 0;
    for (int base = ls; base < le; base += 64) {
        const int i = base + lane;
        const bool valid = i < le;
        int o = 0, flag = 0;
        if (valid) {
            o = m_idx[i];
            const uint4 cw = code_at(o & MID_IDX_MASK);
            flag = (int)(code_byte(cw, bf) <= (uint32_t)bb);
        }
        const unsigned long long lm = __ballot(valid && flag);
        const unsigned long long below = (1ULL << lane) - 1ULL;
        const int rank = __popcll(lm & below);
        const int chunk_left = __popcll(lm);
        const int chunk_n = min(64, le - base);
        if (valid) {
            const int dst = flag
                ? ls + lo + rank
                : ls + nL + ro + (i - base) - rank;
            m_idx2[dst] = (uint16_t)o;
        }
        lo += chunk_left;
        ro += chunk_n - chunk_left;
    }
    for (int i = ls + lane; i < le; i += 64) m_idx[i] = m_idx2[i];

    // Route children: > SMALL_N to the shared stack; <= SMALL_N to the
    // global small queue with final global ranges and this mid item's
    // buffer tag (the write-back lands in the mid root's buffer).
    if (lane == 0) {
        auto route = [&](int s, int e, int child) {
            if (e - s > SMALL_N) {
                const int idx = atomicAdd(sh_count, 1);
                if (idx < MID_STACK) {
                    stack[idx] = {(short)s, (short)e, depth + 1, child};
                } else {
                    atomicSub(sh_count, 1);
                    atomicExch(a.err_flag, 1);   // unreachable (MID_STACK)
                }
            } else {
                mid_farm_small(a, it, s, e, depth + 1, child);
            }
        };
        route(ls, ls + nL, lid);
        route(ls + nL, le, lid + 1);
    }
}

// Waves per SIMD each variant is built for: the staged one is bounded by
// its LDS (2 blocks per CU); the unstaged one fits 4 blocks per CU and must
// stay within 128 VGPRs to use them.
template <bool STAGED>
__launch_bounds__(HBLK, STAGED ? 2 : 4)
__global__ void mid_subtree_kernel(ForestDev a) {
    __shared__ uint4 m_codes[STAGED ? MID_N : 1];   // 32 KiB staged rows
    __shared__ int m_rows[MID_N];             // 8 KiB original global rows
    // sample ordering / partition scratch, 4 KiB each: local index with
    // the label in bit 15 (MID_LAB_BIT)
    __shared__ uint16_t m_idx[MID_N];
    __shared__ uint16_t m_idx2[MID_N];
    __shared__ uint32_t hist[FPAD * 256];     // 16 KiB packed histogram
    __shared__ int sh_wsum[HBLK / 64];
    __shared__ int sh_bmin[FPAD], sh_bmax[FPAD];
    __shared__ int sh_cand[FPAD], sh_ncand;
    __shared__ double sh_score[FPAD];
    __shared__ int sh_bin[FPAD], sh_nL[FPAD];
    __shared__ BestSplit sh_best;
    __shared__ int sh_lid;
    __shared__ MidFrame stack[MID_STACK];
    // this round's frames (one per wave in wave-parallel mode)
    __shared__ MidFrame wframes[HBLK / 64];
    __shared__ int sh_count, sh_take, sh_nblock;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n_items = min(*a.mid_count, a.mid_cap);

    for (int wi = blockIdx.x; wi < n_items; wi += gridDim.x) {
        const WorkItem it = a.mid[wi];
        const int n0 = it.end - it.start;
        const long sbase = a.j_sidx_off[it.job];
        // the item's own buffer (tag): staged from and written back to
        int* const sidx_it = it.hist_slot ? a.sidx_b : a.sidx_a;
        const long nbase = a.j_node_off[it.job];
        const uint32_t key = (uint32_t)a.j_key[it.job];
        const int F = a.F;

        // Stage the subtree's samples into LDS (one gather, reused by
        // every internal level).
        for (int i = tid; i < n0; i += HBLK) {
            const int row = sidx_it[sbase + it.start + i];
            m_rows[i] = row;
            if (STAGED)
                m_codes[i] = *reinterpret_cast<const uint4*>(
                    a.codes + (size_t)row * FPAD);
            m_idx[i] = (uint16_t)(i | ((a.labels[row] != 0) << MID_LAB_BIT));
        }

        auto code_at = [&](int o) -> uint4 {
            if (STAGED) return m_codes[o];
            return *reinterpret_cast<const uint4*>(
                a.codes + (size_t)m_rows[o] * FPAD);
        };

        // Per-node block-wide builder (histogram, split, partition over
        // the staged window) shared by the DFS path and the wave mode's
        // small-frontier rounds; > SMALL_N children go on the stack with
        // the smaller one on top.
        auto block_node = [&](int ls, int le, int depth, int node) {
            const int n = le - ls;
            const int splitter_random = a.j_rand[it.job];
            // global job-relative range (the RNG identity)
            const int gs = it.start + ls;
            const int ge = it.start + le;

            // histogram from LDS-resident samples
            for (int i = tid; i < F * 64; i += HBLK)
                reinterpret_cast<uint4*>(hist)[i] = uint4{0, 0, 0, 0};
            __syncthreads();
            for (int i = ls + tid; i < le; i += HBLK) {
                const int ent = m_idx[i];
                const uint4 cw = code_at(ent & MID_IDX_MASK);
                const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
                const uint32_t inc =
                    1u | ((uint32_t)(ent >> MID_LAB_BIT) << 16);
                #pragma unroll
                for (int f = 0; f < FPAD; ++f) {   // static word indices
                    if (f >= F) break;
                    const uint32_t b = (w[f >> 2] >> ((f & 3) * 8)) & 0xFFu;
                    atomicAdd(&hist[f * 256 + b], inc);
                }
            }
            __syncthreads();

            // class counts from the feature-0 histogram
            const int c1 = block_sum_i32((int)(hist[tid] >> 16), sh_wsum);
            const int c0 = n - c1;

            if (tid == 0) {
                a.ncnt0[nbase + node] = (float)c0;
                a.ncnt1[nbase + node] = (float)c1;
            }
            if (n < 2 || c0 == 0 || c1 == 0) {
                __syncthreads();
                return;
            }

            block_bin_ranges(
                F, [&](int f, int b) { return hist[f * 256 + b] & 0xFFFFu; },
                sh_bmin, sh_bmax);

            // permutation + candidate walk; ET: sh_bin[ci] takes candidate
            // ci's drawn bin, which is the bin its evaluation reports
            const int ncand = block_candidates(
                a, key, depth, gs, ge, a.j_mf[it.job], splitter_random,
                sh_bmin, sh_bmax, sh_cand, sh_bin, &sh_ncand);
            if (ncand == 0) {
                __syncthreads();
                return;
            }

            // evaluate candidates, one wave per candidate
            for (int ci = wave; ci < ncand; ci += HBLK / 64) {
                const int f = sh_cand[ci];
                double best_s;
                int best_b, best_nl;
                if (splitter_random) {
                    // ET: left counts at the drawn bin = the row's counts
                    // over bins <= it (both in one sum: n <= MID_N).  The
                    // bin lies in [bmin, bmax), so neither child is empty.
                    best_b = sh_bin[ci];
                    int part = 0;
                    #pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int b = lane * 4 + k;
                        part += b <= best_b ? (int)hist[f * 256 + b] : 0;
                    }
                    const uint2 t =
                        unpack_counts((uint32_t)wave_sum_i32(part));
                    best_nl = (int)t.x;
                    best_s = split_score(t.x, t.y, n, c0, c1);
                } else {
                    wave_best_bin<true>(
                        [&](int b) {
                            return unpack_counts(hist[f * 256 + b]);
                        },
                        sh_bmin[f], sh_bmax[f], n, c0, c1, best_s, best_b,
                        best_nl);
                }
                if (lane == 0) {
                    sh_score[ci] = best_s;
                    sh_bin[ci] = best_b;
                    sh_nL[ci] = best_nl;
                }
            }
            __syncthreads();

            // select in permutation order and commit (thread 0)
            if (tid == 0) {
                BestSplit best = no_split();
                for (int ci = 0; ci < ncand; ++ci)
                    offer_split(best, sh_score[ci], sh_cand[ci], sh_bin[ci],
                                sh_nL[ci]);
                sh_best = best;
                if (best.feat >= 0)
                    sh_lid = commit_split(a, it.job, nbase, node, best.feat,
                                          best.bin);
            }
            __syncthreads();

            const BestSplit best = sh_best;
            if (best.feat < 0) {
                __syncthreads();
                return;
            }
            const int nL = best.nL;

            // stable partition of m_idx[ls,le) via m_idx2 (LDS); the whole
            // entry moves, its label bit with it
            block_partition(
                ls, le, nL, sh_wsum,
                [&](int i, int& o) {
                    o = m_idx[i];
                    return code_byte(code_at(o & MID_IDX_MASK), best.feat)
                           <= (uint32_t)best.bin;
                },
                [&](int dst, int o) { m_idx2[dst] = (uint16_t)o; });
            for (int i = ls + tid; i < le; i += HBLK) m_idx[i] = m_idx2[i];
            __syncthreads();

            if (tid == 0) {
                auto route = [&](int s, int e, int child) {
                    if (e - s <= SMALL_N)
                        mid_farm_small(a, it, s, e, depth + 1, child);
                    else if (sh_count < MID_STACK)
                        stack[sh_count++] =
                            {(short)s, (short)e, depth + 1, child};
                    else
                        atomicExch(a.err_flag, 1);   // unreachable
                };
                const int lid = sh_lid, mid = ls + nL;
                if (nL <= n - nL) {   // larger pushed first
                    route(mid, le, lid + 1);
                    route(ls, mid, lid);
                } else {
                    route(ls, mid, lid);
                    route(mid, le, lid + 1);
                }
            }
            __syncthreads();
        };

        // Rounds over the stack of > SMALL_N frames.  Wave-parallel mode
        // (max_features <= WAVE_CANDS) takes up to HBLK/64 frames per
        // round, each built by one wave with no block barrier inside a
        // node; a single-frame round — the top of every staged subtree —
        // and a round of two big frames are built block-wide instead, so
        // no wave idles there.  Block-serial mode (DT) takes one frame per
        // round: a DFS with the smaller child on top.  The block-wide
        // 16 KiB `hist` array is re-sliced as one WAVE_CANDS*256-word
        // histogram region per wave.
        const int per_round =
            a.wave_mid && a.j_mf[it.job] <= WAVE_CANDS ? HBLK / 64 : 1;
        if (tid == 0) {
            sh_count = 1;
            stack[0] = {0, (short)n0, it.depth, it.node};
        }
        while (true) {
            __syncthreads();
            if (tid == 0) {
                const int take = min(per_round, sh_count);
                for (int w = 0; w < take; ++w)
                    wframes[w] = stack[sh_count - 1 - w];
                sh_count -= take;
                sh_take = take;
                // two big frontier nodes: sequential block-wide processing
                // beats two waves with two idle
                sh_nblock =
                    take == 1 ? 1
                    : take == 2 && (wframes[0].e - wframes[0].s)
                                   + (wframes[1].e - wframes[1].s) > 1024
                        ? 2 : 0;
            }
            __syncthreads();
            const int take = sh_take, nblock = sh_nblock;
            if (take == 0) break;
            for (int x = 0; x < nblock; ++x) {
                const MidFrame fr = wframes[x];
                block_node(fr.s, fr.e, fr.depth, fr.node);
            }
            if (nblock == 0 && wave < take) {
                const MidFrame fr = wframes[wave];
                mid_wave_node<STAGED>(
                    a, it, fr.s, fr.e, fr.depth, fr.node,
                    m_codes, m_rows, m_idx, m_idx2,
                    hist + wave * (WAVE_CANDS * 256), stack, &sh_count);
            }
        }

        // write the final arrangement back so the small kernel (launched
        // after this one) reads each farmed subtree's samples
        __syncthreads();
        for (int i = tid; i < n0; i += HBLK)
            sidx_it[sbase + it.start + i] =
                m_rows[m_idx[i] & MID_IDX_MASK];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Wave-per-subtree builder for nodes with n <= SMALL_N (=64) samples.
//
// One 64-lane wave finishes the WHOLE subtree: each lane holds one
// sample's 16 packed codes + label in registers; node membership is a
// 64-bit lane mask; class/prefix counts come from __ballot+popcount; the
// DFS stack lives in LDS.  No histograms, no sample-index traffic, no
// further level round-trips.  The feature permutation, the min/max and
// argmax reductions and all broadcasts stay in registers (wave_ops.h).
// All randomness stays keyed on the node's
// (start, end) range (child ranges follow the stable-partition arithmetic
// [s, s+nL) / [s+nL, e)), and split scores use the identical fp64
// expression — trees are bit-identical to the histogram path / numpy
// reference.
// ---------------------------------------------------------------------------
struct SmallFrame {
    unsigned long long mask;
    int s, e, depth, node;
};

#define SMALL_STACK 68

__launch_bounds__(HBLK)
__global__ void small_subtree_kernel(ForestDev a) {
    __shared__ SmallFrame stack_ws[HBLK / 64][SMALL_STACK];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * (HBLK / 64);
    const int wave_id = blockIdx.x * (HBLK / 64) + wave;
    const int n_items = min(*a.small_count, a.small_cap);
    SmallFrame* stack = stack_ws[wave];

    for (int wi = wave_id; wi < n_items; wi += waves_total) {
        const WorkItem it = a.small[wi];
        const int n0 = it.end - it.start;
        const long sbase = a.j_sidx_off[it.job];
        const long nbase = a.j_node_off[it.job];
        const uint32_t key = (uint32_t)a.j_key[it.job];
        const int F = a.F;
        const int max_features = a.j_mf[it.job];
        const int splitter_random = a.j_rand[it.job];

        // lane -> sample (register-resident)
        uint32_t w[4] = {0, 0, 0, 0};
        int label = 0;
        if (lane < n0) {
            const int row =
                (it.hist_slot ? a.sidx_b : a.sidx_a)[sbase + it.start + lane];
            uint4 cw = *reinterpret_cast<const uint4*>(
                a.codes + (size_t)row * FPAD);
            w[0] = cw.x; w[1] = cw.y; w[2] = cw.z; w[3] = cw.w;
            label = a.labels[row];
        }
        const unsigned long long lab_mask = __ballot(label != 0);

        int sp = 0;
        if (lane == 0)
            stack[0] = {n0 >= 64 ? ~0ULL : ((1ULL << n0) - 1ULL),
                        it.start, it.end, it.depth, it.node};

        while (sp >= 0) {
            // pop (lane-uniform: all lanes read the same LDS entry)
            const unsigned long long mask = stack[sp].mask;
            const int s = stack[sp].s;
            const int e = stack[sp].e;
            const int depth = stack[sp].depth;
            const int node = stack[sp].node;
            --sp;

            const int n = __popcll(mask);
            const int c1 = __popcll(mask & lab_mask);
            const int c0 = n - c1;
            if (lane == 0) {
                a.ncnt0[nbase + node] = (float)c0;
                a.ncnt1[nbase + node] = (float)c1;
            }
            if (n < 2 || c0 == 0 || c1 == 0) continue;

            // feature permutation in a 64-bit register (wave_ops.h)
            const uint64_t perm = featsel_perm(a, key, depth, s, e);
            const uint32_t u_thresh =
                splitter_random ? thresh_draws(a, key, depth, s, e) : 0u;

            BestSplit best = no_split();
            int n_eval = 0;

            for (int pi = 0; pi < F && n_eval < max_features; ++pi) {
                const int f = perm_at(perm, pi);
                const int my_code = (int)((w[f >> 2] >> ((f & 3) * 8))
                                          & 0xFFu);
                const bool in = (mask >> lane) & 1ULL;
                // occupied-bin range in ONE packed reduction: low half
                // min(code), high half min(255 - code) = 255 - max(code);
                // inactive lanes carry the neutral 256 in both halves
                const uint32_t rng = wave_pkmin_u16x2(
                    in ? (uint32_t)my_code | ((uint32_t)(255 - my_code) << 16)
                       : 0x01000100u);
                const int cmin = (int)(rng & 0xFFFFu);
                const int cmax = 255 - (int)(rng >> 16);
                if (cmin == cmax) continue;   // constant: not counted
                ++n_eval;

                if (splitter_random) {
                    const int b = et_bin(u_thresh, f, cmin, cmax);
                    const unsigned long long lm =
                        mask & __ballot(in && my_code <= b);
                    const int nL = __popcll(lm);
                    if (nL > 0 && nL < n)
                        offer_split(best,
                                    split_score(nL, __popcll(lm & lab_mask),
                                                n, c0, c1),
                                    f, b, nL);
                } else {
                    // parallel-rank: every in-mask lane scores its OWN
                    // code as the threshold candidate (duplicates give
                    // identical (score, bin) pairs; the argmax tie-break
                    // to the lowest bin matches the ascending sequential
                    // scan exactly).  The rank (lanes with code <= mine)
                    // comes from 8 bit-plane ballots instead of a 64-step
                    // shuffle scan: after the loop E = lanes whose code
                    // equals mine, L = lanes whose code is strictly less.
                    unsigned long long E = ~0ULL, L = 0ULL;
                    #pragma unroll
                    for (int b = 7; b >= 0; --b) {
                        const unsigned long long B =
                            __ballot((my_code >> b) & 1);
                        if ((my_code >> b) & 1) {
                            L |= E & ~B;
                            E &= B;
                        } else {
                            E &= ~B;
                        }
                    }
                    const unsigned long long le_mask = (L | E) & mask;
                    const int cnt = __popcll(le_mask);
                    const int cnt1 = __popcll(le_mask & lab_mask);
                    double sc = -1.0e300;
                    int sb = 0x7FFFFFFF, snl = 0;
                    if (in && my_code < cmax) {
                        sc = split_score(cnt, cnt1, n, c0, c1);
                        sb = my_code;
                        snl = cnt;
                    }
                    wave_argmax_small(sc, sb, snl);
                    offer_split(best, sc, f, sb, snl);
                }
            }

            if (best.feat < 0) continue;   // no valid split: leaf
            const int best_f = best.feat, best_b = best.bin, nL = best.nL;

            int lid = 0;
            if (lane == 0)
                lid = commit_split(a, it.job, nbase, node, best_f, best_b);
            lid = wave_bcast(lid, 0);

            const int bc = (int)((w[best_f >> 2] >> ((best_f & 3) * 8))
                                 & 0xFFu);
            const unsigned long long lmask =
                mask & __ballot(((mask >> lane) & 1ULL) && bc <= best_b);

            if (lane == 0) {
                stack[sp + 1] = {mask & ~lmask, s + nL, e, depth + 1,
                                 lid + 1};
                stack[sp + 2] = {lmask, s, s + nL, depth + 1, lid};
            }
            sp += 2;   // left child on top: DFS order (order immaterial)
        }
    }
}

// ---------------------------------------------------------------------------
// Ensemble prediction + confusion, two stages for parallelism:
//   stage 1: one thread per (pair, tree-block of PREDICT_TREE_BLOCK) —
//            partial fp64 probability sums (sequential within the block);
//   stage 2: one thread per pair — blocks summed in ASCENDING order
//            (deterministic; forest_ref.predict_forest uses the same
//            association), then the confusion atomics
//            (k = 2*y + pred - 1, true negatives skipped; reference
//            experiment.py:476-483).
// ---------------------------------------------------------------------------
#define PREDICT_TREE_BLOCK 10

__global__ void predict_partial_kernel(
    const uint8_t* __restrict__ codes_test,   // [M, FPAD]
    const int* __restrict__ pair_row,         // [P]
    const int* __restrict__ pair_fold,        // [P]
    int n_pairs,
    const long* __restrict__ j_node_off,      // [J]
    const int* __restrict__ nfeat, const int* __restrict__ nsplit,
    const int* __restrict__ nleft,
    const float* __restrict__ ncnt0, const float* __restrict__ ncnt1,
    int trees_per_fold, int n_blocks,
    double* __restrict__ partial /* [P, n_blocks, 2] */) {
    const long total = (long)n_pairs * n_blocks;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int p = (int)(idx % n_pairs);
    const int tb = (int)(idx / n_pairs);

    const int row = pair_row[p];
    const int fold = pair_fold[p];
    const uint8_t* cr = codes_test + (size_t)row * FPAD;

    const int t0 = tb * PREDICT_TREE_BLOCK;
    const int t1 = min(trees_per_fold, t0 + PREDICT_TREE_BLOCK);
    double acc0 = 0.0, acc1 = 0.0;
    for (int t = t0; t < t1; ++t) {
        const long nbase = j_node_off[fold * trees_per_fold + t];
        int node = 0;
        int f = nfeat[nbase];
        while (f != LEAF_SENTINEL) {
            int go_right = (int)cr[f] > nsplit[nbase + node];
            node = nleft[nbase + node] + go_right;
            f = nfeat[nbase + node];
        }
        const double c0 = (double)ncnt0[nbase + node];
        const double c1 = (double)ncnt1[nbase + node];
        const double tot = c0 + c1;
        acc0 += c0 / tot;
        acc1 += c1 / tot;
    }
    partial[((size_t)p * n_blocks + tb) * 2 + 0] = acc0;
    partial[((size_t)p * n_blocks + tb) * 2 + 1] = acc1;
}

__global__ void predict_combine_kernel(
    const uint8_t* __restrict__ y_test,       // [M]
    const int* __restrict__ proj_id,          // [M]
    const int* __restrict__ pair_row, int n_pairs,
    const double* __restrict__ partial, int n_blocks,
    uint8_t* __restrict__ pred_out,
    int* __restrict__ confusion, int n_proj) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    double acc0 = 0.0, acc1 = 0.0;
    for (int tb = 0; tb < n_blocks; ++tb) {
        acc0 += partial[((size_t)p * n_blocks + tb) * 2 + 0];
        acc1 += partial[((size_t)p * n_blocks + tb) * 2 + 1];
    }
    const int pred = acc1 > acc0;
    pred_out[p] = (uint8_t)pred;
    const int row = pair_row[p];
    const int k = 2 * (int)y_test[row] + pred - 1;
    if (k >= 0) {
        atomicAdd(&confusion[proj_id[row] * 3 + k], 1);
        atomicAdd(&confusion[n_proj * 3 + k], 1);
    }
}
