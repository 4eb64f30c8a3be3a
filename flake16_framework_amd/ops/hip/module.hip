// Torch-extension host layer for the flake16 MI355X kernels.
//
// Single translation unit: includes the kernel files and exposes
// tensor-based entry points.  Compiled by hipcc for gfx950 with
// -ffp-contract=off (bit-parity of fp64 split scores / fp32 SMOTE
// interpolation with the numpy reference).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

#include "forest.hip"
#include "knn_balance.hip"
#include "scaler_pca.hip"
#include "treeshap.hip"
#include "detect.hip"
#include "detector_shap.hip"
#include "holdout.hip"
#include "importance.hip"
#include "dependence.hip"
#include "similar.hip"

#include <vector>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#define CHECK_HIP(expr)                                                     \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        TORCH_CHECK(_e == hipSuccess, "HIP error: ",                        \
                    hipGetErrorString(_e));                                 \
    } while (0)

static hipStream_t current_stream() {
    return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

// ---------------------------------------------------------------------------
// forest_fit
// ---------------------------------------------------------------------------
// Core fit over a batch of jobs with PER-JOB model spec (max_features,
// splitter, bootstrap) — one call can build a whole balance group's
// DT + RF + ET forests in a single level pipeline.
static std::vector<at::Tensor> forest_fit_impl(
    at::Tensor codes, at::Tensor labels, at::Tensor j_row_off,
    at::Tensor j_n, at::Tensor j_key, at::Tensor j_mf, at::Tensor j_rand,
    at::Tensor j_boot, int64_t F, int64_t seed) {
    TORCH_CHECK(codes.is_cuda() && codes.dtype() == at::kByte &&
                codes.size(1) == FPAD && codes.is_contiguous());
    TORCH_CHECK(labels.is_cuda() && labels.dtype() == at::kByte);
    const at::cuda::OptionalCUDAGuard guard(codes.device());

    const int J = j_n.size(0);
    auto opts_i32 = codes.options().dtype(at::kInt);
    auto opts_i64 = codes.options().dtype(at::kLong);
    auto opts_f32 = codes.options().dtype(at::kFloat);

    // Job arrays may arrive CPU-resident (preferred: the host needs
    // j_n / j_rand values for sizing and kernel selection, and device
    // tensors would force blocking D2H copies here)
    auto j_n_cpu = j_n.is_cuda() ? j_n.to(at::kCPU) : j_n;
    auto j_n_dev = j_n.is_cuda() ? j_n : j_n.to(codes.device());
    auto j_rand_cpu = j_rand.is_cuda() ? j_rand.to(at::kCPU) : j_rand;
    auto j_rand_dev = j_rand.is_cuda() ? j_rand : j_rand.to(codes.device());
    auto j_mf_dev = j_mf.is_cuda() ? j_mf : j_mf.to(codes.device());
    auto j_boot_dev = j_boot.is_cuda() ? j_boot : j_boot.to(codes.device());
    const int* jn = j_n_cpu.data_ptr<int>();
    const uint8_t* jr = j_rand_cpu.data_ptr<uint8_t>();
    bool any_rand = false, any_best = false;
    for (int j = 0; j < J; ++j)
        (jr[j] ? any_rand : any_best) = true;
    std::vector<long> sidx_off(J), node_off(J);
    long S = 0, Ntot = 0;
    bool has_wide = false;   // any node >= 2^16 samples needs the WIDE path
    for (int j = 0; j < J; ++j) {
        has_wide |= jn[j] >= 65536;
        sidx_off[j] = S;
        node_off[j] = Ntot;
        S += jn[j];
        Ntot += 2L * jn[j] + 1;
    }
    TORCH_CHECK(S > 0, "empty forest_fit batch");

    auto j_sidx_off = at::from_blob(sidx_off.data(), {J}, at::kLong)
                          .to(codes.device());
    auto j_node_off = at::from_blob(node_off.data(), {J}, at::kLong)
                          .to(codes.device());

    // Workspace sizes are rounded to a coarse granularity so cells of
    // similar size hit the same caching-allocator buckets: per-cell
    // workspaces here reach GBs at large N, and exact (per-balance-group)
    // sizes would force hipMalloc/hipFree churn — whose device syncs
    // serialize the concurrent cell streams (measured: the N=40k sweep
    // ran at ~79% single-stream occupancy before this).
    const long GRAN = 1L << 23;
    const long S_alloc = (S + GRAN - 1) / GRAN * GRAN;
    const long Ntot_alloc = (Ntot + GRAN - 1) / GRAN * GRAN;

    // No global sentinel fill (it was 1 GB/group at large N): every
    // allocated node is written LEAF_SENTINEL at allocation time (root in
    // forest_init_kernel, children at their parent's split), and the
    // other node fields are written for every reached node before any
    // read — so plain at::empty suffices for all five arrays.
    auto nfeat = at::empty({Ntot_alloc}, opts_i32);
    auto nsplit = at::empty({Ntot_alloc}, opts_i32);
    auto nleft = at::empty({Ntot_alloc}, opts_i32);
    auto ncnt0 = at::empty({Ntot_alloc}, opts_f32);
    auto ncnt1 = at::empty({Ntot_alloc}, opts_f32);
    auto node_alloc = at::zeros({J}, opts_i32);

    auto sidx_a = at::empty({S_alloc}, opts_i32);
    auto sidx_b = at::empty({S_alloc}, opts_i32);

    // Histogram-subtraction pools (see forest.hip): sized for the worst
    // per-level allocation, 2 slots per splitting node >= HIST_SAVE_MIN.
    // Larger batches raise the subtraction threshold: with the pool
    // clamped at 131072 slots, small thresholds exhaust it mid-band and
    // the 16 KiB/slot store+load traffic overtakes the saved
    // re-accumulation (measured at N=40k fused: 23.0 -> 15.3 s with
    // 8192).
    int HIST_SAVE_MIN = S < (1L << 24) ? 2048 : 8192;
    if (const char* e = getenv("FLAKE16_HIST_SAVE_MIN"))
        HIST_SAVE_MIN = atoi(e);
    // cap bounds pool memory at ~2 GB per parity (16 KiB per slot);
    // exhaustion is correct but silently degrades to full accumulation
    const long pool_cap =
        std::min<long>(2 * (S_alloc / HIST_SAVE_MIN) + 8, 131072);

    // Level work queue: only nodes > MID_N samples (disjoint: <= S/MID_N)
    // plus <= MID_N children carrying a subtraction slot (<= 2 per pool
    // slot) and the J roots; overflow trips err_flag loudly.
    const long work_cap = S_alloc / MID_N + 2 * pool_cap + J + 64;
    auto work_a = at::empty({work_cap * (long)sizeof(WorkItem)},
                            codes.options().dtype(at::kByte));
    auto work_b = at::empty({work_cap * (long)sizeof(WorkItem)},
                            codes.options().dtype(at::kByte));
    // per-level counter state, one 8 B memset per level:
    // state[parity*4 + 0] = work count, +1 = pool count.
    // Fixed slots outside the parity state, accumulating over the fit:
    // state[8] = small count, state[9] = mid count.
    auto state = at::zeros({12}, opts_i32);
    auto err = at::zeros({1}, opts_i32);

    // Small queue: disjoint <= SMALL_N subtrees, accumulated until the
    // host drains it; S/4 covers any non-adversarial fit (the drain
    // threshold below and err_flag guard the theoretical S bound).
    const long small_cap = S_alloc / 4 + 1024;
    auto small_q = at::empty({small_cap * (long)sizeof(WorkItem)},
                             codes.options().dtype(at::kByte));

    // mid-subtree queue: disjoint ranges of > SMALL_N samples each, so
    // even a whole fit's items cannot exceed S / (SMALL_N + 1)
    const long mid_cap = S_alloc / (SMALL_N + 1) + 64;
    auto mid_q = at::empty({mid_cap * (long)sizeof(WorkItem)},
                           codes.options().dtype(at::kByte));
    auto hist_pool0 = at::empty({pool_cap * FPAD * 256},
                                codes.options().dtype(at::kInt));
    auto hist_pool1 = at::empty({pool_cap * FPAD * 256},
                                codes.options().dtype(at::kInt));

    hipStream_t stream = current_stream();

    forest_init_kernel<<<J, HBLK, 0, stream>>>(
        j_row_off.data_ptr<int>(), j_n_dev.data_ptr<int>(),
        j_sidx_off.data_ptr<long>(), j_key.data_ptr<int>(),
        j_node_off.data_ptr<long>(), nfeat.data_ptr<int>(),
        node_alloc.data_ptr<int>(), sidx_a.data_ptr<int>(),
        (WorkItem*)work_a.data_ptr(), j_boot_dev.data_ptr<uint8_t>(),
        (uint32_t)seed);
    state.narrow(0, 0, 1).fill_((int)J);

    const int PINSZ = 64;
    auto pinned = at::empty({PINSZ}, at::TensorOptions()
                                         .dtype(at::kInt)
                                         .pinned_memory(true));
    int* pinned_p = pinned.data_ptr<int>();

    ForestDev a{};
    a.codes = codes.data_ptr<uint8_t>();
    a.labels = labels.data_ptr<uint8_t>();
    a.j_row_off = j_row_off.data_ptr<int>();
    a.j_n = j_n_dev.data_ptr<int>();
    a.j_sidx_off = j_sidx_off.data_ptr<long>();
    a.j_node_off = j_node_off.data_ptr<long>();
    a.j_key = j_key.data_ptr<int>();
    a.node_alloc = node_alloc.data_ptr<int>();
    a.nfeat = nfeat.data_ptr<int>();
    a.nsplit = nsplit.data_ptr<int>();
    a.nleft = nleft.data_ptr<int>();
    a.ncnt0 = ncnt0.data_ptr<float>();
    a.ncnt1 = ncnt1.data_ptr<float>();
    a.err_flag = err.data_ptr<int>();
    a.F = (int)F;
    a.j_mf = j_mf_dev.data_ptr<int>();
    a.j_rand = j_rand_dev.data_ptr<uint8_t>();
    a.seed = (uint32_t)seed;
    a.work_cap = (int)work_cap;
    a.hist_pool0 = (uint32_t*)hist_pool0.data_ptr<int>();
    a.hist_pool1 = (uint32_t*)hist_pool1.data_ptr<int>();
    a.pool_cap = (int)pool_cap;
    a.hist_save_min = HIST_SAVE_MIN;
    a.small = (WorkItem*)small_q.data_ptr();
    a.small_cap = (int)small_cap;
    a.mid = (WorkItem*)mid_q.data_ptr();
    a.mid_cap = (int)mid_cap;
    a.sidx_a = sidx_a.data_ptr<int>();
    a.sidx_b = sidx_b.data_ptr<int>();
    int* st = state.data_ptr<int>();
    a.pool_count = st + 1;   // kernel indexes [wp * 4]
    a.small_count = st + 8;
    a.mid_count = st + 9;
    // wave-parallel mid-subtree mode (per-item: jobs with
    // max_features <= WAVE_CANDS); the env var forces the block-serial
    // DFS for same-box A/B runs
    a.wave_mid = getenv("FLAKE16_NO_WAVE_MID") ? 0 : 1;

    int GRID = 4096;
    if (const char* e = getenv("FLAKE16_FIT_GRID")) GRID = atoi(e);
    // STAGED keeps code rows in LDS (2 blocks/CU); the unstaged variant
    // reads them through L1/L2 and doubles the resident blocks — A/B via
    // FLAKE16_MID_UNSTAGED=1.
    const bool mid_staged = !getenv("FLAKE16_MID_UNSTAGED");

    // Adaptive level grids: the deep tail of the band (skewed-split
    // chains) has a handful of items per level, where scheduling the
    // full 4096-block grid of empty blocks is the dominant cost; once the
    // synced queue count is tiny the next chunk launches small grids
    // (grid-stride loops keep any count correct regardless).
    int lv_grid = GRID, sub_grid = 2048;

    // Drain schedule.  Mid and small items are terminal — they never feed
    // the level queue — and their sample ranges stay valid in their tagged
    // buffer (see route_child), so nothing forces a drain per level.  By
    // default the level loop runs only the split kernels and the two
    // queues accumulate; they are drained once after the band is
    // exhausted (mid first: it farms into the small queue).  The old
    // per-level drain paid the slowest block's whole subtree as a
    // critical path at every level (profiles/deferred_subtree_drain.md).
    // FLAKE16_LEVEL_DRAIN=1 keeps that schedule for same-box A/B runs and
    // the equivalence test.
    const bool level_drain = getenv("FLAKE16_LEVEL_DRAIN") != nullptr;
    // Capacity safety: the accumulated counts are synced with every chunk
    // and a queue above its threshold is drained and reset mid-band.
    // FLAKE16_DRAIN_AT=<items> lowers both thresholds (tests: the 8M-sample
    // workspace rounding makes the real caps unreachable at small sizes).
    long small_drain_at = small_cap / 2, mid_drain_at = mid_cap / 2;
    if (const char* e = getenv("FLAKE16_DRAIN_AT"))
        small_drain_at = mid_drain_at = atol(e);
    const bool drain_stats = getenv("FLAKE16_DRAIN_STATS") != nullptr;
    long n_drains = 0;

    auto launch_mid = [&](int grid) {
        if (mid_staged)
            mid_subtree_kernel<true><<<grid, HBLK, 0, stream>>>(a);
        else
            mid_subtree_kernel<false><<<grid, HBLK, 0, stream>>>(a);
    };

    // Drain both queues given their synced counts: one block per mid item
    // and one wave per small item (the mid kernel farms more small items
    // than the host has seen: allow 16 per mid item), capped at 2048
    // blocks, beyond which the grid-stride loops take over.  Measured:
    // uncapped per-item grids (up to 65536 blocks, balanced by the
    // hardware dispatcher) were 3.5 % slower over the sweep than this cap
    // (profiles/deferred_subtree_drain.md); FLAKE16_DRAIN_GRID=<blocks>
    // overrides it for A/B runs.
    long drain_grid = 2048;
    if (const char* e = getenv("FLAKE16_DRAIN_GRID"))
        drain_grid = std::max<long>(1, atol(e));
    auto drain = [&](long n_small, long n_mid) {
        if (n_mid > 0)
            launch_mid((int)std::min<long>(n_mid, drain_grid));
        if (n_mid > 0 || n_small > 0) {
            const long waves = n_small + 16 * n_mid;
            small_subtree_kernel<<<
                (int)std::min<long>((waves + 3) / 4, drain_grid), HBLK, 0,
                stream>>>(a);
        }
        ++n_drains;
        if (drain_stats) {
            int after[2];
            CHECK_HIP(hipMemcpyAsync(after, st + 8, 8,
                                     hipMemcpyDeviceToHost, stream));
            CHECK_HIP(hipStreamSynchronize(stream));
            fprintf(stderr,
                    "forest_fit drain %ld: S=%ld mid=%ld/%ld small=%d/%ld "
                    "(%ld before the mid drain)\n",
                    n_drains, S, n_mid, mid_cap, after[0], small_cap,
                    n_small);
        }
    };

    // One level's dispatches: clear next-parity counters, split kernel(s),
    // next-level count -> pinned slot.
    auto level_ops = [&](int cur_par, int pinned_slot) {
        const int nx = cur_par ^ 1;
        // one 8 B memset clears the next level's work and pool counts
        CHECK_HIP(hipMemsetAsync(st + nx * 4, 0, 8, stream));
        if (level_drain)
            CHECK_HIP(hipMemsetAsync(st + 8, 0, 8, stream));
        a.sidx_cur = (cur_par == 0 ? sidx_a : sidx_b).data_ptr<int>();
        a.sidx_nxt = (cur_par == 0 ? sidx_b : sidx_a).data_ptr<int>();
        a.cur = (const WorkItem*)(cur_par == 0 ? work_a : work_b).data_ptr();
        a.nxt = (WorkItem*)(cur_par == 0 ? work_b : work_a).data_ptr();
        a.cur_count = st + cur_par * 4;
        a.nxt_count = st + nx * 4;
        if (any_best) {
            hist_split_kernel<false><<<lv_grid, HBLK, 0, stream>>>(a);
            if (has_wide)
                hist_split_kernel<true><<<lv_grid, HBLK, 0, stream>>>(a);
        }
        if (any_rand)
            et_split_kernel<<<lv_grid, HBLK, 0, stream>>>(a);
        if (level_drain) {
            launch_mid(sub_grid);
            small_subtree_kernel<<<sub_grid, HBLK, 0, stream>>>(a);
        }
        CHECK_HIP(hipMemcpyAsync(pinned_p + pinned_slot, st + nx * 4, 4,
                                 hipMemcpyDeviceToHost, stream));
    };

    const int CHUNK = 8;
    int* const pinned_q = pinned_p + CHUNK;   // [0] small, [1] mid count
    int cur = 0;
    long lev = 0;
    bool done = false;
    while (!done) {
        for (int c = 0; c < CHUNK; ++c, ++lev) {
            level_ops(cur, c);
            cur ^= 1;
        }
        if (!level_drain)
            CHECK_HIP(hipMemcpyAsync(pinned_q, st + 8, 8,
                                     hipMemcpyDeviceToHost, stream));
        CHECK_HIP(hipStreamSynchronize(stream));
        for (int c = 0; c < CHUNK; ++c)
            if (pinned_p[c] == 0) { done = true; break; }
        // shrink the next chunk's grids when the band has thinned
        // (items can at most double per level: 16 items now bound
        // the whole next chunk well under a 512-block grid)
        const int last_cnt = pinned_p[CHUNK - 1];
        lv_grid = last_cnt <= 16 ? 512 : GRID;
        sub_grid = last_cnt <= 16 ? 512 : 2048;
        TORCH_CHECK(lev < 8192, "forest_fit: depth limit exceeded");
        if (!level_drain && !done &&
            (pinned_q[0] > small_drain_at || pinned_q[1] > mid_drain_at)) {
            drain(pinned_q[0], pinned_q[1]);
            CHECK_HIP(hipMemsetAsync(st + 8, 0, 8, stream));
        }
    }
    // band exhausted: the one drain of everything deferred
    if (!level_drain)
        drain(pinned_q[0], pinned_q[1]);

    TORCH_CHECK(err.to(at::kCPU).item<int>() == 0,
                "forest_fit: work-queue capacity exceeded");

    return {nfeat, nsplit, nleft, ncnt0, ncnt1, j_node_off, node_alloc};
}

// Uniform-spec compatibility surface (single-model batches).
std::vector<at::Tensor> forest_fit(
    at::Tensor codes, at::Tensor labels, at::Tensor j_row_off,
    at::Tensor j_n, at::Tensor j_key, int64_t F, int64_t max_features,
    bool bootstrap, bool splitter_random, int64_t seed) {
    const int J = j_n.size(0);
    auto mf = at::full({J}, (int)max_features, at::kInt);
    auto rnd = at::full({J}, splitter_random ? 1 : 0, at::kByte);
    auto boot = at::full({J}, bootstrap ? 1 : 0, at::kByte);
    return forest_fit_impl(codes, labels, j_row_off, j_n, j_key, mf, rnd,
                           boot, F, seed);
}

// Mixed-spec batches (fused balance-group fits).
std::vector<at::Tensor> forest_fit_multi(
    at::Tensor codes, at::Tensor labels, at::Tensor j_row_off,
    at::Tensor j_n, at::Tensor j_key, at::Tensor j_mf, at::Tensor j_rand,
    at::Tensor j_boot, int64_t F, int64_t seed) {
    return forest_fit_impl(codes, labels, j_row_off, j_n, j_key, j_mf,
                           j_rand, j_boot, F, seed);
}

// ---------------------------------------------------------------------------
// forest_predict_confusion
// ---------------------------------------------------------------------------
std::vector<at::Tensor> forest_predict_confusion(
    at::Tensor codes_test, at::Tensor y_test, at::Tensor proj_id,
    at::Tensor pair_row, at::Tensor pair_fold, at::Tensor j_node_off,
    at::Tensor nfeat, at::Tensor nsplit, at::Tensor nleft,
    at::Tensor ncnt0, at::Tensor ncnt1, int64_t trees_per_fold,
    int64_t n_proj) {
    const at::cuda::OptionalCUDAGuard guard(codes_test.device());
    const int P = pair_row.size(0);
    const int n_blocks =
        ((int)trees_per_fold + PREDICT_TREE_BLOCK - 1) / PREDICT_TREE_BLOCK;
    auto pred = at::zeros({P}, codes_test.options().dtype(at::kByte));
    auto confusion = at::zeros({n_proj + 1, 3},
                               codes_test.options().dtype(at::kInt));
    auto partial = at::empty({(long)P * n_blocks * 2},
                             codes_test.options().dtype(at::kDouble));
    hipStream_t s = current_stream();
    const long total = (long)P * n_blocks;
    predict_partial_kernel<<<(int)((total + 255) / 256), 256, 0, s>>>(
        codes_test.data_ptr<uint8_t>(), pair_row.data_ptr<int>(),
        pair_fold.data_ptr<int>(), P, j_node_off.data_ptr<long>(),
        nfeat.data_ptr<int>(), nsplit.data_ptr<int>(),
        nleft.data_ptr<int>(), ncnt0.data_ptr<float>(),
        ncnt1.data_ptr<float>(), (int)trees_per_fold, n_blocks,
        partial.data_ptr<double>());
    predict_combine_kernel<<<(P + 255) / 256, 256, 0, s>>>(
        y_test.data_ptr<uint8_t>(), proj_id.data_ptr<int>(),
        pair_row.data_ptr<int>(), P, partial.data_ptr<double>(), n_blocks,
        pred.data_ptr<uint8_t>(), confusion.data_ptr<int>(), (int)n_proj);
    return {pred, confusion};
}

// ---------------------------------------------------------------------------
// knn / balancing / binning
// ---------------------------------------------------------------------------
// Shared implementation: MFMA two-phase kernel by default (matrix cores
// compute the fp32 distance filter; survivors are re-checked in exact
// fp64 — output bits identical to the scalar kernels), scalar tile
// kernels under FLAKE16_NO_MFMA_KNN=1 for A/B runs.
static at::Tensor knn_run(at::Tensor X, at::Tensor seg_off, const int* so,
                          int n_seg, int64_t k, bool skip_identity) {
    const int R = X.size(0);
    hipStream_t stream = current_stream();
    auto out = at::empty({R, k}, X.options().dtype(at::kInt));

    if (getenv("FLAKE16_NO_MFMA_KNN")) {
        std::vector<int> blk(n_seg + 1);
        blk[0] = 0;
        for (int s = 0; s < n_seg; ++s) {
            int n = so[s + 1] - so[s];
            blk[s + 1] = blk[s] + (n + KNN_BLK - 1) / KNN_BLK;
        }
        auto seg_blk = at::from_blob(blk.data(), {n_seg + 1}, at::kInt)
                           .to(X.device());
        if (blk[n_seg] > 0)
            knn_segmented_kernel<<<blk[n_seg], KNN_BLK, 0, stream>>>(
                X.data_ptr<float>(), seg_off.data_ptr<int>(),
                seg_blk.data_ptr<int>(), n_seg, (int)k,
                skip_identity ? 1 : 0, out.data_ptr<int>());
        return out;
    }

    std::vector<int> blk(n_seg + 1);
    blk[0] = 0;
    for (int s = 0; s < n_seg; ++s) {
        int n = so[s + 1] - so[s];
        blk[s + 1] = blk[s] + (n + 63) / 64;
    }
    auto seg_blk = at::from_blob(blk.data(), {n_seg + 1}, at::kInt)
                       .to(X.device());
    auto norms = at::empty({R}, X.options());
    auto fb_list = at::empty({R}, X.options().dtype(at::kInt));
    auto fb_count = at::zeros({1 + n_seg}, X.options().dtype(at::kInt));
    auto fb_off = at::empty({n_seg + 1}, X.options().dtype(at::kInt));
    auto fb_cursor = at::empty({n_seg}, X.options().dtype(at::kInt));
    const long fb_cap = (long)R + (long)KNN_BLK * n_seg;
    auto fb_sorted = at::empty({fb_cap}, X.options().dtype(at::kInt));

    knn_norms_kernel<<<(R + 255) / 256, 256, 0, stream>>>(
        X.data_ptr<float>(), R, norms.data_ptr<float>());
    if (blk[n_seg] > 0) {
        knn_mfma_kernel<<<blk[n_seg], KNN_BLK, 0, stream>>>(
            X.data_ptr<float>(), seg_off.data_ptr<int>(),
            seg_blk.data_ptr<int>(), n_seg, (int)k, skip_identity ? 1 : 0,
            norms.data_ptr<float>(), out.data_ptr<int>(),
            fb_list.data_ptr<int>(), fb_count.data_ptr<int>());
        // regroup flagged queries by segment (256-padded) and re-scan
        // them exactly with LDS candidate tiling; all plumbing is
        // device-bounded — when nothing was flagged these kernels are
        // a few empty dispatches
        knn_fb_scan_kernel<<<1, 1, 0, stream>>>(
            fb_count.data_ptr<int>(), n_seg, fb_off.data_ptr<int>(),
            fb_cursor.data_ptr<int>());
        knn_fb_fill_kernel<<<(int)((fb_cap + 255) / 256), 256, 0, stream>>>(
            fb_off.data_ptr<int>(), n_seg, fb_sorted.data_ptr<int>());
        knn_fb_scatter_kernel<<<(R + 255) / 256, 256, 0, stream>>>(
            fb_list.data_ptr<int>(), fb_count.data_ptr<int>(),
            seg_off.data_ptr<int>(), n_seg, fb_off.data_ptr<int>(),
            fb_cursor.data_ptr<int>(), fb_sorted.data_ptr<int>());
        knn_fallback_kernel<<<(int)((fb_cap + KNN_BLK - 1) / KNN_BLK),
                              KNN_BLK, 0, stream>>>(
            X.data_ptr<float>(), seg_off.data_ptr<int>(), n_seg, (int)k,
            skip_identity ? 1 : 0, fb_sorted.data_ptr<int>(),
            fb_off.data_ptr<int>(), out.data_ptr<int>());
    }
    if (getenv("FLAKE16_KNN_DEBUG")) {
        const int fb = fb_count.narrow(0, 0, 1).to(at::kCPU).item<int>();
        fprintf(stderr, "[knn] R=%d n_seg=%d k=%ld fallback=%d\n",
                R, n_seg, (long)k, fb);
    }
    return out;
}

at::Tensor knn(at::Tensor X, int64_t k, bool skip_identity) {
    const at::cuda::OptionalCUDAGuard guard(X.device());
    TORCH_CHECK(X.is_cuda() && X.dtype() == at::kFloat &&
                X.size(1) == FPAD && X.is_contiguous());
    TORCH_CHECK(k >= 1 && k <= KMAX);
    const int n = X.size(0);
    int so[2] = {0, n};
    auto seg_off = at::from_blob(so, {2}, at::kInt).to(X.device());
    return knn_run(X, seg_off, so, 1, k, skip_identity);
}

at::Tensor knn_segmented(at::Tensor X, at::Tensor seg_off, int64_t k,
                         bool skip_identity) {
    const at::cuda::OptionalCUDAGuard guard(X.device());
    TORCH_CHECK(X.is_cuda() && X.dtype() == at::kFloat &&
                X.size(1) == FPAD && X.is_contiguous());
    TORCH_CHECK(k >= 1 && k <= KMAX);
    const int n_seg = seg_off.size(0) - 1;
    auto seg_off_cpu = seg_off.to(at::kCPU);
    return knn_run(X, seg_off, seg_off_cpu.data_ptr<int>(), n_seg, k,
                   skip_identity);
}

at::Tensor smote_interpolate(at::Tensor X, at::Tensor min_rows,
                             at::Tensor nn, int64_t n_new, int64_t k0,
                             int64_t k1) {
    const at::cuda::OptionalCUDAGuard guard(X.device());
    const int n_min = min_rows.size(0);
    const int k = nn.size(1);
    auto out = at::empty({n_new, FPAD}, X.options());
    const int grid = (n_new + 255) / 256;
    smote_kernel<<<grid, 256, 0, current_stream()>>>(
        X.data_ptr<float>(), min_rows.data_ptr<int>(), nn.data_ptr<int>(),
        n_min, k, (int)n_new, (uint32_t)k0, (uint32_t)k1,
        out.data_ptr<float>());
    return out;
}

at::Tensor enn_keep(at::Tensor y, at::Tensor nn, int64_t n_neighbors,
                    int64_t maj_label, bool clean_all) {
    const at::cuda::OptionalCUDAGuard guard(y.device());
    const int n = y.size(0);
    auto keep = at::empty({n}, y.options());
    const int grid = (n + 255) / 256;
    enn_keep_kernel<<<grid, 256, 0, current_stream()>>>(
        y.data_ptr<uint8_t>(), nn.data_ptr<int>(), n, (int)nn.size(1),
        (int)n_neighbors, (int)maj_label, clean_all ? 1 : 0,
        keep.data_ptr<uint8_t>());
    return keep;
}

at::Tensor tomek_keep(at::Tensor y, at::Tensor nn1, int64_t maj_label,
                      bool remove_all) {
    const at::cuda::OptionalCUDAGuard guard(y.device());
    const int n = y.size(0);
    auto keep = at::empty({n}, y.options());
    const int grid = (n + 255) / 256;
    tomek_keep_kernel<<<grid, 256, 0, current_stream()>>>(
        y.data_ptr<uint8_t>(), nn1.data_ptr<int>(), n, (int)maj_label,
        remove_all ? 1 : 0, keep.data_ptr<uint8_t>());
    return keep;
}

at::Tensor bin_codes_dev(at::Tensor X, at::Tensor cuts, at::Tensor cut_off,
                         int64_t F) {
    const at::cuda::OptionalCUDAGuard guard(X.device());
    const int n = X.size(0);
    auto codes = at::zeros({n, FPAD}, X.options().dtype(at::kByte));
    const int grid = (n + 255) / 256;
    bin_codes_kernel<<<grid, 256, 0, current_stream()>>>(
        X.data_ptr<float>(), cuts.data_ptr<float>(), cut_off.data_ptr<int>(),
        n, (int)F, codes.data_ptr<uint8_t>());
    return codes;
}

// ---------------------------------------------------------------------------
// scaler / pca  (fp64 in, fp64 out)
// ---------------------------------------------------------------------------
at::Tensor scaler_fit_transform_dev(at::Tensor X) {
    const at::cuda::OptionalCUDAGuard guard(X.device());
    TORCH_CHECK(X.dtype() == at::kDouble && X.size(1) == FPAD);
    const int n = X.size(0);
    auto mean = at::empty({FPAD}, X.options());
    auto scale = at::empty({FPAD}, X.options());
    auto out = at::empty_like(X);
    hipStream_t s = current_stream();
    col_mean_kernel<<<FPAD, RBLK, 0, s>>>(X.data_ptr<double>(), n,
                                          mean.data_ptr<double>());
    col_scale_kernel<<<FPAD, RBLK, 0, s>>>(X.data_ptr<double>(), n,
                                           mean.data_ptr<double>(),
                                           scale.data_ptr<double>());
    scale_transform_kernel<<<(n + 255) / 256, 256, 0, s>>>(
        X.data_ptr<double>(), n, mean.data_ptr<double>(),
        scale.data_ptr<double>(), out.data_ptr<double>());
    return out;
}

at::Tensor pca_fit_transform_dev(at::Tensor X, int64_t F) {
    const at::cuda::OptionalCUDAGuard guard(X.device());
    TORCH_CHECK(X.dtype() == at::kDouble && X.size(1) == FPAD);
    const int n = X.size(0);
    auto mean = at::empty({FPAD}, X.options());
    auto C = at::zeros({FPAD, FPAD}, X.options());
    auto V = at::zeros({FPAD, FPAD}, X.options());
    auto evals = at::zeros({FPAD}, X.options());
    auto T = at::empty_like(X);
    hipStream_t s = current_stream();
    col_mean_kernel<<<FPAD, RBLK, 0, s>>>(X.data_ptr<double>(), n,
                                          mean.data_ptr<double>());
    gram_kernel<<<FPAD * FPAD, RBLK, 0, s>>>(X.data_ptr<double>(), n,
                                             mean.data_ptr<double>(),
                                             C.data_ptr<double>());
    jacobi_eigen_kernel<<<1, 1, 0, s>>>(C.data_ptr<double>(),
                                        V.data_ptr<double>(),
                                        evals.data_ptr<double>(), (int)F);
    pca_project_kernel<<<(n + 255) / 256, 256, 0, s>>>(
        X.data_ptr<double>(), n, mean.data_ptr<double>(),
        V.data_ptr<double>(), (int)F, T.data_ptr<double>());
    pca_signflip_kernel<<<FPAD, RBLK, 0, s>>>(T.data_ptr<double>(), n,
                                              (int)F);
    return T;
}

// ---------------------------------------------------------------------------
// treeshap
// ---------------------------------------------------------------------------
at::Tensor treeshap(at::Tensor codes, at::Tensor j_node_off,
                    at::Tensor nfeat, at::Tensor nsplit, at::Tensor nleft,
                    at::Tensor ncnt0, at::Tensor ncnt1) {
    const at::cuda::OptionalCUDAGuard guard(codes.device());
    const int n_samples = codes.size(0);
    const int n_trees = j_node_off.size(0);
    hipStream_t s = current_stream();

    auto depth = at::zeros({n_trees}, codes.options().dtype(at::kInt));
    tree_depth_kernel<<<(n_trees + 63) / 64, 64, 0, s>>>(
        j_node_off.data_ptr<long>(), nfeat.data_ptr<int>(),
        nleft.data_ptr<int>(), n_trees, depth.data_ptr<int>());
    const int d_max = depth.max().to(at::kCPU).item<int>() + 1;

    int GRID = 2048;   // same-box sweep: 512/1024/2048/4096 -> 21.7/15.1/11.3/12.2 s
    if (const char* e = getenv("FLAKE16_SHAP_GRID")) GRID = atoi(e);
    const long n_threads = (long)GRID * SHAP_BLK;
    const long tri = (long)(d_max + 1) * (d_max + 2) / 2;
    auto path_ws = at::empty({n_threads * tri * (long)sizeof(PathElem)},
                             codes.options().dtype(at::kByte));
    auto frame_ws = at::empty(
        {n_threads * (d_max + 2) * (long)sizeof(ShapFrame)},
        codes.options().dtype(at::kByte));
    auto phi = at::zeros({n_samples, 16},
                         codes.options().dtype(at::kDouble));

    treeshap_kernel<<<GRID, SHAP_BLK, 0, s>>>(
        codes.data_ptr<uint8_t>(), n_samples, j_node_off.data_ptr<long>(),
        nfeat.data_ptr<int>(), nsplit.data_ptr<int>(),
        nleft.data_ptr<int>(), ncnt0.data_ptr<float>(),
        ncnt1.data_ptr<float>(), n_trees, d_max,
        (PathElem*)path_ws.data_ptr(), (ShapFrame*)frame_ws.data_ptr(),
        phi.data_ptr<double>());
    return phi;
}

at::Tensor treeshap_paths(at::Tensor codes, at::Tensor leaf_tree,
                          at::Tensor leaf_off, at::Tensor path_nodes,
                          at::Tensor j_node_off, at::Tensor nfeat,
                          at::Tensor nsplit, at::Tensor nleft,
                          at::Tensor ncnt0, at::Tensor ncnt1) {
    const at::cuda::OptionalCUDAGuard guard(codes.device());
    const int n_samples = codes.size(0);
    const int n_leaves = leaf_tree.size(0);
    auto phi = at::zeros({n_samples, 16},
                         codes.options().dtype(at::kDouble));
    treeshap_paths_kernel<<<2048, SHAP_BLK, 0, current_stream()>>>(
        codes.data_ptr<uint8_t>(), n_samples, leaf_tree.data_ptr<int>(),
        leaf_off.data_ptr<int>(), path_nodes.data_ptr<int>(),
        j_node_off.data_ptr<long>(), nfeat.data_ptr<int>(),
        nsplit.data_ptr<int>(), nleft.data_ptr<int>(),
        ncnt0.data_ptr<float>(), ncnt1.data_ptr<float>(), n_leaves,
        phi.data_ptr<double>());
    return phi;
}

// ---------------------------------------------------------------------------
// checks and launch arithmetic the saved-detector ops share
// (detector_steps.h and the kernel files built on it)
// ---------------------------------------------------------------------------
static void check_raw_rows(const at::Tensor& X, int64_t F, const char* op) {
    TORCH_CHECK(X.is_cuda() && X.dtype() == at::kDouble && X.dim() == 2 &&
                X.size(1) == FPAD && X.is_contiguous() &&
                X.size(0) < (1L << 31), op,
                ": X must be device float64 [M, 16]");
    TORCH_CHECK(F >= 1 && F <= FPAD, op, ": F must be between 1 and 16");
}

static void check_codes(const at::Tensor& codes, const char* op) {
    TORCH_CHECK(codes.is_cuda() && codes.dtype() == at::kByte &&
                codes.dim() == 2 && codes.size(1) == FPAD &&
                codes.is_contiguous() && codes.size(0) < (1L << 31), op,
                ": codes must be device uint8 [M, 16]");
}

static void check_labels(const at::Tensor& labels, long M, const char* op) {
    TORCH_CHECK(labels.is_cuda() && labels.dtype() == at::kByte &&
                labels.dim() == 1 && labels.is_contiguous() &&
                labels.numel() == M, op, ": labels must be device uint8 [M]");
}

// D packed forests of n_trees trees each, back to back: the
// root ids of forest d are tree_off[d * n_trees ..], node ids are global.
// The caller guarantees well-formed forests (engine/detector.py validates
// child ids before packing); shapes are checked here.
static void check_forest(const at::Tensor& tree_off,
                         const at::Tensor& nodes_packed, long D,
                         int64_t n_trees, long max_trees, const char* op) {
    TORCH_CHECK(tree_off.is_cuda() && tree_off.dtype() == at::kLong &&
                tree_off.is_contiguous() && n_trees >= 1 &&
                n_trees <= max_trees &&
                tree_off.numel() == D * n_trees + 1, op,
                ": n_trees root ids per forest and an end");
    TORCH_CHECK(nodes_packed.is_cuda() && nodes_packed.dtype() == at::kInt &&
                nodes_packed.dim() == 2 && nodes_packed.size(1) == 2 &&
                nodes_packed.is_contiguous() &&
                nodes_packed.size(0) < (1L << 31), op,
                ": nodes must be device int32 [n_nodes, 2]");
}
// n_trees bound of holdout_proba, permuted_counts and partial_dependence
static const long MAX_GROUPED_TREES = (1L << 20) - 1;

static int n_tree_blocks(int64_t n_trees) {
    return ((int)n_trees + PREDICT_TREE_BLOCK - 1) / PREDICT_TREE_BLOCK;
}

// Grid of the kernels that give a wave per job (permuted_counts,
// partial_dependence): nb row blocks in x, and the `rounds` rounds of
// jobs (one job per wave of a block) split over blockIdx.y until the grid
// holds about four waves per SIMD (256 CUs x 4 SIMDs = 1024 blocks), never
// more shares than there are rounds and within the 65535 limit of grid.y.
static dim3 job_grid(long nb, long rounds) {
    const long want = (1024 + nb - 1) / nb;
    return dim3((unsigned)nb,
                (unsigned)std::max(1L, std::min({rounds, want, 65535L})));
}

// Host checks of G stacked parameter sets (CPU tensors): mean / scale /
// pca_mean [G, FPAD], W [G, FPAD, FPAD], cut_off [G, FPAD + 1] with
// group-local offsets into the groups' cuts, which lie back to back in
// `cuts`.  Returns cut_base int32 [G] (CPU), each group's first cut.
static at::Tensor grouped_params_check(const at::Tensor& mean,
                                       const at::Tensor& scale,
                                       const at::Tensor& pca_mean,
                                       const at::Tensor& W,
                                       const at::Tensor& cuts,
                                       const at::Tensor& cut_off, long G,
                                       const char* op) {
    for (const at::Tensor* p : {&mean, &scale, &pca_mean, &W})
        TORCH_CHECK(!p->is_cuda() && p->dtype() == at::kDouble &&
                    p->is_contiguous());
    TORCH_CHECK(mean.numel() == G * FPAD && scale.numel() == G * FPAD &&
                pca_mean.numel() == G * FPAD &&
                W.numel() == G * FPAD * FPAD,
                op, ": one parameter set per group");
    TORCH_CHECK(!cuts.is_cuda() && cuts.dtype() == at::kFloat &&
                cuts.is_contiguous());
    TORCH_CHECK(!cut_off.is_cuda() && cut_off.dtype() == at::kInt &&
                cut_off.is_contiguous() &&
                cut_off.numel() == G * (FPAD + 1));
    const int* co = cut_off.data_ptr<int>();
    auto cut_base = at::empty({G}, at::kInt);
    long n_cuts = 0;
    for (long g = 0; g < G; ++g, co += FPAD + 1) {
        TORCH_CHECK(co[0] == 0, op, ": cut offsets of group ", g,
                    " must start at 0");
        for (int f = 0; f < FPAD; ++f)
            TORCH_CHECK(co[f + 1] >= co[f] &&
                        co[f + 1] - co[f] <= DETECT_MAX_CUTS,
                        op, ": bad cut count for group ", g, " feature ", f);
        cut_base.data_ptr<int>()[g] = (int)n_cuts;
        n_cuts += co[FPAD];
        TORCH_CHECK(n_cuts < (1L << 31));
    }
    TORCH_CHECK(n_cuts == cuts.numel(), op,
                ": cut offsets do not cover the cut array");
    return cut_base;
}

// A checked parameter set on the device.  cuts_ptr() is null for a set
// without cuts (data_ptr of an empty tensor is not to be relied on).
struct DeviceParams {
    at::Tensor mean, scale, pca_mean, W, cuts, cut_off, cut_base;
    const float* cuts_ptr() const {
        return cuts.numel() ? cuts.data_ptr<float>() : nullptr;
    }
};

// cut_base may be undefined, for a kernel that serves one set.
static DeviceParams upload_params(const at::Tensor& mean,
                                  const at::Tensor& scale,
                                  const at::Tensor& pca_mean,
                                  const at::Tensor& W, const at::Tensor& cuts,
                                  const at::Tensor& cut_off,
                                  const at::Tensor& cut_base,
                                  c10::Device dev) {
    return {mean.to(dev), scale.to(dev), pca_mean.to(dev), W.to(dev),
            cuts.to(dev), cut_off.to(dev),
            cut_base.defined() ? cut_base.to(dev) : cut_base};
}

// ---------------------------------------------------------------------------
// saved-detector inference (detect.hip)
// ---------------------------------------------------------------------------
// Parameters and cuts arrive CPU-resident: they are a few KB, and the cut
// offsets are validated here before anything indexes LDS with them.
at::Tensor detect_encode(at::Tensor X, at::Tensor mean, at::Tensor scale,
                         at::Tensor pca_mean, at::Tensor W, bool has_pca,
                         at::Tensor cuts, at::Tensor cut_off, int64_t F) {
    const char* op = "detect_encode";
    check_raw_rows(X, F, op);
    grouped_params_check(mean, scale, pca_mean, W, cuts, cut_off, 1, op);

    const at::cuda::OptionalCUDAGuard guard(X.device());
    const long M = X.size(0);
    auto codes = at::empty({M, FPAD}, X.options().dtype(at::kByte));
    if (M == 0) return codes;
    auto p = upload_params(mean, scale, pca_mean, W, cuts, cut_off,
                           at::Tensor(), X.device());
    detect_encode_kernel<<<(int)((M + DETECT_BLK - 1) / DETECT_BLK),
                           DETECT_BLK, 0, current_stream()>>>(
        X.data_ptr<double>(), p.mean.data_ptr<double>(),
        p.scale.data_ptr<double>(), p.pca_mean.data_ptr<double>(),
        p.W.data_ptr<double>(), has_pca ? 1 : 0, p.cuts_ptr(),
        p.cut_off.data_ptr<int>(), (int)M, (int)F,
        codes.data_ptr<uint8_t>());
    return codes;
}

// (acc0, acc1) per row as float64 [M, 2].
at::Tensor forest_proba(at::Tensor codes, at::Tensor tree_off,
                        at::Tensor nodes_packed, int64_t n_trees) {
    const char* op = "forest_proba";
    check_codes(codes, op);
    check_forest(tree_off, nodes_packed, 1, n_trees, (1L << 31) - 1, op);
    const at::cuda::OptionalCUDAGuard guard(codes.device());
    const long M = codes.size(0);
    const int n_blocks = n_tree_blocks(n_trees);
    auto acc = at::empty({M, 2}, codes.options().dtype(at::kDouble));
    if (M == 0) return acc;
    auto partial = at::empty({(long)n_blocks * M, 2},
                             codes.options().dtype(at::kDouble));
    hipStream_t s = current_stream();
    const long total = M * n_blocks;
    forest_proba_partial_kernel<<<
        (int)((total + DETECT_BLK - 1) / DETECT_BLK), DETECT_BLK, 0, s>>>(
        codes.data_ptr<uint8_t>(), tree_off.data_ptr<long>(),
        (const int2*)nodes_packed.data_ptr<int>(), (int)M, (int)n_trees,
        n_blocks, (double2*)partial.data_ptr<double>());
    forest_proba_combine_kernel<<<(int)((M + DETECT_BLK - 1) / DETECT_BLK),
                                  DETECT_BLK, 0, s>>>(
        (const double2*)partial.data_ptr<double>(), (int)M, n_blocks,
        (double2*)acc.data_ptr<double>());
    return acc;
}

// ---------------------------------------------------------------------------
// saved-detector TreeSHAP and SHAP interaction values (detector_shap.hip)
// ---------------------------------------------------------------------------
// The checks the ops over the merged-path table share: shapes and dtypes
// on the host, then (when there are rows) everything a kernel indexes
// with, on the device, with one readback.
static void check_path_table(const char* op, const at::Tensor& codes,
                             const at::Tensor& tree_leaf_off,
                             const at::Tensor& leaf_off,
                             const at::Tensor& leaf_val,
                             const at::Tensor& elem_code,
                             const at::Tensor& elem_z, int64_t n_trees,
                             int64_t F) {
    check_codes(codes, op);
    TORCH_CHECK(F >= 1 && F <= FPAD);
    TORCH_CHECK(n_trees >= 1 && n_trees <= 65535, op,
                ": tree count out of range");
    for (const at::Tensor* p : {&tree_leaf_off, &leaf_off, &elem_code})
        TORCH_CHECK(p->is_cuda() && p->dtype() == at::kInt &&
                    p->dim() == 1 && p->is_contiguous());
    for (const at::Tensor* p : {&leaf_val, &elem_z})
        TORCH_CHECK(p->is_cuda() && p->dtype() == at::kDouble &&
                    p->dim() == 1 && p->is_contiguous());
    const long L = leaf_val.numel(), E = elem_z.numel();
    TORCH_CHECK(tree_leaf_off.numel() == n_trees + 1 &&
                leaf_off.numel() == L + 1 && elem_code.numel() == E &&
                L >= n_trees && L < (1L << 31) && E < (1L << 31),
                op, ": path table sizes");
    if (codes.size(0) == 0) return;

    // offsets start at 0, end at the array they index and never step
    // back; a tree owns a leaf, a leaf at most F elements, and every
    // element names a feature below F
    const at::cuda::OptionalCUDAGuard guard(codes.device());
    auto t_step = tree_leaf_off.diff();
    auto l_step = leaf_off.diff();
    auto ok = tree_leaf_off[0].eq(0) & tree_leaf_off[n_trees].eq(L) &
              t_step.ge(1).all() & leaf_off[0].eq(0) &
              leaf_off[L].eq(E) & l_step.ge(0).all() & l_step.le(F).all();
    if (E > 0)
        ok = ok & elem_code.bitwise_and(0xFF).lt(F).all();
    TORCH_CHECK(ok.item<bool>(), op, ": malformed path table");
}

// What the two ops over the table share past the checks: the workspace
// partial [T, G, FPAD, rows] (G = F slots g when PAIRS, else 1) bounded at
// 256 MiB, so rows go in chunks; per chunk the tree kernel, then
// combine(partial, row0, rows of the chunk, gx, stream), the op's own
// launch.  An empty element table is passed as null pointers.
template <bool PAIRS, typename Combine>
static void shap_row_chunks(const at::Tensor& codes,
                            const at::Tensor& tree_leaf_off,
                            const at::Tensor& leaf_off,
                            const at::Tensor& leaf_val,
                            const at::Tensor& elem_code,
                            const at::Tensor& elem_z, int64_t n_trees,
                            int64_t F, Combine combine) {
    const long M = codes.size(0), E = elem_z.numel();
    const long G = PAIRS ? F : 1;
    const long ws_cap = 256L << 20;
    const long per_row = n_trees * G * FPAD * (long)sizeof(double);
    long chunk = std::max<long>(EXPLAIN_BLK,
                                ws_cap / per_row / EXPLAIN_BLK * EXPLAIN_BLK);
    chunk = std::min(chunk, M);
    auto partial = at::empty({n_trees * G * FPAD * chunk},
                             codes.options().dtype(at::kDouble));
    hipStream_t s = current_stream();
    for (long row0 = 0; row0 < M; row0 += chunk) {
        const int mc = (int)std::min(chunk, M - row0);
        const int gx = (mc + EXPLAIN_BLK - 1) / EXPLAIN_BLK;
        detector_shap_tree_kernel<PAIRS>
            <<<dim3(gx, (int)n_trees, (int)G), EXPLAIN_BLK, 0, s>>>(
                codes.data_ptr<uint8_t>(), tree_leaf_off.data_ptr<int>(),
                leaf_off.data_ptr<int>(), leaf_val.data_ptr<double>(),
                E ? elem_code.data_ptr<int>() : nullptr,
                E ? elem_z.data_ptr<double>() : nullptr, (int)row0, mc,
                partial.data_ptr<double>());
        combine(partial.data_ptr<double>(), (int)row0, mc, gx, s);
    }
}

// Class-1 attributions as float64 [M, FPAD] (columns >= F are zero) from
// the codes of detect_encode and the merged-path table of
// models/mergedpaths.py, all device-resident.
at::Tensor detector_shap(at::Tensor codes, at::Tensor tree_leaf_off,
                         at::Tensor leaf_off, at::Tensor leaf_val,
                         at::Tensor elem_code, at::Tensor elem_z,
                         int64_t n_trees, int64_t F) {
    check_path_table("detector_shap", codes, tree_leaf_off, leaf_off,
                     leaf_val, elem_code, elem_z, n_trees, F);
    const long M = codes.size(0);

    const at::cuda::OptionalCUDAGuard guard(codes.device());
    auto phi = at::empty({M, FPAD}, codes.options().dtype(at::kDouble));
    if (M == 0) return phi;
    shap_row_chunks<false>(
        codes, tree_leaf_off, leaf_off, leaf_val, elem_code, elem_z, n_trees,
        F, [&](const double* partial, int row0, int mc, int gx,
               hipStream_t s) {
            detector_shap_combine_kernel<<<dim3(gx, FPAD), EXPLAIN_BLK, 0,
                                           s>>>(
                partial, row0, mc, (int)n_trees, phi.data_ptr<double>());
        });
    return phi;
}

// Class-1 interaction values as float64 [M, FPAD, FPAD] (rows and columns
// >= F are zero) from the inputs of detector_shap and its output phi.
at::Tensor detector_shap_interactions(
    at::Tensor codes, at::Tensor tree_leaf_off, at::Tensor leaf_off,
    at::Tensor leaf_val, at::Tensor elem_code, at::Tensor elem_z,
    at::Tensor phi, int64_t n_trees, int64_t F) {
    check_path_table("detector_shap_interactions", codes, tree_leaf_off,
                     leaf_off, leaf_val, elem_code, elem_z, n_trees, F);
    const long M = codes.size(0);
    TORCH_CHECK(phi.is_cuda() && phi.device() == codes.device() &&
                phi.dtype() == at::kDouble && phi.dim() == 2 &&
                phi.size(0) == M && phi.size(1) == FPAD &&
                phi.is_contiguous(),
                "detector_shap_interactions: phi is detector_shap's "
                "float64 [M, 16] on the device of codes");

    const at::cuda::OptionalCUDAGuard guard(codes.device());
    auto out = at::zeros({M, FPAD, FPAD}, codes.options().dtype(at::kDouble));
    if (M == 0) return out;
    shap_row_chunks<true>(
        codes, tree_leaf_off, leaf_off, leaf_val, elem_code, elem_z, n_trees,
        F, [&](const double* partial, int row0, int mc, int gx,
               hipStream_t s) {
            detector_interact_combine_kernel<<<dim3(gx, (int)F), EXPLAIN_BLK,
                                               0, s>>>(
                partial, phi.data_ptr<double>(), row0, mc, (int)n_trees,
                out.data_ptr<double>());
        });
    return out;
}

// ---------------------------------------------------------------------------
// grouped leave-one-project-out evaluation (holdout.hip)
// ---------------------------------------------------------------------------
// seg_off arrives CPU-resident (int32 [G + 1]): the block table is built
// from its values, and nothing on the device indexes with an unchecked
// offset.  Returns the int4 (group, first row, end row, 0) table for
// `rows` rows per block on `dev`; groups without rows get no block.  With
// det (int [G], checked by the caller) w holds the group's detector, and
// with det_as_group x holds it as well, for the kernels that index their
// parameters with x.
static at::Tensor holdout_block_table(const at::Tensor& seg_off, long M,
                                      int rows, c10::Device dev,
                                      const char* op,
                                      const int* det = nullptr,
                                      bool det_as_group = false) {
    TORCH_CHECK(!seg_off.is_cuda() && seg_off.dtype() == at::kInt &&
                seg_off.dim() == 1 && seg_off.is_contiguous() &&
                seg_off.numel() >= 2, op, ": seg_off must be CPU int32 [G+1]");
    TORCH_CHECK(M < (1L << 31));
    const int G = (int)seg_off.numel() - 1;
    const int* so = seg_off.data_ptr<int>();
    TORCH_CHECK(so[0] == 0 && so[G] == M, op,
                ": seg_off must run from 0 to the row count");
    std::vector<int> tab;
    for (int g = 0; g < G; ++g) {
        TORCH_CHECK(so[g + 1] >= so[g], op, ": seg_off steps back at group ",
                    g);
        for (int r = so[g]; r < so[g + 1]; r += rows) {
            tab.push_back(det_as_group ? det[g] : g);
            tab.push_back(r);
            tab.push_back(so[g + 1]);
            tab.push_back(det ? det[g] : 0);
        }
    }
    auto t = at::empty({(long)tab.size() / 4, 4}, at::kInt);
    std::copy(tab.begin(), tab.end(), t.data_ptr<int>());
    return t.to(dev);
}

static void launch_holdout_encode(const at::Tensor& X, const at::Tensor& tab,
                                  const DeviceParams& p, bool has_pca,
                                  int64_t F, at::Tensor& codes,
                                  hipStream_t s) {
    holdout_encode_kernel<<<(int)tab.size(0), DETECT_BLK, 0, s>>>(
        X.data_ptr<double>(), (const int4*)tab.data_ptr<int>(),
        p.mean.data_ptr<double>(), p.scale.data_ptr<double>(),
        p.pca_mean.data_ptr<double>(), p.W.data_ptr<double>(),
        has_pca ? 1 : 0, p.cuts_ptr(), p.cut_off.data_ptr<int>(),
        p.cut_base.data_ptr<int>(), (int)F, codes.data_ptr<uint8_t>());
}

static void launch_holdout_proba(const at::Tensor& codes,
                                 const at::Tensor& tab,
                                 const at::Tensor& tree_off,
                                 const at::Tensor& nodes_packed,
                                 int64_t n_trees, at::Tensor& acc,
                                 hipStream_t s) {
    holdout_proba_kernel<<<(int)tab.size(0), DETECT_BLK, 0, s>>>(
        codes.data_ptr<uint8_t>(), (const int4*)tab.data_ptr<int>(),
        tree_off.data_ptr<long>(), (const int2*)nodes_packed.data_ptr<int>(),
        (int)n_trees, n_tree_blocks(n_trees),
        (double2*)acc.data_ptr<double>());
}

// The unmodified rows of permuted_counts and partial_dependence, once per
// call: (codes uint8 [M, 16], acc fp64 [M, 2]).  tab_enc and tab_acc are
// block tables of DETECT_BLK and HOLDOUT_PROBA_ROWS rows whose x names the
// block's detector.
static std::pair<at::Tensor, at::Tensor> encode_and_sum(
    const at::Tensor& X, const at::Tensor& tab_enc, const at::Tensor& tab_acc,
    const DeviceParams& p, bool has_pca, int64_t F,
    const at::Tensor& tree_off, const at::Tensor& nodes_packed,
    int64_t n_trees, hipStream_t s) {
    auto codes = at::empty({X.size(0), FPAD}, X.options().dtype(at::kByte));
    auto acc = at::empty({X.size(0), 2}, X.options());
    launch_holdout_encode(X, tab_enc, p, has_pca, F, codes, s);
    launch_holdout_proba(codes, tab_acc, tree_off, nodes_packed, n_trees, acc,
                         s);
    return {codes, acc};
}

// detect_encode per group: rows seg_off[g]:seg_off[g+1] are encoded with
// row g of mean / scale / pca_mean / W and with group g's cuts.  cut_off
// row g holds group-local offsets (a detector's own cut_off); the groups'
// cuts lie back to back in `cuts`.
at::Tensor holdout_encode(at::Tensor X, at::Tensor seg_off, at::Tensor mean,
                          at::Tensor scale, at::Tensor pca_mean,
                          at::Tensor W, bool has_pca, at::Tensor cuts,
                          at::Tensor cut_off, int64_t F) {
    const char* op = "holdout_encode";
    check_raw_rows(X, F, op);
    const long M = X.size(0);
    auto dev = X.device();
    auto tab = holdout_block_table(seg_off, M, DETECT_BLK, dev, op);
    const long G = seg_off.numel() - 1;
    auto cut_base = grouped_params_check(mean, scale, pca_mean, W, cuts,
                                         cut_off, G, op);

    const at::cuda::OptionalCUDAGuard guard(dev);
    auto codes = at::empty({M, FPAD}, X.options().dtype(at::kByte));
    if (M == 0) return codes;
    auto p = upload_params(mean, scale, pca_mean, W, cuts, cut_off, cut_base,
                           dev);
    launch_holdout_encode(X, tab, p, has_pca, F, codes, current_stream());
    return codes;
}

// forest_proba per group over one concatenated packed forest: group g
// owns trees g * n_trees .. (g + 1) * n_trees - 1, node ids are global.
at::Tensor holdout_proba(at::Tensor codes, at::Tensor seg_off,
                         at::Tensor tree_off, at::Tensor nodes_packed,
                         int64_t n_trees) {
    const char* op = "holdout_proba";
    check_codes(codes, op);
    const long M = codes.size(0);
    auto tab = holdout_block_table(seg_off, M, HOLDOUT_PROBA_ROWS,
                                   codes.device(), op);
    const long G = seg_off.numel() - 1;
    check_forest(tree_off, nodes_packed, G, n_trees, MAX_GROUPED_TREES, op);
    const at::cuda::OptionalCUDAGuard guard(codes.device());
    auto acc = at::empty({M, 2}, codes.options().dtype(at::kDouble));
    if (M == 0) return acc;
    launch_holdout_proba(codes, tab, tree_off, nodes_packed, n_trees, acc,
                         current_stream());
    return acc;
}

// (curve int32 [G + 1, K, 3], argmax int32 [G + 1, 3]), columns FP, FN,
// TP, row G pooled.  thresholds arrive CPU-resident and are checked here.
std::vector<at::Tensor> threshold_counts(at::Tensor acc, at::Tensor labels,
                                         at::Tensor seg_off, int64_t n_trees,
                                         at::Tensor thresholds) {
    TORCH_CHECK(acc.is_cuda() && acc.dtype() == at::kDouble &&
                acc.dim() == 2 && acc.size(1) == 2 && acc.is_contiguous());
    const long M = acc.size(0);
    check_labels(labels, M, "threshold_counts");
    TORCH_CHECK(n_trees >= 1 && n_trees < (1L << 31));
    TORCH_CHECK(!thresholds.is_cuda() && thresholds.dtype() == at::kDouble &&
                thresholds.dim() == 1 && thresholds.is_contiguous());
    const long K = thresholds.numel();
    TORCH_CHECK(K >= 1 && K <= HOLDOUT_MAX_K,
                "threshold_counts: between 1 and ", HOLDOUT_MAX_K,
                " thresholds");
    const double* th = thresholds.data_ptr<double>();
    for (long k = 0; k < K; ++k)
        TORCH_CHECK(std::isfinite(th[k]) && (k == 0 || th[k] > th[k - 1]),
                    "threshold_counts: thresholds must be finite and "
                    "strictly ascending");
    auto tab = holdout_block_table(seg_off, M, DETECT_BLK, acc.device(),
                                   "threshold_counts");
    const long G = seg_off.numel() - 1;

    const at::cuda::OptionalCUDAGuard guard(acc.device());
    auto opts = acc.options().dtype(at::kInt);
    // both outputs in one allocation, cleared by one memset
    auto out = at::empty({(G + 1) * (K + 1) * 3}, opts);
    hipStream_t s = current_stream();
    TORCH_CHECK(hipMemsetAsync(out.data_ptr<int>(), 0,
                               out.numel() * sizeof(int), s) == hipSuccess);
    auto curve = out.narrow(0, 0, (G + 1) * K * 3).view({G + 1, K, 3});
    auto argmax = out.narrow(0, (G + 1) * K * 3, (G + 1) * 3)
                      .view({G + 1, 3});
    if (M == 0) return {curve, argmax};
    auto thr_d = thresholds.to(acc.device());
    threshold_counts_kernel<<<(int)tab.size(0), DETECT_BLK, 0, s>>>(
        (const double2*)acc.data_ptr<double>(), labels.data_ptr<uint8_t>(),
        (const int4*)tab.data_ptr<int>(), thr_d.data_ptr<double>(), (int)K,
        (int)n_trees, (int)G, curve.data_ptr<int>(),
        argmax.data_ptr<int>());
    return {curve, argmax};
}

// ---------------------------------------------------------------------------
// permutation importance (importance.hip)
// ---------------------------------------------------------------------------
// (counts int32 [J, R, G + 1, 3], baseline int32 [G + 1, 3]), columns FP,
// FN, TP, row G pooled.  Job (j, r) classifies X with the columns of
// masks[j] taken from row perm[r][i]; group g is served by detector
// det_of_group[g] of the D stacked ones (the layout of holdout_encode and
// holdout_proba, D in place of G).  threshold < 0 selects the argmax rule,
// otherwise a row is predicted flaky iff acc1 / n_trees >= threshold.
//
// seg_off, det_of_group, masks, perm and the parameters arrive
// CPU-resident.  perm is checked HERE, entry by entry, to stay inside the
// row's own group, and uploaded afterwards: the kernel follows it
// unchecked, so there is no device-resident form of the argument.
std::vector<at::Tensor> permuted_counts(
    at::Tensor X, at::Tensor labels, at::Tensor seg_off,
    at::Tensor det_of_group, at::Tensor perm, at::Tensor masks,
    at::Tensor mean, at::Tensor scale, at::Tensor pca_mean, at::Tensor W,
    bool has_pca, at::Tensor cuts, at::Tensor cut_off, int64_t F,
    at::Tensor tree_off, at::Tensor nodes_packed, int64_t n_trees,
    double threshold) {
    const char* op = "permuted_counts";
    check_raw_rows(X, F, op);
    const long M = X.size(0);
    auto dev = X.device();
    check_labels(labels, M, op);
    TORCH_CHECK(std::isfinite(threshold) || threshold < 0.0, op,
                ": threshold must be finite (negative: argmax rule)");
    TORCH_CHECK(!seg_off.is_cuda() && seg_off.dtype() == at::kInt &&
                seg_off.dim() == 1 && seg_off.numel() >= 2, op,
                ": seg_off must be CPU int32 [G+1]");
    const long G = seg_off.numel() - 1;
    TORCH_CHECK(mean.dim() == 2 && mean.size(0) >= 1, op,
                ": parameters must be [D, 16]");
    const long D = mean.size(0);
    auto cut_base = grouped_params_check(mean, scale, pca_mean, W, cuts,
                                         cut_off, D, op);
    TORCH_CHECK(!det_of_group.is_cuda() && det_of_group.dtype() == at::kInt &&
                det_of_group.dim() == 1 && det_of_group.is_contiguous() &&
                det_of_group.numel() == G, op,
                ": det_of_group must be CPU int32 [G]");
    const int* det = det_of_group.data_ptr<int>();
    for (long g = 0; g < G; ++g)
        TORCH_CHECK(det[g] >= 0 && det[g] < D, op, ": group ", g,
                    " names detector ", det[g], " of ", D);
    auto tab = holdout_block_table(seg_off, M, IMPORTANCE_ROWS, dev, op, det);
    auto tab_enc = holdout_block_table(seg_off, M, DETECT_BLK, dev, op, det,
                                       true);
    auto tab_acc = holdout_block_table(seg_off, M, HOLDOUT_PROBA_ROWS, dev,
                                       op, det, true);

    TORCH_CHECK(!masks.is_cuda() && masks.dtype() == at::kInt &&
                masks.dim() == 1 && masks.is_contiguous() &&
                masks.numel() >= 1, op, ": masks must be CPU int32 [J]");
    const long J = masks.numel();
    for (long j = 0; j < J; ++j) {
        const int m = masks.data_ptr<int>()[j];
        TORCH_CHECK(m > 0 && (m >> F) == 0, op, ": mask ", j,
                    " must be non-zero and within the low F bits");
    }
    TORCH_CHECK(!perm.is_cuda() && perm.dtype() == at::kInt &&
                perm.dim() == 2 && perm.is_contiguous() &&
                perm.size(0) >= 1 && perm.size(1) == M, op,
                ": perm must be CPU int32 [R, M]");
    const long R = perm.size(0);
    const int* so = seg_off.data_ptr<int>();
    for (long r = 0; r < R; ++r) {
        const int* pr = perm.data_ptr<int>() + r * M;
        for (long g = 0; g < G; ++g)
            for (int i = so[g]; i < so[g + 1]; ++i)
                TORCH_CHECK(pr[i] >= so[g] && pr[i] < so[g + 1], op,
                            ": perm[", r, "][", i,
                            "] leaves the row's own group");
    }
    TORCH_CHECK(J * R * (G + 1) * 3 < (1L << 31), op, ": too many jobs");

    check_forest(tree_off, nodes_packed, D, n_trees, MAX_GROUPED_TREES, op);

    const at::cuda::OptionalCUDAGuard guard(dev);
    auto opts = X.options().dtype(at::kInt);
    // both outputs in one allocation, cleared by one memset
    const long n_counts = J * R * (G + 1) * 3;
    auto out = at::empty({n_counts + (G + 1) * 3}, opts);
    hipStream_t s = current_stream();
    TORCH_CHECK(hipMemsetAsync(out.data_ptr<int>(), 0,
                               out.numel() * sizeof(int), s) == hipSuccess);
    auto counts = out.narrow(0, 0, n_counts).view({J, R, G + 1, 3});
    auto baseline = out.narrow(0, n_counts, (G + 1) * 3).view({G + 1, 3});
    if (M == 0) return {counts, baseline};

    auto p = upload_params(mean, scale, pca_mean, W, cuts, cut_off, cut_base,
                           dev);
    auto perm_d = perm.to(dev), masks_d = masks.to(dev);
    auto [codes, acc] = encode_and_sum(X, tab_enc, tab_acc, p, has_pca, F,
                                       tree_off, nodes_packed, n_trees, s);

    const long n_jobs = J * R;
    auto launch = has_pca ? permuted_counts_kernel<true>
                          : permuted_counts_kernel<false>;
    launch<<<job_grid(tab.size(0), (n_jobs + IMPORTANCE_WAVES - 1)
                                       / IMPORTANCE_WAVES),
             DETECT_BLK, 0, s>>>(
        X.data_ptr<double>(), labels.data_ptr<uint8_t>(),
        (const int4*)tab.data_ptr<int>(), codes.data_ptr<uint8_t>(),
        (const double2*)acc.data_ptr<double>(), perm_d.data_ptr<int>(),
        masks_d.data_ptr<int>(), p.mean.data_ptr<double>(),
        p.scale.data_ptr<double>(), p.pca_mean.data_ptr<double>(),
        p.W.data_ptr<double>(), p.cuts_ptr(), p.cut_off.data_ptr<int>(),
        p.cut_base.data_ptr<int>(), (int)F, tree_off.data_ptr<long>(),
        (const int2*)nodes_packed.data_ptr<int>(), (int)n_trees,
        n_tree_blocks(n_trees), (int)n_jobs, (int)R, (int)M, (int)G,
        threshold, counts.data_ptr<int>(), baseline.data_ptr<int>());
    return {counts, baseline};
}

// ---------------------------------------------------------------------------
// partial dependence and ICE (dependence.hip)
// ---------------------------------------------------------------------------
// (S fp64 [J + 1, G + 1], flagged int32 [J + 1, G + 1], ice fp64 [J, M] or
// an empty tensor).  Job j classifies X with column job_col[j] of every
// row set to job_val[j]; row J is the unmodified X.  S[j][g] is the sum of
// acc1 over group g in the reduction order pinned in dependence.hip,
// flagged[j][g] the rows predicted flaky, column G pooled; ice[j][i] is
// acc1 of row i under job j.  threshold < 0 selects the argmax rule,
// otherwise a row is predicted flaky iff acc1 / n_trees >= threshold.
//
// One detector serves every group: the parameters are one set in the
// stacked layout of holdout_encode (D = 1).  seg_off, the jobs and the
// parameters arrive CPU-resident and are checked here.
std::vector<at::Tensor> partial_dependence(
    at::Tensor X, at::Tensor seg_off, at::Tensor job_col, at::Tensor job_val,
    at::Tensor mean, at::Tensor scale, at::Tensor pca_mean, at::Tensor W,
    bool has_pca, at::Tensor cuts, at::Tensor cut_off, int64_t F,
    at::Tensor tree_off, at::Tensor nodes_packed, int64_t n_trees,
    double threshold, bool want_ice) {
    const char* op = "partial_dependence";
    check_raw_rows(X, F, op);
    const long M = X.size(0);
    auto dev = X.device();
    TORCH_CHECK(std::isfinite(threshold) || threshold < 0.0, op,
                ": threshold must be finite (negative: argmax rule)");
    TORCH_CHECK(!seg_off.is_cuda() && seg_off.dtype() == at::kInt &&
                seg_off.dim() == 1 && seg_off.numel() >= 2, op,
                ": seg_off must be CPU int32 [G+1]");
    const long G = seg_off.numel() - 1;
    auto cut_base = grouped_params_check(mean, scale, pca_mean, W, cuts,
                                         cut_off, 1, op);

    TORCH_CHECK(!job_col.is_cuda() && job_col.dtype() == at::kInt &&
                job_col.dim() == 1 && job_col.is_contiguous(), op,
                ": job_col must be CPU int32 [J]");
    const long J = job_col.numel();
    TORCH_CHECK(J >= 1 && J <= DEPENDENCE_MAX_JOBS, op, ": between 1 and ",
                DEPENDENCE_MAX_JOBS, " jobs");
    TORCH_CHECK(!job_val.is_cuda() && job_val.dtype() == at::kDouble &&
                job_val.dim() == 1 && job_val.is_contiguous() &&
                job_val.numel() == J, op,
                ": job_val must be CPU float64 [J]");
    for (long j = 0; j < J; ++j) {
        const int c = job_col.data_ptr<int>()[j];
        TORCH_CHECK(c >= 0 && c < F, op, ": job ", j, " names column ", c,
                    " of ", F);
        TORCH_CHECK(std::isfinite(job_val.data_ptr<double>()[j]), op,
                    ": job ", j, " has a non-finite value");
    }
    TORCH_CHECK(!want_ice || M * J < (1L << 31), op,
                ": too many rows x jobs for the ICE output");

    // one detector: every group's blocks read parameter set 0
    const std::vector<int> det((size_t)G, 0);
    auto tab_enc = holdout_block_table(seg_off, M, DETECT_BLK, dev, op,
                                       det.data(), true);
    static_assert(DEPENDENCE_ROWS == HOLDOUT_PROBA_ROWS,
                  "one 64-row table serves both kernels");
    auto tab = holdout_block_table(seg_off, M, DEPENDENCE_ROWS, dev, op,
                                   det.data(), true);
    // first 64-row block of every group, in the table's order
    auto grp_blk = at::empty({G + 1}, at::kInt);
    {
        const int* so = seg_off.data_ptr<int>();
        int* gb = grp_blk.data_ptr<int>();
        gb[0] = 0;
        for (long g = 0; g < G; ++g)
            gb[g + 1] = gb[g] + (so[g + 1] - so[g] + DEPENDENCE_ROWS - 1)
                                    / DEPENDENCE_ROWS;
        TORCH_CHECK(gb[G] == tab.size(0));
    }

    check_forest(tree_off, nodes_packed, 1, n_trees, MAX_GROUPED_TREES, op);
    TORCH_CHECK(tree_off.device() == dev && nodes_packed.device() == dev, op,
                ": X and the forest must share a device");

    const at::cuda::OptionalCUDAGuard guard(dev);
    if (M == 0)
        return {at::zeros({J + 1, G + 1}, X.options()),
                at::zeros({J + 1, G + 1}, X.options().dtype(at::kInt)),
                at::empty({want_ice ? J : 0, 0}, X.options())};
    const long nb = tab.size(0);
    // every cell of the outputs and of the per-block intermediates has
    // exactly one writer: nothing is cleared
    auto S = at::empty({J + 1, G + 1}, X.options());
    auto flagged = at::empty({J + 1, G + 1}, X.options().dtype(at::kInt));
    auto ice = want_ice ? at::empty({J, M}, X.options())
                        : at::empty({0, 0}, X.options());
    auto blk_sum = at::empty({J + 1, nb}, X.options());
    auto blk_cnt = at::empty({J + 1, nb}, X.options().dtype(at::kInt));

    auto p = upload_params(mean, scale, pca_mean, W, cuts, cut_off, cut_base,
                           dev);
    auto col_d = job_col.to(dev), val_d = job_val.to(dev);
    auto grp_d = grp_blk.to(dev);
    hipStream_t s = current_stream();
    auto [codes, acc] = encode_and_sum(X, tab_enc, tab, p, has_pca, F,
                                       tree_off, nodes_packed, n_trees, s);

    auto launch = has_pca ? partial_dependence_kernel<true>
                          : partial_dependence_kernel<false>;
    launch<<<job_grid(nb, (J + DEPENDENCE_WAVES - 1) / DEPENDENCE_WAVES),
             DETECT_BLK, 0, s>>>(
        X.data_ptr<double>(), (const int4*)tab.data_ptr<int>(),
        codes.data_ptr<uint8_t>(), (const double2*)acc.data_ptr<double>(),
        col_d.data_ptr<int>(), val_d.data_ptr<double>(),
        p.mean.data_ptr<double>(), p.scale.data_ptr<double>(),
        p.pca_mean.data_ptr<double>(), p.W.data_ptr<double>(), p.cuts_ptr(),
        p.cut_off.data_ptr<int>(), (int)F, tree_off.data_ptr<long>(),
        (const int2*)nodes_packed.data_ptr<int>(), (int)n_trees,
        n_tree_blocks(n_trees), (int)J, (int)M, threshold,
        blk_sum.data_ptr<double>(), blk_cnt.data_ptr<int>(),
        want_ice ? ice.data_ptr<double>() : nullptr);
    dependence_reduce_kernel<<<(int)(J + 1), DEPENDENCE_REDUCE_BLK, 0, s>>>(
        blk_sum.data_ptr<double>(), blk_cnt.data_ptr<int>(),
        grp_d.data_ptr<int>(), (int)nb, (int)G, S.data_ptr<double>(),
        flagged.data_ptr<int>());
    return {S, flagged, ice};
}

// ---------------------------------------------------------------------------
// forest proximity (similar.hip)
// ---------------------------------------------------------------------------
// Tree-local canonical leaf ids as int32 [M, T].  The caller guarantees a
// well-formed packed forest, as for forest_proba.
at::Tensor forest_leaves(at::Tensor codes, at::Tensor tree_off,
                         at::Tensor nodes_packed, int64_t n_trees) {
    const char* op = "forest_leaves";
    check_codes(codes, op);
    check_forest(tree_off, nodes_packed, 1, n_trees, PROX_MAX_T, op);
    TORCH_CHECK(codes.device() == tree_off.device() &&
                codes.device() == nodes_packed.device(), op,
                ": tensors on different devices");
    const at::cuda::OptionalCUDAGuard guard(codes.device());
    const long M = codes.size(0);
    auto leaf = at::empty({M, n_trees}, codes.options().dtype(at::kInt));
    if (M == 0) return leaf;
    const long total = M * n_trees;
    const long blocks = (total + DETECT_BLK - 1) / DETECT_BLK;
    TORCH_CHECK(blocks < (1L << 31), op, ": too many (row, tree) pairs");
    forest_leaves_kernel<<<(unsigned)blocks, DETECT_BLK, 0,
                           current_stream()>>>(
        codes.data_ptr<uint8_t>(), tree_off.data_ptr<long>(),
        (const int2*)nodes_packed.data_ptr<int>(), (int)M, (int)n_trees,
        leaf.data_ptr<int>());
    return leaf;
}

template <int K, bool PACKED>
static void launch_proximity(dim3 grid, hipStream_t s, const uint32_t* qT,
                             const uint32_t* cP, const int* self, int M,
                             int N, int T, int W, int chunk_rows, int k,
                             int* o_idx, int* o_sh) {
    proximity_topk_kernel<K, PACKED><<<grid, PROX_BLK, 0, s>>>(
        qT, cP, self, M, N, T, W, chunk_rows, k, o_idx, o_sh);
}

// For every row of leaf_q the first k rows of leaf_c in the order (more
// equal ids, then lower row), leaving out row self_idx[q] (-1: none):
// (idx, shared), both int32 [M, k], short lists padded with (-1, 0).
// self_idx may live on either side; it is range-checked on the host.
std::vector<at::Tensor> proximity_topk(at::Tensor leaf_q, at::Tensor leaf_c,
                                       at::Tensor self_idx, int64_t k) {
    const char* op = "proximity_topk";
    for (const at::Tensor* p : {&leaf_q, &leaf_c})
        TORCH_CHECK(p->is_cuda() && p->dtype() == at::kInt &&
                    p->dim() == 2 && p->is_contiguous(), op,
                    ": leaf ids must be contiguous device int32 [rows, T]");
    TORCH_CHECK(leaf_q.device() == leaf_c.device(), op,
                ": leaf matrices on different devices");
    const long M = leaf_q.size(0), N = leaf_c.size(0), T = leaf_q.size(1);
    TORCH_CHECK(leaf_c.size(1) == T, op, ": query rows hold ", T,
                " trees, corpus rows ", leaf_c.size(1));
    TORCH_CHECK(T >= 1 && T <= PROX_MAX_T, op, ": T must be in 1..",
                PROX_MAX_T);
    TORCH_CHECK(k >= 1 && k <= PROX_MAX_K, op, ": k must be in 1..",
                PROX_MAX_K);
    TORCH_CHECK(M < (1L << 31) && N < (1L << 31) - PROX_CHUNK, op,
                ": too many rows");
    TORCH_CHECK(self_idx.dtype() == at::kInt && self_idx.dim() == 1 &&
                self_idx.size(0) == M, op, ": self_idx must be int32 [M]");
    auto self_host = self_idx.cpu().contiguous();
    for (long q = 0; q < M; ++q) {
        const int v = self_host.data_ptr<int>()[q];
        TORCH_CHECK(v >= -1 && v < N, op, ": self_idx[", q, "] = ", v,
                    " is outside [-1, ", N, ")");
    }

    const at::cuda::OptionalCUDAGuard guard(leaf_q.device());
    auto opts = leaf_q.options();
    auto idx = at::empty({M, k}, opts), shared = at::empty({M, k}, opts);
    if (M == 0) return {idx, shared};
    if (N == 0) {
        idx.fill_(-1);
        shared.zero_();
        return {idx, shared};
    }
    hipStream_t s = current_stream();
    auto self_d = self_host.to(leaf_q.device());

    // do all ids fit 16 bits?  one pass and one 4-byte readback
    auto flag = at::zeros({1}, opts);
    for (const at::Tensor* p : {&leaf_q, &leaf_c}) {
        const long n = p->numel();
        const long blocks =
            std::min(2048L, (n + PROX_BLK - 1) / PROX_BLK);
        prox_wide_kernel<<<(unsigned)blocks, PROX_BLK, 0, s>>>(
            p->data_ptr<int>(), n, flag.data_ptr<int>());
    }
    const bool packed = flag.cpu().data_ptr<int>()[0] == 0;

    const long per = packed ? 2 : 1;
    const long W = ((T + per - 1) / per + PROX_D - 1) / PROX_D * PROX_D;
    auto qT = at::empty({W, M}, opts), cP = at::empty({N, W}, opts);
    auto pack = packed ? prox_pack_kernel<true> : prox_pack_kernel<false>;
    TORCH_CHECK((M * W + PROX_BLK - 1) / PROX_BLK < (1L << 31) &&
                (N * W + PROX_BLK - 1) / PROX_BLK < (1L << 31), op,
                ": too many ids");
    pack<<<(unsigned)((M * W + PROX_BLK - 1) / PROX_BLK), PROX_BLK, 0, s>>>(
        leaf_q.data_ptr<int>(), M, (int)T, (int)W, 1L, M,
        (uint32_t*)qT.data_ptr<int>());
    pack<<<(unsigned)((N * W + PROX_BLK - 1) / PROX_BLK), PROX_BLK, 0, s>>>(
        leaf_c.data_ptr<int>(), N, (int)T, (int)W, W, 1L,
        (uint32_t*)cP.data_ptr<int>());

    // Chunks of PROX_CHUNK corpus rows; of a whole multiple of that once
    // the grid would pass 2048 workgroups (8 per CU), so the partial
    // lists stay a small multiple of the output.
    const long q_blocks = (M + PROX_BLK - 1) / PROX_BLK;
    const long most = std::min(65535L, std::max(1L, 2048 / q_blocks));
    const long n_least = (N + PROX_CHUNK - 1) / PROX_CHUNK;
    const long chunk_rows = PROX_CHUNK * ((n_least + most - 1) / most);
    const long n_chunks = (N + chunk_rows - 1) / chunk_rows;

    at::Tensor p_idx = idx, p_sh = shared;
    if (n_chunks > 1) {
        p_idx = at::empty({n_chunks, k, M}, opts);
        p_sh = at::empty({n_chunks, k, M}, opts);
    }
    const int kmax = k == 1 ? 1 : (k <= 8 ? 8 : 16);
    auto launch =
        kmax == 1 ? (packed ? launch_proximity<1, true>
                            : launch_proximity<1, false>)
        : kmax == 8 ? (packed ? launch_proximity<8, true>
                              : launch_proximity<8, false>)
                    : (packed ? launch_proximity<16, true>
                              : launch_proximity<16, false>);
    launch(dim3((unsigned)q_blocks, (unsigned)n_chunks), s,
           (const uint32_t*)qT.data_ptr<int>(),
           (const uint32_t*)cP.data_ptr<int>(), self_d.data_ptr<int>(),
           (int)M, (int)N, (int)T, (int)W, (int)chunk_rows, (int)k,
           p_idx.data_ptr<int>(), p_sh.data_ptr<int>());
    if (n_chunks > 1) {
        auto merge = kmax == 1 ? proximity_merge_kernel<1>
                     : kmax == 8 ? proximity_merge_kernel<8>
                                 : proximity_merge_kernel<16>;
        merge<<<(unsigned)q_blocks, PROX_BLK, 0, s>>>(
            p_idx.data_ptr<int>(), p_sh.data_ptr<int>(), (int)M,
            (int)n_chunks, (int)k, idx.data_ptr<int>(),
            shared.data_ptr<int>());
    }
    return {idx, shared};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("treeshap", &treeshap, py::call_guard<py::gil_scoped_release>(),
          "Path-dependent TreeSHAP (class-0), summed over trees");
    m.def("treeshap_paths", &treeshap_paths,
          py::call_guard<py::gil_scoped_release>(),
          "Leaf-path TreeSHAP (class-0), summed over trees");
    // gil_scoped_release: the forest_fit level loop blocks on stream syncs;
    // releasing the GIL lets other Python threads drive their own streams.
    m.def("forest_fit", &forest_fit,
          py::call_guard<py::gil_scoped_release>(),
          "Batched histogram-forest fit (gfx950)");
    m.def("forest_fit_multi", &forest_fit_multi,
          py::call_guard<py::gil_scoped_release>(),
          "Mixed-model batched forest fit (per-job spec)");
    m.def("forest_predict_confusion", &forest_predict_confusion,
          py::call_guard<py::gil_scoped_release>(),
          "Ensemble predict + confusion accumulation");
    m.def("knn", &knn, py::call_guard<py::gil_scoped_release>(),
          "Brute-force k-NN (fp64 distances)");
    m.def("knn_segmented", &knn_segmented,
          py::call_guard<py::gil_scoped_release>(),
          "Fold-batched segmented k-NN (segment-local indices)");
    m.def("smote_interpolate", &smote_interpolate,
          py::call_guard<py::gil_scoped_release>(), "SMOTE synthesis");
    m.def("enn_keep", &enn_keep, py::call_guard<py::gil_scoped_release>(),
          "ENN keep-mask");
    m.def("tomek_keep", &tomek_keep,
          py::call_guard<py::gil_scoped_release>(), "Tomek-link keep-mask");
    m.def("bin_codes", &bin_codes_dev,
          py::call_guard<py::gil_scoped_release>(), "Quantile-bin codes");
    m.def("scaler_fit_transform", &scaler_fit_transform_dev,
          py::call_guard<py::gil_scoped_release>(),
          "StandardScaler fit_transform");
    m.def("pca_fit_transform", &pca_fit_transform_dev,
          py::call_guard<py::gil_scoped_release>(),
          "Full PCA fit_transform");
    m.def("detect_encode", &detect_encode,
          py::call_guard<py::gil_scoped_release>(),
          "Saved-detector scale/PCA/bin in one pass");
    m.def("forest_proba", &forest_proba,
          py::call_guard<py::gil_scoped_release>(),
          "Per-row class-probability sums over a packed forest");
    m.def("detector_shap", &detector_shap,
          py::call_guard<py::gil_scoped_release>(),
          "Per-row class-1 TreeSHAP over a detector's merged leaf paths");
    m.def("detector_shap_interactions", &detector_shap_interactions,
          py::call_guard<py::gil_scoped_release>(),
          "Per-row class-1 SHAP interaction values over merged leaf paths");
    m.def("holdout_encode", &holdout_encode,
          py::call_guard<py::gil_scoped_release>(),
          "detect_encode with per-group parameters and cuts");
    m.def("holdout_proba", &holdout_proba,
          py::call_guard<py::gil_scoped_release>(),
          "forest_proba with one forest per group, one launch");
    m.def("threshold_counts", &threshold_counts,
          py::call_guard<py::gil_scoped_release>(),
          "Per-group [FP, FN, TP] under argmax and K probability thresholds");
    m.def("permuted_counts", &permuted_counts,
          py::call_guard<py::gil_scoped_release>(),
          "Per-group [FP, FN, TP] of J column masks x R row permutations");
    m.def("partial_dependence", &partial_dependence,
          py::call_guard<py::gil_scoped_release>(),
          "fused partial-dependence / ICE jobs -> (S [J+1, G+1], flagged "
          "[J+1, G+1], ice [J, M] or empty)");
    m.def("forest_leaves", &forest_leaves,
          py::call_guard<py::gil_scoped_release>(),
          "Per-row, per-tree canonical leaf ids over a packed forest");
    m.def("proximity_topk", &proximity_topk,
          py::call_guard<py::gil_scoped_release>(),
          "First k corpus rows by shared leaves, ties to the lower row");
}
