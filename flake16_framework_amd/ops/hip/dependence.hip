// Partial-dependence / ICE kernels (engine/dependence.py), gfx950.
//
// Job j sets raw column job_col[j] of EVERY row to job_val[j], classifies
// the rows again and reports, per project and pooled, how many rows are
// predicted flaky and the fp64 sum of acc1; optionally acc1 of every
// (job, row), the ICE curves.  One launch serves all J jobs.
//
//   partial_dependence_kernel  block = 64 rows of one project (the int4
//                              block table of holdout.hip), lane = row,
//                              wave = job, striding over the jobs of the
//                              block's blockIdx.y share.  Per (row, job):
//                              encode with the replaced value, walk the
//                              forest, apply the rule; per (block, job) one
//                              count and one block sum leave with plain
//                              stores.
//   dependence_reduce_kernel   one thread per (job, project): the
//                              project's block sums and counts added
//                              sequentially in ascending block order, then
//                              the pooled value from the project values.
//
// The unmodified rows are encoded and summed once per call by
// holdout_encode_kernel and holdout_proba_kernel; the first kernel reads
// their codes and (acc0, acc1) per row, keeps them in registers across its
// jobs and reports the baseline from them as row J (blockIdx.y == 0,
// wave 0).  Parameters and cuts are staged into LDS once per block.
//
// The replaced value is wave-uniform.  Without a projection its z and its
// code are wave-uniform too, only one code byte changes, and a row whose
// baseline byte already equals the new code takes its baseline sums
// without walking the forest (exact: equal codes give equal walks).  With
// a projection every component depends on the column: the rows' own
// centred values are kept in LDS and the uniform term takes column f's
// place in the sum.
//
// Bit-parity contract: that of detector_steps.h for (acc0, acc1) and the
// rule, and for the sums the reduction tree pinned in engine/dependence.py:
//   - a block is 64 consecutive rows of a project from its first row; its
//     sum B is the pairwise tree v = v[0::2] + v[1::2] six times over the
//     rows' acc1, 0.0 past the last row: wave_sum_f64 (wave_ops.h) is that
//     tree, and a wave holds all 64 rows of its block for a job
//   - S[g] = 0.0 + B_first + B_next + ... over the project's blocks in
//     ascending order, S[G] = 0.0 + S[0] + S[1] + ... over the projects
//   - counts are popcounts of ballots, added as integers
// Every cell of the [J + 1, n_blocks64] intermediates has exactly one
// writer: no atomics of either kind, and nothing to clear.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detector_steps.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

#define DEPENDENCE_ROWS 64        // rows per block: one per lane
#define DEPENDENCE_WAVES (DETECT_BLK / DEPENDENCE_ROWS)
#define DEPENDENCE_MAX_JOBS 1024
#define DEPENDENCE_REDUCE_BLK 64

template <bool HAS_PCA>
__global__ __launch_bounds__(DETECT_BLK) void partial_dependence_kernel(
    const double* __restrict__ X,          // [M, FPAD] raw, zero-padded
    const int4* __restrict__ blk_tab,      // [gridDim.x] y, z = row range
    const uint8_t* __restrict__ base_codes,    // [M, FPAD]
    const double2* __restrict__ base_acc,  // [M]
    const int* __restrict__ job_col,       // [J] positions in [0, F)
    const double* __restrict__ job_val,    // [J] finite raw values
    const double* __restrict__ mean,       // [FPAD]
    const double* __restrict__ scale,      // [FPAD]
    const double* __restrict__ pca_mean,   // [FPAD]
    const double* __restrict__ W,          // [FPAD, FPAD], W[f][k]
    const float* __restrict__ cuts,        // flat, n_cuts entries
    const int* __restrict__ cut_off,       // [FPAD + 1]
    int F,
    const long* __restrict__ tree_off,     // [n_trees + 1] root ids
    const int2* __restrict__ nodes,        // packed records
    int n_trees, int n_blocks, int n_jobs, int M,
    double threshold,                      // < 0: argmax rule
    double* __restrict__ blk_sum,          // [J + 1, gridDim.x]
    int* __restrict__ blk_cnt,             // [J + 1, gridDim.x]
    double* __restrict__ ice /* [J, M] acc1, or null */) {
    // s_own is placed on a 16-byte boundary: 8 B of padding follow the
    // 18,824 B of s
    __shared__ DetectorLds s;
    __shared__ double s_own[HAS_PCA ? FPAD * DEPENDENCE_ROWS : 1];

    const int tid = threadIdx.x;
    const int lane = tid % DEPENDENCE_ROWS;
    const int wave = __builtin_amdgcn_readfirstlane(tid / DEPENDENCE_ROWS);
    const int4 blk = blk_tab[blockIdx.x];
    stage_detector(s, mean, scale, pca_mean, W, cuts, cut_off);

    // lanes past the block's last row repeat it and are masked out of
    // every result, so every lane reads valid rows and the wave is fully
    // active where it reduces
    const bool live = blk.y + lane < blk.z;
    const int row = live ? blk.y + lane : blk.z - 1;
    const RowCodes b_codes = load_codes(base_codes, row);
    const double2 b_acc = base_acc[row];

    // the rows' own centred values z[f] - pca_mean[f], column-major (the
    // block's waves share their rows; wave w fills columns 4w..4w+3)
    if (HAS_PCA) {
        for (int f = wave * (FPAD / DEPENDENCE_WAVES);
             f < (wave + 1) * (FPAD / DEPENDENCE_WAVES); ++f)
            s_own[f * DEPENDENCE_ROWS + lane] =
                scaled(s, f, X[(size_t)row * FPAD + f]) - s.pmean[f];
        __syncthreads();
    }

    const size_t nb = gridDim.x;
    if (blockIdx.y == 0 && wave == 0) {
        const bool pred = predicted(b_acc, n_trees, threshold);
        const int cnt = __popcll(__ballot(live && pred));
        const double B = wave_sum_f64(live ? b_acc.y : 0.0);
        if (lane == 0) {
            blk_sum[(size_t)n_jobs * nb + blockIdx.x] = B;
            blk_cnt[(size_t)n_jobs * nb + blockIdx.x] = cnt;
        }
    }

    for (int job = blockIdx.y * DEPENDENCE_WAVES + wave; job < n_jobs;
         job += gridDim.y * DEPENDENCE_WAVES) {
        // wave-uniform: the job's column and its scaled value
        const int jf = job_col[job];
        const double jz = scaled(s, jf, job_val[job]);

        RowCodes c;
        if (HAS_PCA) {
            const double jd = jz - s.pmean[jf];
            double t[FPAD];
#pragma unroll
            for (int k = 0; k < FPAD; ++k) t[k] = 0.0;
            // rolled, as in permuted_counts_kernel: one column live at a
            // time
#pragma unroll 1
            for (int f = 0; f < F; ++f) {
                const double dv =
                    f == jf ? jd : s_own[f * DEPENDENCE_ROWS + lane];
#pragma unroll
                for (int k = 0; k < FPAD; ++k)
                    t[k] = t[k] + dv * s.W[f * FPAD + k];
            }
            c = search_codes(s, t, F);
        } else {
            c = with_code(b_codes, jf, __builtin_amdgcn_readfirstlane(
                                           cut_code(s, jf, jz)));
        }

        // the walk diverges per lane; the wave is whole again after it
        const double2 acc = same_codes(c, b_codes)
            ? b_acc : forest_sums(nodes, tree_off, n_trees, n_blocks, c);
        const bool pred = predicted(acc, n_trees, threshold);
        const int cnt = __popcll(__ballot(live && pred));
        const double B = wave_sum_f64(live ? acc.y : 0.0);
        if (lane == 0) {
            blk_sum[(size_t)job * nb + blockIdx.x] = B;
            blk_cnt[(size_t)job * nb + blockIdx.x] = cnt;
        }
        if (ice != nullptr && live) ice[(size_t)job * M + row] = acc.y;
    }
}

// Definition steps 3 and 4 and the integer sums.  Block j serves job j
// (row J: the baseline); thread g adds the block values of project g,
// blocks grp_blk[g] .. grp_blk[g + 1] - 1, sequentially from 0.0; after
// the barrier thread 0 adds the project values in ascending order.  S and
// flagged carry no __restrict__: thread 0 reads what the block's other
// threads stored.
__global__ __launch_bounds__(DEPENDENCE_REDUCE_BLK)
void dependence_reduce_kernel(
    const double* __restrict__ blk_sum,    // [J + 1, nb]
    const int* __restrict__ blk_cnt,       // [J + 1, nb]
    const int* __restrict__ grp_blk,       // [G + 1] first block of project
    int nb, int G,
    double* S,                             // [J + 1, G + 1]
    int* flagged /* [J + 1, G + 1] */) {
    const size_t j = blockIdx.x;
    const double* bs = blk_sum + j * (size_t)nb;
    const int* bc = blk_cnt + j * (size_t)nb;
    double* Sj = S + j * (size_t)(G + 1);
    int* Fj = flagged + j * (size_t)(G + 1);
    for (int g = threadIdx.x; g < G; g += DEPENDENCE_REDUCE_BLK) {
        double s = 0.0;
        int c = 0;
        for (int b = grp_blk[g]; b < grp_blk[g + 1]; ++b) {
            s += bs[b];
            c += bc[b];
        }
        Sj[g] = s;
        Fj[g] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        int c = 0;
        for (int g = 0; g < G; ++g) {
            s += Sj[g];
            c += Fj[g];
        }
        Sj[G] = s;
        Fj[G] = c;
    }
}

// Both forms are instantiated here, so that compiling this file alone with
// -Rpass-analysis=kernel-resource-usage reports them
// (profiles/dependence.md).
#define PARTIAL_DEPENDENCE_INSTANCE(HAS_PCA)                                \
    template __global__ void partial_dependence_kernel<HAS_PCA>(            \
        const double*, const int4*, const uint8_t*, const double2*,         \
        const int*, const double*, const double*, const double*,            \
        const double*, const double*, const float*, const int*, int,        \
        const long*, const int2*, int, int, int, int, double, double*,      \
        int*, double*)
PARTIAL_DEPENDENCE_INSTANCE(false);
PARTIAL_DEPENDENCE_INSTANCE(true);
#undef PARTIAL_DEPENDENCE_INSTANCE
