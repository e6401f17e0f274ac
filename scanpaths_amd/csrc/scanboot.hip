// Cluster bootstrap of ratio-of-sums statistics: intervals and paired comparisons for every keyed score table.
// float64, every operation rounded on its own (the arithmetic rule of scan_common.h: contraction OFF, plain operators); every sum has
// a fixed, stated order and there are no floating-point atomics, so tests/bootstrap_ref.py reproduces every output bit for bit.
//
//   boot_cluster_sums_kernel: ONE THREAD PER (cluster, column).  The host hands the keys over sorted by cluster (stable, so ascending
//     key index inside a cluster) as start / count runs; N[c][m] = sum of num[start[c] + k][m], k = 0 .. count[c] - 1 in that order from
//     0.0, D[c][m] likewise from den.  A run that does not lie inside [0, G) reads nothing and gives NaN.
//
//   boot_resample_kernel: ONE WAVEFRONT PER REPLICATE, four per block (scan_wave_item); item b < B is replicate b, item B is the POINT
//     ESTIMATE.  THE DRAW: draw j of replicate b is word (j & 3) of the Philox4x32-10 block with key (seed lo, seed hi) and counter
//     (b, j >> 2, 0, 1); the drawn cluster is (uint64(word) * C) >> 32.  The point estimate "draws" cluster j at position j: every
//     cluster once.  THE ORDER OF THE SUMS: lane l adds the rows N[i(b, j)][.] and D[i(b, j)][.] of its draws j = l, l + 64, l + 128, ..
//     in that order from 0.0; the 64 partial sums of every column combine by the xor butterfly 32, 16, 8, 4, 2, 1 (wave_sum_d), after
//     which every lane holds the same totals.  R[m] = (sum N) / (sum D), IEEE (0 / 0 = NaN).  stat[s] = (R[i] - R[j]) / (R[k] - R[l]) for
//     contrast s = (i, j, k, l): j = -1 subtracts nothing, k = -1 divides by nothing, l = -1 subtracts nothing below.  An index outside
//     the launch's columns gives NaN (no memory is read through a contrast index: the column is chosen by a chain of selects over the
//     registers).  Lane s % 64 writes stat[s][b] (the point estimate: estimate[s]).
//     THE TABLE IS READ STRAIGHT FROM L2, NOT THROUGH LDS: at the package's scale (1000 clusters x 32 columns x 2 tables of doubles =
//     512 KB) it does not fit the 160 KB of LDS but sits in every XCD's 4 MB L2, each lane reads whole rows (Mc consecutive doubles),
//     and the sums of a lane live in registers: 2 * MAXCOL doubles = 128 of the kernel's 155 VGPRs at MAXCOL = 32, 3 waves per SIMD.
//     MAXCOL = sp_boot_max_columns() columns per launch; the host chunks wider tables (same seed, hence identical draws).
//
//   boot_moments_kernel: ONE BLOCK PER STATISTIC over its B replicates v.  A replicate is valid iff it is not NaN.  n_valid, n_le0
//     (v <= 0), n_ge0 (v >= 0) are integer counts.  THE ORDER OF THE TWO PASSES: thread t adds the valid v[t], v[t + 256], .. in that
//     order from 0.0 (an invalid one adds 0.0); the 64 partial sums of a wave combine by the xor butterfly, the four wave totals as
//     ((w0 + w1) + w2) + w3; mean = that / n_valid.  The second pass sums (v - mean) * (v - mean) of the valid replicates the same way;
//     sd = sqrt(that / (n_valid - 1)), NaN for n_valid < 2; mean NaN for n_valid = 0.  It also sets the statistic's Q quantiles to NaN.
//   boot_rank_kernel: ONE THREAD PER (statistic, replicate).  rank(i) = #{j : v[j] < v[i] or (v[j] == v[i] and j < i)} over the valid
//     replicates -- exact, tie-safe, +-inf like any other value, NaN never counted and never ranked.  The ranks of the valid replicates
//     are a permutation of 0 .. n_valid - 1, so for every quantile q exactly one thread finds its rank equal to
//     min(max(ceil(q * n_valid) - 1, 0), n_valid - 1) (q * n_valid in float64 as written) and stores its value: an order statistic, no
//     arithmetic on the values.  The v[j] pass through LDS in tiles of 256.
// Every element of every output is written; all stores are plain vector stores.
#include "common.h"
#include "scan_common.h"
#include "philox.h"

namespace {

constexpr int MAXCOL = 32;        // = sp_boot_max_columns()
constexpr int MAXCLUSTERS = 1 << 24;

struct SumArgs {
    const double *num, *den;
    const int64_t* start;
    const int* count;
    int G, C, M;
    double *N, *D;
};

__global__ __launch_bounds__(256) void boot_cluster_sums_kernel(const SumArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.C * a.M) return;
    const int c = (int)(i / a.M), m = (int)(i % a.M);
    const int64_t s = a.start[c];
    const int n = a.count[c];
    double sn = 0.0, sd = 0.0;
    if (s < 0 || n < 0 || s + n > (int64_t)a.G) {
        sn = sd = __builtin_nan("");
    } else {
        for (int k = 0; k < n; ++k) {
            sn = sn + a.num[(s + k) * a.M + m];
            sd = sd + a.den[(s + k) * a.M + m];
        }
    }
    a.N[i] = sn;
    a.D[i] = sd;
}

struct ResampleArgs {
    const double *N, *D;
    int C, M, ld;
    const int* contrast;
    int S, B;
    uint32_t k0, k1;
    double *stat, *estimate;
};

// column idx of R, NaN for an index that is not a column of this launch
__device__ __forceinline__ double boot_pick(const double (&R)[MAXCOL], int idx) {
    double r = __builtin_nan("");
#pragma unroll
    for (int m = 0; m < MAXCOL; ++m) r = (m == idx) ? R[m] : r;
    return r;
}

__global__ __launch_bounds__(256) void boot_resample_kernel(const ResampleArgs a) {
    int lane;
    int64_t b;
    if (!scan_wave_item((int64_t)a.B + 1, lane, b)) return;
    const bool point = b == a.B;                                      // wave-uniform
    double sn[MAXCOL], sd[MAXCOL];
#pragma unroll
    for (int m = 0; m < MAXCOL; ++m) sn[m] = sd[m] = 0.0;
    for (int j = lane; j < a.C; j += 64) {
        uint32_t c[4] = {(uint32_t)b, (uint32_t)(j >> 2), 0u, 1u};
        philox4x32_10(c, a.k0, a.k1);
        const uint32_t w = (j & 3) == 0 ? c[0] : (j & 3) == 1 ? c[1] : (j & 3) == 2 ? c[2] : c[3];
        const int64_t row = point ? j : (int64_t)__umulhi(w, (uint32_t)a.C);      // < C
        const double* __restrict__ n = a.N + row * a.ld;
        const double* __restrict__ d = a.D + row * a.ld;
#pragma unroll
        for (int m = 0; m < MAXCOL; ++m)
            if (m < a.M) {
                sn[m] = sn[m] + n[m];
                sd[m] = sd[m] + d[m];
            }
    }
    double R[MAXCOL];
#pragma unroll
    for (int m = 0; m < MAXCOL; ++m) R[m] = m < a.M ? wave_sum_d(sn[m]) / wave_sum_d(sd[m]) : __builtin_nan("");
    for (int s = lane; s < a.S; s += 64) {
        const int ci = a.contrast[4 * s], cj = a.contrast[4 * s + 1], ck = a.contrast[4 * s + 2], cl = a.contrast[4 * s + 3];
        double v = boot_pick(R, ci);
        if (cj != -1) v = v - boot_pick(R, cj);
        if (ck != -1) {
            double u = boot_pick(R, ck);
            if (cl != -1) u = u - boot_pick(R, cl);
            v = v / u;
        }
        if (point)
            a.estimate[s] = v;
        else
            a.stat[(int64_t)s * a.B + b] = v;
    }
}

struct SummaryArgs {
    const double* stat;
    int S, B;
    const double* q;
    int Q, ntiles;
    double *mean, *sd, *quant;
    int *n_valid, *n_le0, *n_ge0;
};

// ((w0 + w1) + w2) + w3 of the four waves' butterfly totals; result in every thread.  Two barriers: call from block-uniform flow.
__device__ __forceinline__ double boot_block_sum(double v, double* sh4) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

__global__ __launch_bounds__(256) void boot_moments_kernel(const SummaryArgs a) {
    __shared__ double sh4[4];
    __shared__ int cnt[3][4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ v = a.stat + (int64_t)s * a.B;
    int nv = 0, nle = 0, nge = 0;
    double sum = 0.0;
    for (int i = tid; i < a.B; i += 256) {
        const double x = v[i];
        const bool ok = x == x;
        nv += ok;
        nle += ok && x <= 0.0;
        nge += ok && x >= 0.0;
        sum = sum + (ok ? x : 0.0);
    }
    nv = wave_sum_i(nv);
    nle = wave_sum_i(nle);
    nge = wave_sum_i(nge);
    if ((tid & 63) == 0) {
        cnt[0][tid >> 6] = nv;
        cnt[1][tid >> 6] = nle;
        cnt[2][tid >> 6] = nge;
    }
    const double total = boot_block_sum(sum, sh4);                     // its barriers publish cnt too
    nv = cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3];
    nle = cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3];
    nge = cnt[2][0] + cnt[2][1] + cnt[2][2] + cnt[2][3];
    const double nan = __builtin_nan("");
    const double mean = nv > 0 ? total / (double)nv : nan;
    double ss = 0.0;
    for (int i = tid; i < a.B; i += 256) {
        const double x = v[i];
        const double d = x - mean;
        ss = ss + (x == x ? d * d : 0.0);
    }
    const double sst = boot_block_sum(ss, sh4);
    for (int k = tid; k < a.Q; k += 256) a.quant[(int64_t)s * a.Q + k] = nan;
    if (tid == 0) {
        a.n_valid[s] = nv;
        a.n_le0[s] = nle;
        a.n_ge0[s] = nge;
        a.mean[s] = mean;
        a.sd[s] = nv > 1 ? __builtin_sqrt(sst / (double)(nv - 1)) : nan;
    }
}

// after boot_moments_kernel on the same stream: reads n_valid, overwrites the quantiles of a statistic that has a valid replicate
__global__ __launch_bounds__(256) void boot_rank_kernel(const SummaryArgs a) {
    __shared__ double tile[256];
    const int s = (int)(blockIdx.x / (unsigned)a.ntiles), tid = threadIdx.x;
    const int i = (int)(blockIdx.x % (unsigned)a.ntiles) * 256 + tid;
    const double* __restrict__ v = a.stat + (int64_t)s * a.B;
    const double x = i < a.B ? v[i] : __builtin_nan("");
    int rank = 0;
    for (int j0 = 0; j0 < a.B; j0 += 256) {                            // block-uniform trip count: every thread meets every barrier
        __syncthreads();
        tile[tid] = j0 + tid < a.B ? v[j0 + tid] : __builtin_nan("");
        __syncthreads();
        const int before = i - j0;                                     // tile entries t < before come before i
#pragma unroll 8
        for (int t = 0; t < 256; ++t) {
            const double y = tile[t];
            rank += (y < x) || (y == x && t < before);
        }
    }
    if (!(x == x)) return;                                             // past the last barrier
    const int nv = a.n_valid[s];
    for (int k = 0; k < a.Q; ++k) {
        const int want = min(max((int)ceil(a.q[k] * (double)nv) - 1, 0), nv - 1);
        if (rank == want) a.quant[(int64_t)s * a.Q + k] = x;
    }
}

}  // namespace

extern "C" int sp_boot_max_columns(void) { return MAXCOL; }

extern "C" int sp_boot_cluster_sums(const double* num, const double* den, const int64_t* start, const int* count, int G, int C, int M,
                                    double* N, double* D, void* stream) {
    if (!num || !den || !start || !count || !N || !D) return SP_ENULL;
    if (G < 1 || C < 1 || C > MAXCLUSTERS || M < 1) return SP_EINVAL;
    const int64_t total = (int64_t)C * M;
    if (sp_cdiv(total, 256) > (int64_t)INT32_MAX) return SP_EINVAL;
    const SumArgs a{num, den, start, count, G, C, M, N, D};
    hipLaunchKernelGGL(boot_cluster_sums_kernel, dim3((unsigned)sp_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_boot_resample(const double* N, const double* D, int C, int M, int ld, const int* contrast, int S, int B, uint64_t seed,
                                double* stat, double* estimate, void* stream) {
    if (!N || !D || !contrast || !stat || !estimate) return SP_ENULL;
    if (C < 1 || C > MAXCLUSTERS || M < 1 || M > MAXCOL || ld < M || S < 1 || B < 1) return SP_EINVAL;
    const ResampleArgs a{N, D, C, M, ld, contrast, S, B, (uint32_t)seed, (uint32_t)(seed >> 32), stat, estimate};
    hipLaunchKernelGGL(boot_resample_kernel, dim3((unsigned)sp_cdiv((int64_t)B + 1, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_boot_summarise(const double* stat, int S, int B, const double* q, int Q, double* mean, double* sd, double* quant,
                                 int* n_valid, int* n_le0, int* n_ge0, void* stream) {
    if (!stat || !mean || !sd || !n_valid || !n_le0 || !n_ge0) return SP_ENULL;
    if (Q > 0 && (!q || !quant)) return SP_ENULL;
    if (S < 1 || B < 1 || Q < 0) return SP_EINVAL;
    const int ntiles = (int)sp_cdiv(B, 256);
    if ((int64_t)S * ntiles > (int64_t)INT32_MAX) return SP_EINVAL;
    const SummaryArgs a{stat, S, B, q, Q, ntiles, mean, sd, quant, n_valid, n_le0, n_ge0};
    hipLaunchKernelGGL(boot_moments_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    if (Q > 0) {
        hipLaunchKernelGGL(boot_rank_kernel, dim3((unsigned)((int64_t)S * ntiles)), dim3(256), 0, (hipStream_t)stream, a);
        SP_LAUNCH_CHECK();
    }
    return SP_OK;
}
