// Gaussian kernel sums between fixations with a leave-group-out rule, at K bandwidths at once: the KDE centre-bias
// baseline of "IG" and the human gold standard of the likelihood scorers (scanlik.hip, §19).  N fixations (x, y) in rows of ncol
// doubles, SORTED BY IMAGE: image g owns rows img_start[g] .. img_start[g + 1], in an order that the caller fixes from the image's own
// data (scanpath by scanpath, step by step).  path[i] / step[i]: the scanpath and the position t of fixation i.  A fixation outside the
// frame or with a non-finite coordinate is dropped: no source, NaN as a query.  The cell kernel of source j at bandwidth b is the
// separable softmax form  k_j(c) = wy_j(row) wx_j(col),  wx_j(col) = exp(ax(col) - max ax) / sum_col exp(ax(col) - max ax),
// ax(col) = -(cx(col) - x_j)^2 / (2 b^2),  cx(col) = (col + 0.5) w / Wm  (wy likewise): it sums to 1 over the map whatever b is.
//
//   kde_prep_kernel    one thread per (source, bandwidth): the two axis maxima and the two normalisers, 4 doubles; the sums run over
//                      the columns (rows) in index order.  The axis weights themselves are never stored.
//   kde_table_kernel   one block per (image, bandwidth): own[g][k][c] = sum of k_j(c) over the image's valid sources IN THE IMAGE'S
//                      ORDER; the sources' axis weights are staged through LDS in tiles, every thread keeps its <= 8 cells in registers.
//   kde_others_kernel  one thread per (bandwidth, cell): others[g] = (own[0] + .. + own[g - 1]) + (own[G - 1] + .. + own[g + 1]), two
//                      serial passes over the images: the other images are summed DIRECTLY, never as total - own, so nothing cancels, a
//                      call with one image gets an exact zero row, and a cell no other image reaches stays an exact zero.
//   kde_image_kernel   one thread per (query, bandwidth): the leave="image" score from the query's cell of others[g].
//   kde_pair_kernel    leave="scanpath" / "scanpath_step": one thread per (query, bandwidth), blocks of 256 items of ONE image (the
//                      host lists them), the image's sources staged through LDS in tiles of 32 -- an image may hold any number of
//                      fixations.  Every thread adds its sources serially in the image's order.
// No floating-point atomics; no sum's order depends on the launch geometry or on what else is in the call.  Every element of every
// output is written.  float64 under the arithmetic rule of scan_common.h.
#include "common.h"
#include "scan_common.h"

namespace {

constexpr int MAXBW = 16;          // = sp_scan_kde_max_bandwidths(): a source's 4 * K prologue values of a 32-source tile fit 16 KB of LDS
constexpr int SLOTS = MAXCELLS / 256;
constexpr int WBUF = 4096;         // doubles of staged axis weights per tile: at least one source (Hm + Wm <= MAXCELLS + 1)
constexpr int TILE = 32;           // sources per tile of the pair kernel

struct KdeArgs {
    const double* fix;
    const int *path, *step, *img, *blocks;
    const int64_t* img_start;
    int64_t N;
    int ncol, G, K, Hm, Wm, leave;
    double frame_w, frame_h, u;
    double bw[MAXBW];
    double *prep, *own, *tables, *LL;
    int *nother, *others, *valid;
};

struct Cell {
    int col, row;                  // col < 0: dropped
};

__device__ __forceinline__ Cell kde_cell(const KdeArgs& a, double x, double y) {
    if (!(isfinite(x) && isfinite(y) && x >= 0.0 && x < a.frame_w && y >= 0.0 && y < a.frame_h)) return {-1, -1};
    return {min((int)floor((x * (double)a.Wm) / a.frame_w), a.Wm - 1), min((int)floor((y * (double)a.Hm) / a.frame_h), a.Hm - 1)};
}

// the exponent of a source at v on an axis of n cells of a side of length len, at cell i
__device__ __forceinline__ double kde_arg(int i, double len, int n, double v, double den) {
    const double d = (((double)i + 0.5) * len) / (double)n - v;
    return -(d * d) / den;
}

__device__ __forceinline__ void kde_axis(double len, int n, double v, double den, double& mx, double& sum) {
    mx = kde_arg(0, len, n, v, den);
    for (int i = 1; i < n; ++i) {
        const double e = kde_arg(i, len, n, v, den);
        mx = e > mx ? e : mx;
    }
    sum = 0.0;
    for (int i = 0; i < n; ++i) sum = sum + exp(kde_arg(i, len, n, v, den) - mx);
}

__global__ __launch_bounds__(256) void kde_prep_kernel(const KdeArgs a) {
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= a.N * a.K) return;
    const int64_t j = item / a.K;
    const int k = (int)(item % a.K);
    const double x = a.fix[j * a.ncol], y = a.fix[j * a.ncol + 1];
    double* __restrict__ o = a.prep + item * 4;
    if (kde_cell(a, x, y).col < 0) {                           // never read: a dropped fixation is no source
        o[0] = o[1] = o[2] = o[3] = 0.0;
        return;
    }
    const double b = a.bw[k], den = 2.0 * b * b;
    kde_axis(a.frame_w, a.Wm, x, den, o[0], o[1]);
    kde_axis(a.frame_h, a.Hm, y, den, o[2], o[3]);
}

__global__ __launch_bounds__(256) void kde_table_kernel(const KdeArgs a) {
    __shared__ double w[WBUF];
    __shared__ int part[4];
    const int g = blockIdx.x / a.K, k = blockIdx.x % a.K, tid = threadIdx.x;
    const int P = a.Hm * a.Wm, L = a.Wm + a.Hm, per = WBUF / L;
    const int64_t first = a.img_start[g], n = a.img_start[g + 1] - first;
    const double b = a.bw[k], den = 2.0 * b * b;
    double acc[SLOTS];
    int at[SLOTS];                                             // row * L + col of the slot's cell: where its two weights sit in a source's L
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int c = s * 256 + tid;
        acc[s] = 0.0;
        at[s] = c < P ? (c / a.Wm) << 16 | (c % a.Wm) : -1;
    }
    int nvalid = 0;
    for (int64_t j0 = 0; j0 < n; j0 += per) {
        const int m = (int)min((int64_t)per, n - j0);
        __syncthreads();
        for (int e = tid; e < m * L; e += 256) {               // the tile's axis weights: wx [Wm], then wy [Hm], of every source
            const int64_t j = first + j0 + e / L;
            const int i = e % L;
            const double x = a.fix[j * a.ncol], y = a.fix[j * a.ncol + 1];
            const double* __restrict__ p = a.prep + (j * a.K + k) * 4;
            double v = 0.0;                                    // a dropped fixation adds +0 to every cell: it changes no sum
            if (kde_cell(a, x, y).col >= 0) {
                if (i == 0) ++nvalid;
                v = i < a.Wm ? exp(kde_arg(i, a.frame_w, a.Wm, x, den) - p[0]) / p[1]
                             : exp(kde_arg(i - a.Wm, a.frame_h, a.Hm, y, den) - p[2]) / p[3];
            }
            w[e] = v;
        }
        __syncthreads();
        for (int s = 0; s < m; ++s) {
            const double* __restrict__ ws = w + s * L;
#pragma unroll
            for (int q = 0; q < SLOTS; ++q)
                if (at[q] >= 0) acc[q] = acc[q] + ws[a.Wm + (at[q] >> 16)] * ws[at[q] & 0xffff];
        }
    }
    double* __restrict__ o = a.own + (int64_t)blockIdx.x * P;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
        if (at[s] >= 0) o[s * 256 + tid] = acc[s];
    if (k == 0) {                                              // the image's valid sources: an integer sum, any order
        nvalid = wave_sum_i(nvalid);
        if ((tid & 63) == 0) part[tid >> 6] = nvalid;
        __syncthreads();
        if (tid == 0) a.nother[g] = part[0] + part[1] + part[2] + part[3];
    }
}

__global__ __launch_bounds__(256) void kde_others_kernel(const KdeArgs a) {
    const int64_t KP = (int64_t)a.K * a.Hm * a.Wm, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) {                                              // nother: the image's own count -> the other images' count
        int total = 0;
        for (int g = 0; g < a.G; ++g) total += a.nother[g];
        for (int g = 0; g < a.G; ++g) a.nother[g] = total - a.nother[g];
    }
    if (e >= KP) return;
    double run = 0.0;
    for (int g = 0; g < a.G; ++g) {
        a.tables[g * KP + e] = run;
        run = run + a.own[g * KP + e];
    }
    run = 0.0;
    for (int g = a.G - 1; g >= 0; --g) {
        a.tables[g * KP + e] = a.tables[g * KP + e] + run;
        run = run + a.own[g * KP + e];
    }
}

__device__ __forceinline__ double kde_bits(const KdeArgs& a, double sum, int M) {
    const int P = a.Hm * a.Wm;
    return log2((double)P * ((1.0 - a.u) * (sum / (double)M) + a.u / (double)P));
}

__global__ __launch_bounds__(256) void kde_image_kernel(const KdeArgs a) {
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= a.N * a.K) return;
    const int64_t i = item / a.K;
    const int k = (int)(item % a.K), g = a.img[i], M = a.nother[g], P = a.Hm * a.Wm;
    const Cell c = kde_cell(a, a.fix[i * a.ncol], a.fix[i * a.ncol + 1]);
    a.LL[item] = c.col >= 0 && M > 0 ? kde_bits(a, a.tables[((int64_t)g * a.K + k) * P + c.row * a.Wm + c.col], M) : __builtin_nan("");
    if (k == 0) {
        a.others[i] = M;
        a.valid[i] = c.col >= 0;
    }
}

__global__ __launch_bounds__(256) void kde_pair_kernel(const KdeArgs a) {
    __shared__ double sxy[TILE][2], sprep[TILE * MAXBW * 4];
    __shared__ int spath[TILE], sstep[TILE];                   // spath < 0: a dropped source
    const int g = a.blocks[2 * blockIdx.x], tid = threadIdx.x;
    const int64_t first = a.img_start[g], n = a.img_start[g + 1] - first;
    const int64_t item = (int64_t)a.blocks[2 * blockIdx.x + 1] * 256 + tid;      // (query, bandwidth) of the image
    const bool live = item < n * a.K;
    const int64_t i = first + (live ? item / a.K : 0);
    const int k = live ? (int)(item % a.K) : 0;
    const Cell c = kde_cell(a, a.fix[i * a.ncol], a.fix[i * a.ncol + 1]);
    const int ipath = a.path[i], istep = a.step[i];
    const double b = a.bw[k], den = 2.0 * b * b;
    const double cx = (((double)c.col + 0.5) * a.frame_w) / (double)a.Wm, cy = (((double)c.row + 0.5) * a.frame_h) / (double)a.Hm;
    double so = 0.0, ss = 0.0;                                 // other scanpaths; other scanpaths at the same step
    int no = 0, ns = 0;
    for (int64_t j0 = 0; j0 < n; j0 += TILE) {
        const int m = (int)min((int64_t)TILE, n - j0);
        __syncthreads();
        if (tid < m) {
            const int64_t j = first + j0 + tid;
            const double x = a.fix[j * a.ncol], y = a.fix[j * a.ncol + 1];
            sxy[tid][0] = x;
            sxy[tid][1] = y;
            spath[tid] = kde_cell(a, x, y).col >= 0 ? a.path[j] : -1;
            sstep[tid] = a.step[j];
        }
        for (int e = tid; e < m * a.K * 4; e += 256) sprep[e] = a.prep[(first + j0) * a.K * 4 + e];
        __syncthreads();
        if (live)
            for (int s = 0; s < m; ++s) {
                if (spath[s] < 0 || spath[s] == ipath) continue;
                const bool same = sstep[s] == istep;
                ++no;
                ns += same;
                if (c.col < 0) continue;
                const double* __restrict__ p = sprep + (s * a.K + k) * 4;
                const double dx = cx - sxy[s][0], dy = cy - sxy[s][1];
                const double wx = exp(-(dx * dx) / den - p[0]) / p[1], wy = exp(-(dy * dy) / den - p[2]) / p[3];
                const double kk = wy * wx;
                so = so + kk;
                if (same) ss = ss + kk;
            }
    }
    if (!live) return;
    const int M = a.leave == 1 ? no : ns;
    a.LL[i * a.K + k] = c.col >= 0 && M > 0 ? kde_bits(a, a.leave == 1 ? so : ss, M) : __builtin_nan("");
    if (k == 0) {
        a.others[i] = M;
        a.valid[i] = c.col >= 0;
    }
}

}  // namespace

extern "C" int sp_scan_kde_max_bandwidths(void) { return MAXBW; }

extern "C" int sp_scan_kde(const double* fix, const int* path, const int* step, const int* img, const int64_t* img_start,
                           const int* blocks, int64_t N, int ncol, int G, int nblocks, const double* bandwidths, int K, int Hm, int Wm,
                           double frame_w, double frame_h, double uniform_mix, int leave, double* prep, double* own, int* nother,
                           double* tables, double* LL, int* others, int* valid, void* stream) {
    if (!fix || !img_start || !bandwidths || !prep) return SP_ENULL;
    if (leave == 0 ? !own || !nother || !tables || (LL && (!img || !others || !valid))
                   : !path || !step || !blocks || !LL || !others || !valid)
        return SP_ENULL;
    if (leave < 0 || leave > 2 || N < 0 || G < (leave == 0 ? 0 : 1) || nblocks < 0 || ncol < 2 || Hm < 1 || Wm < 1) return SP_EINVAL;
    if (K < 1 || K > MAXBW || (int64_t)Hm * Wm > MAXCELLS) return SP_EINVAL;
    for (int k = 0; k < K; ++k)
        if (!(bandwidths[k] > 0) || !(bandwidths[k] < INFINITY)) return SP_EINVAL;
    if (!(frame_w > 0) || !(frame_w < INFINITY) || !(frame_h > 0) || !(frame_h < INFINITY)) return SP_EINVAL;
    if (!(uniform_mix >= 0) || !(uniform_mix < 1)) return SP_EINVAL;
    const int64_t KP = (int64_t)K * Hm * Wm;
    if (N * K > (int64_t)INT32_MAX * 256 || (int64_t)G * K > (int64_t)INT32_MAX) return SP_EINVAL;
    KdeArgs a{fix, path, step, img, blocks, img_start, N, ncol, G, K, Hm, Wm, leave, frame_w, frame_h, uniform_mix, {},
              prep, own, tables, LL, nother, others, valid};
    for (int k = 0; k < K; ++k) a.bw[k] = bandwidths[k];
    hipStream_t st = (hipStream_t)stream;
    const unsigned nk = (unsigned)sp_cdiv(N * K, 256);
    if (nk) {
        hipLaunchKernelGGL(kde_prep_kernel, dim3(nk), dim3(256), 0, st, a);
        SP_LAUNCH_CHECK();
    }
    if (leave == 0) {
        if (G) {
            hipLaunchKernelGGL(kde_table_kernel, dim3((unsigned)(G * K)), dim3(256), 0, st, a);
            SP_LAUNCH_CHECK();
            hipLaunchKernelGGL(kde_others_kernel, dim3((unsigned)sp_cdiv(KP, 256)), dim3(256), 0, st, a);
            SP_LAUNCH_CHECK();
        }
        if (LL && nk) {
            hipLaunchKernelGGL(kde_image_kernel, dim3(nk), dim3(256), 0, st, a);
            SP_LAUNCH_CHECK();
        }
    } else if (nblocks) {
        hipLaunchKernelGGL(kde_pair_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, a);
        SP_LAUNCH_CHECK();
    }
    return SP_OK;
}
