// Fixation and density maps from scanpaths, float64: the producers of the saliency-map metrics' inputs (salmaps.hip
// saliency_metrics_kernel).  The reference has no such code: its callers rasterise with numpy and blur with
// scipy.ndimage.gaussian_filter on the host; the pixel rule and the filter below restate those two.
//
// fixation_maps_kernel   one workgroup per map.  Thread t OWNS the pixels p with p % 256 == t: it zeroes them, then every thread walks
//                        the map's fixations in input order (scanpath by scanpath, fixation by fixation) and applies the ones that
//                        land on a pixel it owns.  No atomics, one writer per pixel: duration sums add in np.add.at's order.
//                        The scanpaths of the map are found 256 at a time: one ballot per wave, the four masks walked by all threads.
// blur_axis_kernel       one correlate1d pass (axis 0 or axis 1) of a strip of 32 lines through LDS; each thread slides a window of
//                        8 outputs along the filtered axis: one LDS load, one (scalar) weight and 8 fp64 FMAs per tap.
// normalise_maps_kernel  one workgroup per map: sum or max in a fixed order, then the division.
#include "common.h"
#include <algorithm>
#include <cmath>

namespace {
constexpr int NT = 256;

__global__ __launch_bounds__(NT) void fixation_maps_kernel(const double* __restrict__ fix, int ncol, const int64_t* __restrict__ start,
                                                           const int* __restrict__ count, const int* __restrict__ group, int K, int H,
                                                           int W, double frame_w, double frame_h, int weight,
                                                           double* __restrict__ maps, int* __restrict__ dropped) {
    __shared__ unsigned long long mask[NT / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int P = H * W;
    double* __restrict__ m = maps + (int64_t)g * P;
    for (int p = tid; p < P; p += NT) m[p] = 0.0;
    int ndrop = 0;                                   // every thread counts the same drops; thread 0 reports them
    for (int k0 = 0; k0 < K; k0 += NT) {
        const int k = k0 + tid;
        const unsigned long long b = __ballot(k < K && group[k] == g);
        __syncthreads();                             // the previous chunk's masks have been walked
        if ((tid & 63) == 0) mask[tid >> 6] = b;
        __syncthreads();
        for (int w = 0; w < NT / 64; ++w) {
            unsigned long long mm = mask[w];
            while (mm) {
                const int kk = k0 + w * 64 + __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                const double* __restrict__ f = fix + start[kk] * ncol;
                const int n = count[kk];
                for (int i = 0; i < n; ++i, f += ncol) {
                    const double x = f[0], y = f[1];
                    if (!(isfinite(x) && isfinite(y)) || x < 0.0 || x >= frame_w || y < 0.0 || y >= frame_h) {
                        ++ndrop;
                        continue;
                    }
                    const int col = min((int)floor((x * (double)W) / frame_w), W - 1);
                    const int row = min((int)floor((y * (double)H) / frame_h), H - 1);
                    const int p = row * W + col;
                    if ((p & (NT - 1)) != tid) continue;
                    if (weight == 0) m[p] = 1.0;
                    else if (weight == 1) m[p] += 1.0;
                    else m[p] += f[2];
                }
            }
        }
    }
    if (tid == 0) dropped[g] = ndrop;
}

__global__ __launch_bounds__(NT) void count_positive_kernel(const double* __restrict__ x, int P, int* __restrict__ out) {
    __shared__ int tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    const double* __restrict__ r = x + (int64_t)blockIdx.x * P;
    int c = 0;
    for (int p = threadIdx.x; p < P; p += NT) c += r[p] > 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&tot, c);      // integer: order-free
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// ---- separable Gaussian filter ---------------------------------------------------------------------------------------------------------
constexpr int BL = 32;                   // lines of the filtered axis per workgroup
constexpr int BP = BL + 1;               // LDS pitch: the transposing load of the contiguous axis writes at stride BP (odd: conflict-free)
constexpr int BR = 8;                    // outputs per thread along the filtered axis
constexpr int BLUR_LDS_MAX = 160 * 1024;
constexpr int BLUR_MAX_AXIS = BLUR_LDS_MAX / (BP * 8);

enum { MODE_CONSTANT = 0, MODE_REFLECT = 1, MODE_NEAREST = 2 };

// element i of a line of length L extended by `mode` (scipy's names); the value of the line lives at s[i * BP]
__device__ __forceinline__ double ext_value(const double* s, int i, int L, int mode) {
    if (i < 0 || i >= L) {
        if (mode == MODE_CONSTANT) return 0.0;
        if (mode == MODE_NEAREST) i = i < 0 ? 0 : L - 1;
        else {                                       // reflect: d c b a | a b c d | d c b a, period 2L
            i %= 2 * L;
            if (i < 0) i += 2 * L;
            if (i >= L) i = 2 * L - 1 - i;
        }
    }
    return s[i * BP];
}

// One pass: out[a][c] = sum_{j=-R..R} w[|j|] * ext(in[.][c])[a + j] for the C lines c of length L of every map; element (a, c) is at
// a * sL + c * sC (one of the two strides is 1).  grid ceil(C / BL) * G (strip fastest), LDS L * BP doubles.
__global__ __launch_bounds__(NT) void blur_axis_kernel(const double* __restrict__ in, double* __restrict__ out, int L, int C, int64_t sL,
                                                       int64_t sC, int64_t map_stride, const double* __restrict__ w, int R, int mode) {
    extern __shared__ __attribute__((aligned(16))) double lines[];
    const int strips = (C + BL - 1) / BL;
    const int tid = threadIdx.x, c0 = (int)(blockIdx.x % strips) * BL;
    const int nc = min(BL, C - c0);
    in += (int64_t)(blockIdx.x / strips) * map_stride + c0 * sC;
    out += (int64_t)(blockIdx.x / strips) * map_stride + c0 * sC;
    if (sC == 1) {                                   // lines side by side in memory: lanes along the lines
        for (int e = tid; e < L * BL; e += NT) {
            const int a = e / BL, c = e % BL;
            if (c < nc) lines[a * BP + c] = in[a * sL + c];
        }
    } else {                                         // each line contiguous: lanes along the line, transposed into LDS
        for (int e = tid; e < L * nc; e += NT) {
            const int c = e / L, a = e % L;
            lines[a * BP + c] = in[a + c * sC];
        }
    }
    __syncthreads();
    const int c = tid % BL;
    if (c >= nc) return;
    const double* s = lines + c;
    const int nt = 2 * R + 1;
    for (int a0 = (tid / BL) * BR; a0 < L; a0 += (NT / BL) * BR) {
        double acc[BR], win[BR];                     // at tap j (after s = j % BR slides) win[(o + s) % BR] = ext[a0 - R + j + o]
#pragma unroll
        for (int o = 0; o < BR; ++o) {
            acc[o] = 0.0;
            win[o] = ext_value(s, a0 - R + o, L, mode);
        }
        for (int jb = 0; jb < nt; jb += BR) {
#pragma unroll
            for (int sft = 0; sft < BR; ++sft) {
                const int j = jb + sft;
                if (j < nt) {
                    const double wj = w[abs(j - R)];
#pragma unroll
                    for (int o = 0; o < BR; ++o) acc[o] = fma(wj, win[(o + sft) % BR], acc[o]);
                    win[sft] = ext_value(s, a0 - R + j + BR, L, mode);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < BR; ++o)
            if (a0 + o < L) out[(a0 + o) * sL + c * sC] = acc[o];
    }
}

// norm 1: / sum, 2: / max; partials per thread over p = tid, tid + 256, ..., then lanes, then the four waves: a fixed order
__global__ __launch_bounds__(NT) void normalise_maps_kernel(double* __restrict__ maps, int P, int norm) {
    __shared__ double sh[NT / 64];
    double* __restrict__ m = maps + (int64_t)blockIdx.x * P;
    double v = norm == 1 ? 0.0 : -INFINITY;
    for (int p = threadIdx.x; p < P; p += NT) v = norm == 1 ? v + m[p] : fmax(v, m[p]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = norm == 1 ? v + u : fmax(v, u);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double d = norm == 1 ? (sh[0] + sh[1]) + (sh[2] + sh[3]) : fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    if (d == 0.0) return;
    for (int p = threadIdx.x; p < P; p += NT) m[p] = m[p] / d;
}
}  // namespace

extern "C" int sp_fixation_maps(const double* fix, int ncol, const int64_t* start, const int* count, const int* group, int K, int G, int H,
                                int W, double frame_w, double frame_h, int weight, double* maps, int* dropped, void* stream) {
    if (!maps || !dropped || (K > 0 && (!fix || !start || !count || !group))) return SP_ENULL;
    if (K < 0 || G < 1 || H < 1 || W < 1 || (int64_t)H * W > (1 << 30) || ncol < 2 || weight < 0 || weight > 2 || (weight == 2 && ncol < 3) ||
        !(frame_w > 0.0) || !(frame_h > 0.0) || !std::isfinite(frame_w) || !std::isfinite(frame_h))
        return SP_EINVAL;
    hipLaunchKernelGGL(fixation_maps_kernel, dim3(G), dim3(NT), 0, (hipStream_t)stream, fix, ncol, start, count, group, K, H, W, frame_w,
                       frame_h, weight, maps, dropped);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_count_positive(const double* x, int N, int P, int* out, void* stream) {
    if (!x || !out) return SP_ENULL;
    if (N < 1 || P < 1) return SP_EINVAL;
    hipLaunchKernelGGL(count_positive_kernel, dim3(N), dim3(NT), 0, (hipStream_t)stream, x, P, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_gaussian_blur_maps_max_axis(void) { return BLUR_MAX_AXIS; }

extern "C" int64_t sp_gaussian_blur_maps_workspace(int G, int H, int W) {
    if (G < 1 || H < 1 || W < 1) return 0;
    return (int64_t)G * H * W * 8;
}

extern "C" int sp_gaussian_blur_maps(const double* in, int G, int H, int W, const double* wy, int ry, const double* wx, int rx, int mode,
                                     int norm, void* workspace, double* out, void* stream) {
    if (!in || !wy || !wx || !workspace || !out) return SP_ENULL;
    if (G < 1 || (int64_t)G * sp_cdiv(std::max(H, W), BL) > 0x7fffffff || H < 1 || W < 1 || H > BLUR_MAX_AXIS || W > BLUR_MAX_AXIS || ry < 0 || rx < 0 || ry > (1 << 24) || rx > (1 << 24) ||
        mode < MODE_CONSTANT || mode > MODE_NEAREST || norm < 0 || norm > 2)
        return SP_EINVAL;
    const int64_t P = (int64_t)H * W;
    double* tmp = (double*)workspace;
    int rc = sp_launch_lds<blur_axis_kernel, BLUR_LDS_MAX>({sp_cdiv(W, BL) * G}, NT, (size_t)H * BP * 8, (hipStream_t)stream, in, tmp,
                                                           H, W, (int64_t)W, (int64_t)1, P, wy, ry, mode);
    if (rc != SP_OK) return rc;
    rc = sp_launch_lds<blur_axis_kernel, BLUR_LDS_MAX>({sp_cdiv(H, BL) * G}, NT, (size_t)W * BP * 8, (hipStream_t)stream, (const double*)tmp, out,
                                                       W, H, (int64_t)1, (int64_t)W, P, wx, rx, mode);
    if (rc != SP_OK) return rc;
    if (norm) {
        hipLaunchKernelGGL(normalise_maps_kernel, dim3(G), dim3(NT), 0, (hipStream_t)stream, out, (int)P, norm);
        SP_LAUNCH_CHECK();
    }
    return SP_OK;
}
