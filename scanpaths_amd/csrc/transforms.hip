// The reference's per-sample dataset transforms, batched on the device.
//
//   * images: transforms.Resize((H, W)) -> ToTensor() -> Normalize(mean, std) of torchvision 0.7 on PIL input (AiR/train.py:43-46,
//     OSIE/train.py:41-45, COCO_Search18/train.py:41-45).  Resize is Pillow's 8-bit BILINEAR: a horizontal pass into a uint8
//     intermediate, then a vertical pass, both with 22-bit fixed-point coefficients (the host builds Pillow's tables in float64,
//     scanpaths_amd/transforms.py).  One thread per output pixel recomputes the <= ky horizontal taps of its column (the reads stay in
//     L1/L2), so the intermediate never goes to memory; an axis that keeps its size gets the identity table, which gives exactly the
//     skipped pass.  ToTensor / Normalize are single correctly rounded float32 operations (no contraction, no reciprocal).
//   * maps: skimage 0.17.2 resize(map, out_shape) with its defaults -- Gaussian anti-aliasing prefilter (ndimage mode 'mirror',
//     truncate 4, float64 sums stored as float32 after each axis), bilinear sampling with 'reflect' borders, clip -- followed by the
//     dataset's normalisation (AiR/dataset/dataset.py:151-154: /= max; COCO_Search18/dataset/dataset.py:159: /= max + 1e-7).  The
//     axis-0 pass runs only on the <= 2h source rows the bilinear step reads (launch 1), the axis-1 pass only at the four points each
//     output reads (launch 2, float64 samples to a workspace); launch 3 (one workgroup per map) takes the max and writes the
//     normalised float32 or float64 maps.
//   * boxes: the binary box maps (COCO detector boxes, AiR scene-graph objects) rasterised from integer rectangles into uint8 maps,
//     which then go through the map resize.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int PREC = 22;              // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)

__device__ __forceinline__ int clip8(int v) {          // Pillow's clip8: (v >> 22) clamped to [0, 255]
    v >>= PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// meta: [B][4] = (H_i, W_i, offset of the horizontal table, offset of the vertical table) in int words from meta.
// A table for out outputs: [ksize][out x (min, n)][out x ksize coefficients].
__global__ __launch_bounds__(NT) void resize_normalize_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
                                                              const int* __restrict__ meta, int H, int W, float m0, float m1,
                                                              float m2, float s0, float s1, float s2, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int* mb = meta + 4 * b;
    const int Wi = mb[1];
    const int* ht = meta + mb[2];
    const int* vt = meta + mb[3];
    const int kx = ht[0], ky = vt[0];
    const uint8_t* img = src + src_off[b];
    const int64_t plane = (int64_t)H * W;
    float* ob = out + (int64_t)b * 3 * plane;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < plane; p += (int64_t)gridDim.x * NT) {
        const int oy = (int)(p / W), ox = (int)(p - (int64_t)oy * W);
        const int xmin = ht[1 + 2 * ox], nx = ht[2 + 2 * ox];
        const int* cx = ht + 1 + 2 * W + ox * kx;
        const int ymin = vt[1 + 2 * oy], ny = vt[2 + 2 * oy];
        const int* cy = vt + 1 + 2 * H + oy * ky;
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < ny; ++j) {
            const uint8_t* row = img + ((int64_t)(ymin + j) * Wi + xmin) * 3;
            int h0 = 1 << (PREC - 1), h1 = h0, h2 = h0;
            for (int i = 0; i < nx; ++i) {
                const int k = cx[i];
                h0 += (int)row[3 * i] * k;
                h1 += (int)row[3 * i + 1] * k;
                h2 += (int)row[3 * i + 2] * k;
            }
            const int k = cy[j];
            a0 += clip8(h0) * k;
            a1 += clip8(h1) * k;
            a2 += clip8(h2) * k;
        }
        // ToTensor: x / 255 ; Normalize: (x - mean) / std -- each one IEEE float32 operation
        ob[p] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(a0), 255.f), m0), s0);
        ob[plane + p] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(a1), 255.f), m1), s1);
        ob[2 * plane + p] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(a2), 255.f), m2), s2);
    }
}

// ndimage 'mirror' (skimage 'reflect'): d c b | a b c d | c b a, periodic beyond one reflection
__device__ __forceinline__ int mirror(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i = i < 0 ? -i : i;
    i %= period;
    return i >= n ? period - i : i;
}

template <typename T>
__device__ __forceinline__ double load_map(const T* m, int64_t idx) {
    return (double)(float)m[idx];
}

// axis-0 Gaussian pass at (r, c): ndimage's symmetric correlate1d order -- centre tap, then (left + right) * w from the outermost
// pair inwards, float64, stored as float32
template <typename T>
__device__ __forceinline__ float pass0(const T* m, int h, int w, int C, int ch, int r, int c, int R, const double* wt) {
    double acc = load_map(m, ((int64_t)r * w + c) * C + ch) * wt[0];
    for (int j = R; j >= 1; --j)
        acc += (load_map(m, ((int64_t)mirror(r - j, h) * w + c) * C + ch) + load_map(m, ((int64_t)mirror(r + j, h) * w + c) * C + ch)) *
               wt[j];
    return (float)acc;
}

// source coordinate of output index o along an axis of n_in samples resized to n_out (float64, no contraction)
__device__ __forceinline__ double src_coord(int o, int n_in, int n_out) { return ((double)n_in / (double)n_out) * ((double)o + 0.5) - 0.5; }

// Stage 1: the axis-0 pass at the (at most 2h) source rows the bilinear step reads -- row k of map b = floor (k even) / ceil (k odd) of
// output row k / 2's source coordinate -- over all w_b columns: rows [B][2h][wmax][C] float32.
// dims [B][2] = (h_i, w_i); filt [B][4] = (R0, offset of the axis-0 half kernel in wts, R1, offset of the axis-1 half kernel):
// wts[off + j] = weight of distance j, j = 0..R
template <typename T>
__global__ __launch_bounds__(NT) void filter_rows_kernel(const T* __restrict__ src, const int64_t* __restrict__ src_off,
                                                         const int* __restrict__ dims, const int* __restrict__ filt,
                                                         const double* __restrict__ wts, int C, int h, int wmax, float* __restrict__ rows) {
    const int b = blockIdx.y;
    const int hi = dims[2 * b], wi = dims[2 * b + 1];
    const int R0 = filt[4 * b];
    const double* w0 = wts + filt[4 * b + 1];
    const T* m = src + src_off[b];
    const int64_t n = (int64_t)2 * h * wi * C;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const int ch = (int)(e % C);
        const int64_t q = e / C;
        const int k = (int)(q / wi), c = (int)(q - (int64_t)k * wi);
        const double r = src_coord(k >> 1, hi, h);
        const int ri = mirror((int)((k & 1) ? ceil(r) : floor(r)), hi);
        rows[(((int64_t)b * 2 * h + k) * wmax + c) * C + ch] = pass0(m, hi, wi, C, ch, ri, c, R0, w0);
    }
}

// axis-1 pass of one stage-1 row at column c (same order as pass0), rounded to float32 as ndimage stores it
__device__ __forceinline__ double pass1(const float* row, int w, int C, int c, int R, const double* wt) {
    double acc = (double)row[(int64_t)c * C] * wt[0];
    for (int j = R; j >= 1; --j) acc += ((double)row[(int64_t)mirror(c - j, w) * C] + (double)row[(int64_t)mirror(c + j, w) * C]) * wt[j];
    return (double)(float)acc;
}

// Stage 2: the axis-1 pass at the four points each output reads, bilinear, clip; float64 samples to ws [B][h][w][C]
__global__ __launch_bounds__(NT) void resize_maps_kernel(const float* __restrict__ rows, const int* __restrict__ dims,
                                                         const int* __restrict__ filt, const double* __restrict__ wts, int C, int h, int w,
                                                         int wmax, double* __restrict__ ws) {
    const int b = blockIdx.y;
    const int hi = dims[2 * b], wi = dims[2 * b + 1];
    const int R1 = filt[4 * b + 2];
    const double* w1 = wts + filt[4 * b + 3];
    const int64_t n = (int64_t)h * w * C;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const int ch = (int)(e % C);
        const int64_t pix = e / C;
        const int y = (int)(pix / w), x = (int)(pix - (int64_t)y * w);
        const double r = src_coord(y, hi, h), c = src_coord(x, wi, w);
        const double fr = floor(r), fc = floor(c);
        const double dr = r - fr, dc = c - fc;
        const int mc0 = mirror((int)fc, wi), mc1 = mirror((int)ceil(c), wi);
        const float* row0 = rows + ((int64_t)b * 2 * h + 2 * y) * wmax * C + ch;      // floor(r), then ceil(r)
        const float* row1 = row0 + (int64_t)wmax * C;
        const double tl = pass1(row0, wi, C, mc0, R1, w1);
        const double tr = pass1(row0, wi, C, mc1, R1, w1);
        const double bl = pass1(row1, wi, C, mc0, R1, w1);
        const double br = pass1(row1, wi, C, mc1, R1, w1);
        const double top = (1.0 - dc) * tl + dc * tr;
        const double bottom = (1.0 - dc) * bl + dc * br;
        double v = (1.0 - dr) * top + dr * bottom;
        // skimage clips to the filtered map's [min, max]; a convex combination leaves its four points' range only by rounding
        const double lo = fmin(fmin(tl, tr), fmin(bl, br)), hi_v = fmax(fmax(tl, tr), fmax(bl, br));
        v = v < lo ? lo : (v > hi_v ? hi_v : v);
        ws[(int64_t)b * n + e] = v;
    }
}

// one workgroup per map: norm 0 = none, 1 = / max, 2 = / (max + eps); float64 arithmetic, one rounding to the output type
__global__ __launch_bounds__(NT) void normalise_maps_kernel(const double* __restrict__ ws, int64_t n, int norm, double eps, int out_f64,
                                                            void* __restrict__ out) {
    __shared__ double sh[NT / 64];
    const int b = blockIdx.x;
    const double* v = ws + (int64_t)b * n;
    double div = 1.0;
    if (norm) {
        double mx = -INFINITY;
        for (int64_t i = threadIdx.x; i < n; i += NT) mx = fmax(mx, v[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
        __syncthreads();
        mx = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
        div = norm == 2 ? mx + eps : mx;
    }
    for (int64_t i = threadIdx.x; i < n; i += NT) {
        const double q = norm ? v[i] / div : v[i];
        if (out_f64)
            ((double*)out)[(int64_t)b * n + i] = q;
        else
            ((float*)out)[(int64_t)b * n + i] = (float)q;
    }
}

// boxes [nbox][5] = (y0, y1, x0, x1, channel), half-open, already clipped to the map; sample b owns boxes box_start[b] ..
// box_start[b + 1] - 1.  Every element of every map is written (1 inside a box of its channel, else 0).
__global__ __launch_bounds__(NT) void rasterize_boxes_kernel(const int* __restrict__ boxes, const int* __restrict__ box_start,
                                                             const int64_t* __restrict__ dst_off, const int* __restrict__ dims, int C,
                                                             uint8_t* __restrict__ dst) {
    const int b = blockIdx.y;
    const int hi = dims[2 * b], wi = dims[2 * b + 1];
    const int k0 = box_start[b], k1 = box_start[b + 1];
    uint8_t* m = dst + dst_off[b];
    const int64_t n = (int64_t)hi * wi * C;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const int ch = (int)(e % C);
        const int64_t pix = e / C;
        const int y = (int)(pix / wi), x = (int)(pix - (int64_t)y * wi);
        uint8_t on = 0;
        for (int k = k0; k < k1; ++k) {
            const int* bx = boxes + 5 * k;
            on |= (uint8_t)(bx[4] == ch && y >= bx[0] && y < bx[1] && x >= bx[2] && x < bx[3]);
        }
        m[e] = on;
    }
}

inline int grid_x(int64_t work) { return (int)(sp_cdiv(work, NT) < 1024 ? sp_cdiv(work, NT) : 1024); }

}  // namespace

extern "C" int sp_resize_normalize_images(const uint8_t* src, const int64_t* src_off, const int* meta, int B, int H, int W, float mean0,
                                          float mean1, float mean2, float std0, float std1, float std2, float* out, void* stream) {
    if (!src || !src_off || !meta || !out) return SP_ENULL;
    if (B < 1 || B > 65535 || H < 1 || W < 1) return SP_EINVAL;
    hipLaunchKernelGGL(resize_normalize_kernel, dim3(grid_x((int64_t)H * W), B), dim3(NT), 0, (hipStream_t)stream, src, src_off, meta,
                       H, W, mean0, mean1, mean2, std0, std1, std2, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

// workspace: the float64 samples [B][h][w][C], then the stage-1 rows [B][2h][wmax][C] float32
extern "C" int64_t sp_resize_maps_workspace(int B, int h, int w, int C, int wmax) {
    if (B < 1 || h < 1 || w < 1 || C < 1 || wmax < 1) return 0;
    return (int64_t)B * h * w * C * (int64_t)sizeof(double) + (int64_t)B * 2 * h * wmax * C * (int64_t)sizeof(float);
}

extern "C" int sp_resize_maps(const void* src, int src_u8, const int64_t* src_off, const int* dims, const int* filt, const double* wts,
                              int B, int C, int h, int w, int wmax, int norm, double eps, int out_f64, void* workspace, void* out,
                              void* stream) {
    if (!src || !src_off || !dims || !filt || !wts || !workspace || !out) return SP_ENULL;
    if (B < 1 || B > 65535 || C < 1 || h < 1 || w < 1 || wmax < 1 || norm < 0 || norm > 2) return SP_EINVAL;
    const int64_t n = (int64_t)h * w * C;
    const hipStream_t s = (hipStream_t)stream;
    double* samples = (double*)workspace;
    float* rows = (float*)(samples + (int64_t)B * n);
    const int64_t nrows = (int64_t)2 * h * wmax * C;
    if (src_u8)
        hipLaunchKernelGGL(filter_rows_kernel<uint8_t>, dim3(grid_x(nrows), B), dim3(NT), 0, s, (const uint8_t*)src, src_off, dims, filt,
                           wts, C, h, wmax, rows);
    else
        hipLaunchKernelGGL(filter_rows_kernel<float>, dim3(grid_x(nrows), B), dim3(NT), 0, s, (const float*)src, src_off, dims, filt, wts,
                           C, h, wmax, rows);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(resize_maps_kernel, dim3(grid_x(n), B), dim3(NT), 0, s, (const float*)rows, dims, filt, wts, C, h, w, wmax, samples);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(normalise_maps_kernel, dim3(B), dim3(NT), 0, s, (const double*)samples, n, norm, eps, out_f64, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_rasterize_boxes(const int* boxes, const int* box_start, const int64_t* dst_off, const int* dims, int B, int C,
                                  int max_elems, uint8_t* dst, void* stream) {
    if (!box_start || !dst_off || !dims || !dst) return SP_ENULL;
    if (B < 1 || B > 65535 || C < 1 || max_elems < 1) return SP_EINVAL;
    hipLaunchKernelGGL(rasterize_boxes_kernel, dim3(grid_x(max_elems), B), dim3(NT), 0, (hipStream_t)stream, boxes, box_start, dst_off,
                       dims, C, dst);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
