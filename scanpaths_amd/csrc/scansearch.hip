// Target-search efficiency: did a scanpath reach the target box, and how fast -- for scanpaths that exist (humans,
// samples: scan_target_hits_kernel) and, in closed form, for the model's own step distributions (scan_target_mass_kernel).  float64,
// every operation rounded on its own (the arithmetic rule of scan_common.h: contraction OFF, plain operators).  A box is (x_min, y_min,
// x_max, y_max), HALF-OPEN: a point is inside iff x_min <= x < x_max && y_min <= y < y_max, by comparisons in double -- no box coordinate
// is ever converted to an integer, so boxes of 1e300, negative, empty, inverted or NaN boxes are harmless: they hold nothing.
//
//   scan_target_hits_kernel: ONE WAVEFRONT PER SCANPATH, four per block, one lane per fixation.  Only the first m = min(n, max_steps)
//     fixations count; a fixation with a non-finite coordinate is never inside.  hit = the lowest lane inside (a ballot).  path = d_1 +
//     d_2 + .. + d_hit, d_i = scan_dist(fix_i - fix_{i-1}), added LEFT TO RIGHT IN INDEX ORDER starting from 0.0 (every lane runs the
//     same hit-step loop over shuffled d_i); spr = scan_dist(fix_0 - centre) / path, centre = ((x_min + x_max) / 2, (y_min + y_max) / 2),
//     not clipped.  hit 0: path 0, spr 1.  No hit: -1, NaN, NaN.  A non-finite coordinate before the hit: path and spr NaN.  A count
//     outside [0, MAXFIX]: -1, NaN, NaN and none of its rows is read.
//
//   scan_target_mass_kernel: ONE BLOCK PER BOX, four waves.  The pixel the sampler emits for column c is the FLOAT32 value
//     fmaf((float)c, xg, 0.5f * xg), xg = (float)(frame_w / Wm), widened to double; rows likewise with yg.  csrc/sampling.hip
//     scanpath_kernel writes (float)c * xg + 0.5f * xg under the default contraction and compiles to ONE fused multiply-add per axis
//     (v_pk_fma_f32): the product is not rounded on its own.  The unfused form differs from it by an ulp where c * xg is inexact (row 6
//     of a 7-row map on 75 pixels), so the fusion is written out here -- this file compiles with contraction off -- and
//     tests/test_search_efficiency_gpu.py holds the two kernels equal cell by cell.  A cell belongs to the box iff that pixel is inside.
//     The pixel is monotone in c, so the members are a rectangle [r0, r1) x [c0, c1): every wave finds the first and the last member
//     column and row by ballots over the Wm and Hm centre values (NaN compares false: no member).  cells = (r1 - r0) * (c1 - c0).  Every
//     index into probs is built from these clamped ranges and from a box_row checked against R.
//     Steps are taken in rounds of four, wave w of round k owns step t = 4 k + w.  THE ORDER OF EVERY SUM:
//       Z_t   = scan_step_mass of scan_common.h (the order of scansaccade.hip, scanturn.hip and scanlik.hip, a function of P alone);
//       box_t = the box's cells numbered j = 0 .. cells - 1 in row-major order of the rectangle (cell (r0 + j / w, c0 + j % w), w = c1 -
//               c0): lane l adds j = l, l + 64, .. in that order from 0.0; the same butterfly.  No sum crosses waves.
//     (D_t, q_t) = scan_step_norm(Z_t, ..) of scan_common.h, on lane 0 only;  m_t = box_t / D_t.  Lane 0 of the
//     wave leaves (m_t, q_t, D_t) in LDS (double-buffered by round: one barrier per round); thread 0 of the block then runs the recursion
//     in step order: A_0 = 1, HIT_t = A_t * m_t, TFP_t = TFP_{t-1} + HIT_t (from 0.0, left to right), A_{t+1} = A_t * ((1 - q_t) - m_t);
//     MASS_t = m_t.  D_t == 0, or a NaN in D_t, m_t or q_t, poisons the box: NaN in MASS, HIT and TFP at that step and every later one.
//     A box_row outside [0, R): cells -1 and NaN everywhere, nothing of probs is read.
// Both kernels write every element of every output they are given, use no atomics and store with plain vector stores only.
#include "common.h"
#include "scan_common.h"

namespace {

constexpr int MAXSIDE = 1024;     // Hm, Wm at most this: the ballot loops run at most 16 rounds per axis

__global__ __launch_bounds__(256) void scan_target_hits_kernel(const double* __restrict__ fix, int ncol, const int64_t* __restrict__ start,
                                                               const int* __restrict__ count, const double* __restrict__ box, int nscan,
                                                               int max_steps, int* __restrict__ hit, double* __restrict__ path,
                                                               double* __restrict__ spr) {
    int lane;
    int64_t s;
    if (!scan_wave_item(nscan, lane, s)) return;
    const double nan = __builtin_nan("");
    const int n = count[s];
    int h = -1;
    double len = nan, ratio = nan;
    if (!scan_count_bad(n)) {
        const int m = min(n, max_steps);
        const double x0 = box[4 * s], y0 = box[4 * s + 1], x1 = box[4 * s + 2], y1 = box[4 * s + 3];
        double x = 0.0, y = 0.0;
        bool finite = true, in = false;
        if (lane < m) {
            const double* __restrict__ f = fix + (start[s] + lane) * ncol;
            x = f[0];
            y = f[1];
            finite = isfinite(x) && isfinite(y);
            in = finite && x0 <= x && x < x1 && y0 <= y && y < y1;
        }
        const unsigned long long inside = __ballot(in), broken = __ballot(!finite);
        if (inside) {
            h = __ffsll((long long)inside) - 1;
            const double xp = __shfl_up(x, 1, 64), yp = __shfl_up(y, 1, 64);
            const double d = lane > 0 ? scan_dist(x - xp, y - yp) : 0.0;
            len = 0.0;
            for (int i = 1; i <= h; ++i) len = len + __shfl(d, i, 64);         // h is wave-uniform: left to right
            const double fx = __shfl(x, 0, 64), fy = __shfl(y, 0, 64);
            ratio = h == 0 ? 1.0 : scan_dist(fx - (x0 + x1) / 2.0, fy - (y0 + y1) / 2.0) / len;
            if (broken & ((1ull << h) - 1ull)) len = ratio = nan;               // a non-finite coordinate before the hit
        }
    }
    if (lane == 0) {
        if (hit) hit[s] = h;
        if (path) path[s] = len;
        if (spr) spr[s] = ratio;
    }
}

// the members of one axis: [first, last + 1) of the k < n with lo <= fmaf((float)k, g, 0.5f * g) < hi, (0, 0) without one; wave-uniform
__device__ __forceinline__ void axis_range(int n, float g, double lo, double hi, int lane, int& first, int& end) {
    first = 0;
    end = 0;
    bool found = false;
    const float half = 0.5f * g;
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        const double c = (double)__builtin_fmaf((float)k, g, half);
        const unsigned long long mem = __ballot(k < n && lo <= c && c < hi);
        if (mem) {
            if (!found) first = base + __ffsll((long long)mem) - 1;
            found = true;
            end = base + 64 - __clzll((long long)mem);
        }
    }
}

struct MassArgs {
    const float* probs;
    const double* box;
    const int* box_row;
    int R, T, Hm, Wm, min_length;
    float xg, yg;
    double *MASS, *HIT, *TFP;
    int* cells;
};

__global__ __launch_bounds__(256) void scan_target_mass_kernel(const MassArgs a) {
    __shared__ double sh[2][4][3];                                  // [round parity][wave] (m, q, D)
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double nan = __builtin_nan("");
    const int row = a.box_row[b];
    const bool row_ok = row >= 0 && row < a.R;                      // block-uniform
    int c0, c1, r0, r1;
    axis_range(a.Wm, a.xg, a.box[4 * b], a.box[4 * b + 2], lane, c0, c1);
    axis_range(a.Hm, a.yg, a.box[4 * b + 1], a.box[4 * b + 3], lane, r0, r1);
    const int bw = c1 - c0, ncell = bw * (r1 - r0);                 // <= 1024 * 1024
    const int P = a.Hm * a.Wm;
    if (threadIdx.x == 0 && a.cells) a.cells[b] = row_ok ? ncell : -1;

    double A = 1.0, tfp = 0.0;                                      // thread 0's recursion
    bool poisoned = !row_ok;
    const int rounds = (a.T + 3) >> 2;
    for (int k = 0; k < rounds; ++k) {
        const int t = 4 * k + wave;
        if (t < a.T && row_ok) {                                    // wave-uniform
            const float* __restrict__ p = a.probs + ((int64_t)row * a.T + t) * (int64_t)(P + 1);
            double in = 0.0;
            for (int j = lane; j < ncell; j += 64) in = in + (double)p[1 + (r0 + j / bw) * a.Wm + c0 + j % bw];
            const double Z = scan_step_mass(p, P, lane), B = wave_sum_d(in);
            if (lane == 0) {                                        // a bad step poisons the box below: thread 0 reads it off D
                const ScanStep st = scan_step_norm(Z, p, t >= a.min_length);
                sh[k & 1][wave][0] = B / st.D;
                sh[k & 1][wave][1] = st.q;
                sh[k & 1][wave][2] = st.D;
            }
        }
        __syncthreads();                                            // round k is in LDS; round k - 1's slots (the other parity) are free
        if (threadIdx.x == 0) {
            for (int w = 0; w < 4 && 4 * k + w < a.T; ++w) {
                const int64_t o = b * a.T + 4 * k + w;
                double m = nan, hitp = nan, cum = nan;
                if (!poisoned) {
                    const double mt = sh[k & 1][w][0], q = sh[k & 1][w][1], D = sh[k & 1][w][2];
                    poisoned = D == 0.0 || D != D || mt != mt || q != q;
                    if (!poisoned) {
                        m = mt;
                        hitp = A * mt;
                        tfp = tfp + hitp;
                        cum = tfp;
                        A = A * ((1.0 - q) - mt);
                    }
                }
                if (a.MASS) a.MASS[o] = m;
                if (a.HIT) a.HIT[o] = hitp;
                if (a.TFP) a.TFP[o] = cum;
            }
        }
    }
}

}  // namespace

extern "C" int sp_scan_target_hits(const double* fix, int ncol, const int64_t* start, const int* count, const double* box, int nscan,
                                   int max_steps, int* hit, double* path, double* spr, void* stream) {
    if (!fix || !start || !count || !box) return SP_ENULL;
    if (!hit && !path && !spr) return SP_ENULL;
    if (ncol < 2 || nscan < 1 || max_steps < 1) return SP_EINVAL;
    hipLaunchKernelGGL(scan_target_hits_kernel, dim3((unsigned)sp_cdiv(nscan, 4)), dim3(256), 0, (hipStream_t)stream, fix, ncol, start,
                       count, box, nscan, max_steps, hit, path, spr);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_scan_target_mass(const float* probs, const double* box, const int* box_row, int R, int T, int Hm, int Wm, int NB,
                                   double frame_w, double frame_h, int min_length, double* MASS, double* HIT, double* TFP, int* cells,
                                   void* stream) {
    if (!probs || !box || !box_row) return SP_ENULL;
    if (!MASS && !HIT && !TFP && !cells) return SP_ENULL;
    if (R < 1 || T < 1 || Hm < 1 || Wm < 1 || NB < 1 || min_length < 0) return SP_EINVAL;
    if (Hm > MAXSIDE || Wm > MAXSIDE) return SP_EINVAL;
    if (!scan_frame_ok(frame_w, frame_h)) return SP_EINVAL;
    const MassArgs a{probs, box, box_row, R, T, Hm, Wm, min_length, (float)(frame_w / Wm), (float)(frame_h / Hm), MASS, HIT, TFP, cells};
    hipLaunchKernelGGL(scan_target_mass_kernel, dim3((unsigned)NB), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
