// The model's own fixation density in closed form: the expected fixation map of the sampler's scanpaths, read off the
// T step distributions of one eval-mode forward without drawing a sample.  Built into libscanpaths_amd_model.so
// (include/scanpaths_amd_model.h), NOT into libscanpaths_amd.so or libscanpaths_amd_stats.so, whose entry points are pinned; common.h and
// scan_common.h are header-only, so the step normalisation, the limits and the arithmetic rule are the single copies.
// Fixation t of a sample exists iff no terminate was drawn up to and including step t, and its cell is drawn from step t's map alone,
// so the expected count at cell i is sum_t A_t c_t(i): c_t(i) = p_t(i) / D_t is the probability of cell i AND no terminate at step t
// (the cells of a step add up to 1 - q_t, as in scanrecur.hip), A_t that of being alive before it.  A duration is drawn per (row,
// step) independently of the cell, so the duration-weighted map is the same sum with the step's mean duration as a weight: the
// caller's step_weight [R][T], computed on the host (no transcendental runs here).  float64, every operation rounded on its own
// (scan_common.h: contraction OFF, plain operators).
//
// THE DEFINITION, Tm = min(T, max_steps), stop_t = (t >= min_length), and THE ORDER OF EVERY SUM:
//   Z_t, D_t, q_t, bad_t = the step normalisation of scan_common.h (scan_step_mass: lane l adds cells l, l + 64, .. from 0.0, then the
//            xor butterfly 32 .. 1; scan_step_norm), the code the saccade, turn, search and recurrence kernels run, so bad rows agree;
//   A_0 = 1.0, A_{t+1} = A_t * (1.0 - q_t) in ASCENDING t;
//   w_t = A_t * (1.0 - q_t);  s_t = step_weight[r][t], or absent;  f_t = A_t * s_t (A_t itself without a weight);
//   c_t(i) = (double)p_t[1 + i] / D_t;
//   e_r(i) = sum_t c_t(i) * f_t in ASCENDING t from 0.0, every term the rounded quotient times the rounded f_t, rounded, then added;
//   fixations[r] = sum_t w_t in ASCENDING t from 0.0;
//   m_g(i) = sum of e_r(i) over the good rows of group g in ASCENDING ROW INDEX from 0.0 (e_r(i) is complete before it is added);
//   maps[g][px] = sum of m_g(i) over the cells with cell_pixel[i] == px in ASCENDING CELL INDEX from 0.0; a pixel no cell maps to is
//            0.0, an empty group is a zero map.
//
//   scan_expect_steps_kernel: ONE WAVEFRONT PER ROW, four per block.  The wave walks the Tm steps; every lane holds the same Z, D, q, A
//     (the butterfly leaves the same bits in all lanes), lane 0 writes f_t and D_t into work and fixations / bad of the row.  A row is
//     BAD (bad 1, fixations NaN, nothing added) iff some step t < Tm has D_t zero or not finite or a step_weight that is not finite or
//     negative: the wave leaves at that step (wave-uniform), what it has not written of work is never read.  row_group outside
//     [0, ngroups): bad -1, fixations NaN, nothing of the row is read.
//   scan_expect_order_kernel: one thread per cell.  The cells sorted by (pixel, cell index) -- the rank of cell i is the number of cells
//     that come before it, counted by walking cell_pixel once per thread (at most 2048 x 2048 comparisons a call) -- go to work as keys
//     [P] and cells [P]; a rank is a bijection, so every slot is written exactly once.  A cell_pixel outside [0, H W) sorts behind every
//     pixel under the key H W, which no pixel looks up: its mass is skipped and nothing is stored outside maps.
//   scan_expect_cells_kernel: one thread per (group, cell), a block's 256 threads on consecutive cells of ONE group, so the float32 reads
//     of a step map coalesce and the group test is block-uniform.  Walks the rows in ascending index and the steps of each good row of
//     its group; writes m_g(i) into work.
//   scan_expect_pixels_kernel: one thread per (group, pixel), consecutive threads on consecutive pixels (coalesced stores).  Lower bound
//     of its pixel among the sorted keys (at most 11 halvings), then the cells of the run in order.  Every element of maps is written
//     exactly once.
// work (doubles): f [R][Tm] | D [R][Tm] | m [ngroups][P] | keys int [P] | cells int [P].  No LDS, no floating-point atomics, no memset;
// all stores are plain vector stores.
#include "common.h"
#include "scan_common.h"
#include "../../include/scanpaths_amd_model.h"

namespace {

struct ExpectArgs {
    const float* probs;
    const double* step_weight;
    const int *row_group, *cell_pixel;
    int R, T, Tm, P, ngroups, min_length, HW;
    double *f, *D, *m, *maps, *fixations;
    int *keys, *cells, *bad;
};

__global__ __launch_bounds__(256) void scan_expect_steps_kernel(const ExpectArgs a) {
    int lane;
    int64_t r;
    if (!scan_wave_item(a.R, lane, r)) return;
    const int g = a.row_group[r];
    const double nan = __builtin_nan("");
    if (g < 0 || g >= a.ngroups) {                                   // wave-uniform: nothing of the row is read
        if (lane == 0) {
            a.bad[r] = -1;
            a.fixations[r] = nan;
        }
        return;
    }
    const float* __restrict__ prow = a.probs + r * a.T * (int64_t)(a.P + 1);
    const double* __restrict__ sw = a.step_weight ? a.step_weight + r * a.T : nullptr;
    double* __restrict__ f = a.f + r * a.Tm;
    double* __restrict__ D = a.D + r * a.Tm;
    double A = 1.0, fix = 0.0;
    for (int t = 0; t < a.Tm; ++t) {
        const float* __restrict__ p = prow + (int64_t)t * (a.P + 1);
        const ScanStep st = scan_step_norm(scan_step_mass(p, a.P, lane), p, t >= a.min_length);
        const double s = sw ? sw[t] : 1.0;
        if (st.bad || !isfinite(s) || s < 0.0) {                     // the same bits in every lane: a wave-uniform exit
            if (lane == 0) {
                a.bad[r] = 1;
                a.fixations[r] = nan;
            }
            return;
        }
        const double w = A * (1.0 - st.q);
        fix = fix + w;
        if (lane == 0) {
            f[t] = sw ? A * s : A;
            D[t] = st.D;
        }
        A = w;                                                       // A_{t+1} = A_t * (1.0 - q_t)
    }
    if (lane == 0) {
        a.bad[r] = 0;
        a.fixations[r] = fix;
    }
}

__global__ __launch_bounds__(256) void scan_expect_order_kernel(const ExpectArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    const int pi = a.cell_pixel[i];
    const int ki = pi >= 0 && pi < a.HW ? pi : a.HW;
    int rank = 0;
    for (int j = 0; j < a.P; ++j) {
        const int pj = a.cell_pixel[j];
        const int kj = pj >= 0 && pj < a.HW ? pj : a.HW;
        rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    a.keys[rank] = ki;                                               // rank < P: at most P - 1 cells come before cell i
    a.cells[rank] = i;
}

__global__ __launch_bounds__(256) void scan_expect_cells_kernel(const ExpectArgs a) {
    const int chunks = (a.P + 255) / 256;
    const int g = (int)(blockIdx.x / (unsigned)chunks);              // block-uniform
    const int i = (int)(blockIdx.x % (unsigned)chunks) * 256 + threadIdx.x;
    if (i >= a.P) return;
    double m = 0.0;
    for (int r = 0; r < a.R; ++r) {
        if (a.row_group[r] != g || a.bad[r] != 0) continue;
        const float* __restrict__ p = a.probs + (int64_t)r * a.T * (int64_t)(a.P + 1) + 1 + i;
        const double* __restrict__ f = a.f + (int64_t)r * a.Tm;
        const double* __restrict__ D = a.D + (int64_t)r * a.Tm;
        double e = 0.0;
        for (int t = 0; t < a.Tm; ++t) e = e + ((double)p[(int64_t)t * (a.P + 1)] / D[t]) * f[t];
        m = m + e;
    }
    a.m[(int64_t)g * a.P + i] = m;
}

__global__ __launch_bounds__(256) void scan_expect_pixels_kernel(const ExpectArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.ngroups * a.HW) return;
    const int g = (int)(i / a.HW), px = (int)(i % a.HW);
    int lo = 0, hi = a.P;                                            // the first k with keys[k] >= px
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.keys[mid] < px) lo = mid + 1;
        else hi = mid;
    }
    const double* __restrict__ mg = a.m + (int64_t)g * a.P;
    double v = 0.0;
    for (int k = lo; k < a.P && a.keys[k] == px; ++k) v = v + mg[a.cells[k]];      // cells[k] in [0, P): written by a rank
    a.maps[i] = v;
}

}  // namespace

extern "C" int sp_model_abi_version(void) { return SP_MODEL_ABI_VERSION; }
extern "C" int sp_model_max_fixations(void) { return MAXFIX; }
extern "C" int sp_model_max_cells(void) { return MAXCELLS; }

static bool expect_scalars_ok(int R, int T, int Hm, int Wm, int ngroups, int max_steps) {
    return R >= 0 && T >= 1 && scan_map_ok(Hm, Wm) && ngroups >= 0 && max_steps >= 1 && max_steps <= MAXFIX;
}

extern "C" int64_t sp_model_fixation_expectation_workspace(int R, int T, int Hm, int Wm, int ngroups, int max_steps) {
    if (!expect_scalars_ok(R, T, Hm, Wm, ngroups, max_steps)) return SP_EINVAL;
    const int64_t Tm = T < max_steps ? T : max_steps, P = (int64_t)Hm * Wm;
    return 2 * (int64_t)R * Tm + (int64_t)ngroups * P + P;           // two int arrays [P] take the room of P doubles
}

extern "C" int sp_model_fixation_expectation(const float* probs, const double* step_weight, const int* row_group, int R, int T, int Hm,
                                             int Wm, int ngroups, int min_length, int max_steps, const int* cell_pixel, int H, int W,
                                             double* work, double* maps, double* fixations, int* bad, void* stream) {
    if (!probs || !row_group || !cell_pixel) return SP_ENULL;
    if (!work || !maps || !fixations || !bad) return SP_ENULL;
    if (!expect_scalars_ok(R, T, Hm, Wm, ngroups, max_steps) || min_length < 0 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)INT32_MAX)
        return SP_EINVAL;
    const int Tm = T < max_steps ? T : max_steps, P = Hm * Wm, HW = H * W;
    const int chunks = (P + 255) / 256;
    if ((int64_t)ngroups * chunks > (int64_t)INT32_MAX || sp_cdiv((int64_t)ngroups * HW, 256) > (int64_t)INT32_MAX) return SP_EINVAL;
    double* const f = work;
    double* const D = f + (int64_t)R * Tm;
    double* const m = D + (int64_t)R * Tm;
    int* const keys = (int*)(m + (int64_t)ngroups * P);
    const ExpectArgs a{probs, step_weight, row_group, cell_pixel, R, T, Tm, P, ngroups, min_length, HW, f, D, m, maps, fixations,
                       keys, keys + P, bad};
    hipStream_t s = (hipStream_t)stream;
    if (R > 0) {
        hipLaunchKernelGGL(scan_expect_steps_kernel, dim3((unsigned)sp_cdiv(R, 4)), dim3(256), 0, s, a);
        SP_LAUNCH_CHECK();
    }
    if (ngroups > 0) {
        hipLaunchKernelGGL(scan_expect_order_kernel, dim3((unsigned)chunks), dim3(256), 0, s, a);
        SP_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_expect_cells_kernel, dim3((unsigned)((int64_t)ngroups * chunks)), dim3(256), 0, s, a);
        SP_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_expect_pixels_kernel, dim3((unsigned)sp_cdiv((int64_t)ngroups * HW, 256)), dim3(256), 0, s, a);
        SP_LAUNCH_CHECK();
    }
    return SP_OK;
}
