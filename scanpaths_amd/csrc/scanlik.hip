// Human scanpaths under the model's own step distributions: per-fixation log-likelihood, information gain over a
// baseline, NSS and AUC of each decode step's conditional map at the human fixation of that step, the log-normal duration density, and
// the per-step continue / terminate log-probabilities.  probs [R][T][1 + P] float32 (action 0 = terminate, action 1 + row * Wm + col =
// a cell, models/sampling.py); every probability enters the arithmetic as the float32 value converted exactly to float64, and every
// operation is rounded on its own (the arithmetic rule of scan_common.h: contraction OFF, plain operators).
//
//   scan_likelihood_kernel: ONE WAVEFRONT PER (row, step), four per block.  The wave loads the step's P <= 2048 cell values once into
//     32 registers per lane (cell c in lane c % 64, slot c / 64; fully unrolled and predicated, no dynamically indexed array, no LDS, no
//     atomics) and reduces Z = sum p, min, max and the two-pass sum of (p - Z/P)^2 once: every lane adds its slots in slot order, the 64
//     partial sums are combined by the xor butterfly 32, 16, .., 1 -- an order that depends on P alone, never on what else is in the
//     call.  The wave then walks the scanpaths attached to its row (order[row_first[r] .. + row_n[r]]): the cell of fixation t, the
//     cell's value read again from memory (it hits the cache), the rank counts by a per-lane count over the registers and a wave integer
//     sum; lane 0 writes.  The baseline row's sum is reduced in the same order as Z, and only when the row differs from the one of the
//     scanpath before (the subjects of an image share theirs).
// The kernel writes every [s][t] element of every output it is given (NaN where nothing is scored), so callers may pass uninitialised
// buffers, and it guards itself: a scanpath of more than MAXFIX (or fewer than 0) fixations gets NaN everywhere and none of its rows
// is read.
#include "common.h"
#include "scan_common.h"

namespace {

constexpr int SLOTS = 32;         // registers per lane that hold a step's map
static_assert(SLOTS * 64 == MAXCELLS, "a step map fills the registers of one wave");

struct LikArgs {
    const float *probs, *mu, *sigma2;
    const double* baseline;
    const int* baseline_rows;
    const double* fix;
    const int64_t* start;
    const int *count, *row_first, *row_n, *order;
    int R, T, Hm, Wm, ncol;
    double frame_w, frame_h, u;
    double *LL, *IG, *NSS, *AUC, *DLL, *CONT, *TERM;
    int* dropped;
};

__global__ __launch_bounds__(256) void scan_likelihood_kernel(const LikArgs a) {
    int lane;
    int64_t rt;
    if (!scan_wave_item((int64_t)a.R * a.T, lane, rt)) return;
    const int r = (int)(rt / a.T), t = (int)(rt % a.T);
    const int P = a.Hm * a.Wm;
    const float* __restrict__ p = a.probs + rt * (int64_t)(P + 1);
    const double nan = __builtin_nan("");
    // does slot k of this lane hold a cell (k * 64 + lane < P): a wave-uniform test for every slot but the last one in use
    const int nfull = P >> 6, rem = P & 63;
    auto live = [=](int k) { return k < nfull || (k == nfull && lane < rem); };

    // ---- the step's map, once ----
    float v[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) v[k] = live(k) ? p[1 + k * 64 + lane] : 0.f;
    double z = 0.0;
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k)
        if (live(k)) {
            z = z + (double)v[k];
            lo = fminf(lo, v[k]);
            hi = fmaxf(hi, v[k]);
        }
    const double Z = wave_sum_d(z);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    const double mean = Z / (double)P;
    double q2 = 0.0;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k)
        if (live(k)) {
            const double d = (double)v[k] - mean;
            q2 = q2 + d * d;
        }
    const double sd = P >= 2 && lo != hi ? __builtin_sqrt(wave_sum_d(q2) / (double)(P - 1)) : nan;   // NaN: no NSS on this map
    const double p0 = (double)p[0];
    if (lane == 0) {
        if (a.CONT) a.CONT[rt] = log2(Z / (Z + p0));
        if (a.TERM) a.TERM[rt] = log2(p0 / (Z + p0));
    }
    const double mix = a.u / (double)P, keep = 1.0 - a.u;

    // ---- the scanpaths of the row ----
    int brow = -1;                                             // the baseline row whose sum is bsum
    double bsum = 0.0;
    const int first = a.row_first[r], ns = a.row_n[r];
    for (int i = 0; i < ns; ++i) {
        const int s = a.order[first + i];
        const int n = a.count[s];
        const int64_t o = (int64_t)s * a.T + t;
        const int m = scan_count_bad(n) ? 0 : min(n, a.T);     // fixations that meet a step
        const double* __restrict__ f = a.fix + (a.start[s] + t) * a.ncol;      // read only where t < m
        if (a.dropped && t == 0) {                             // one lane per fixation
            bool out = false;
            if (lane < m) {
                const double x = f[(int64_t)lane * a.ncol], y = f[(int64_t)lane * a.ncol + 1];
                out = !(isfinite(x) && isfinite(y)) || x < 0.0 || x >= a.frame_w || y < 0.0 || y >= a.frame_h;
            }
            const int nd = __popcll(__ballot(out));
            if (lane == 0) a.dropped[s] = nd;
        }
        double ll = nan, ig = nan, nss = nan, auc = nan, dll = nan;
        if (t < m) {
            const double x = f[0], y = f[1];
            if (a.DLL) {
                const double d = f[2], m_ = (double)a.mu[rt], s2 = (double)a.sigma2[rt];
                if (d > 0.0 && isfinite(d) && s2 > 0.0) {
                    const double ld = log(d), e = ld - m_;
                    dll = (-ld - 0.5 * log(2.0 * M_PI * s2) - e * e / (2.0 * s2)) / M_LN2;
                }
            }
            if (scan_in_frame(x, y, a.frame_w, a.frame_h)) {
                const int col = scan_cell(x, a.Wm, a.frame_w);
                const int row = scan_cell(y, a.Hm, a.frame_h);
                const int c = row * a.Wm + col;
                const float pc = p[1 + c];
                if (a.AUC) {
                    int below = 0, equal = 0;
#pragma unroll
                    for (int k = 0; k < SLOTS; ++k)
                        if (live(k)) {
                            below += v[k] < pc;
                            equal += v[k] == pc;
                        }
                    below = wave_sum_i(below);
                    equal = wave_sum_i(equal);
                    if (P >= 2) auc = ((double)below + 0.5 * (double)(equal - 1)) / (double)(P - 1);
                }
                nss = ((double)pc - mean) / sd;
                const double qc = keep * ((double)pc / Z) + mix;
                ll = log2((double)P * qc);
                if (a.IG) {
                    const int b = a.baseline_rows[s];
                    const double* __restrict__ base = a.baseline + (int64_t)b * P;
                    if (b != brow) {                           // wave-uniform
                        double bl = 0.0;
#pragma unroll
                        for (int k = 0; k < SLOTS; ++k)
                            if (live(k)) bl = bl + base[k * 64 + lane];
                        bsum = wave_sum_d(bl);
                        brow = b;
                    }
                    if (bsum > 0.0) ig = log2(qc) - log2(keep * (base[c] / bsum) + mix);
                }
            }
        }
        if (lane == 0) {
            if (a.LL) a.LL[o] = ll;
            if (a.IG) a.IG[o] = ig;
            if (a.NSS) a.NSS[o] = nss;
            if (a.AUC) a.AUC[o] = auc;
            if (a.DLL) a.DLL[o] = dll;
        }
    }
}

}  // namespace

extern "C" int sp_scan_likelihood_max_cells(void) { return MAXCELLS; }

extern "C" int sp_scan_likelihood(const float* probs, const float* mu, const float* sigma2, const double* baseline,
                                  const int* baseline_rows, const double* fix, const int64_t* start, const int* count,
                                  const int* row_first, const int* row_n, const int* order, int R, int T, int Hm, int Wm, int S, int ncol,
                                  double frame_w, double frame_h, double uniform_mix, double* LL, double* IG, double* NSS, double* AUC,
                                  double* DLL, double* CONT, double* TERM, int* dropped, void* stream) {
    if (!probs || !fix || !start || !count || !row_first || !row_n || !order) return SP_ENULL;
    if (!LL && !IG && !NSS && !AUC && !DLL && !CONT && !TERM && !dropped) return SP_ENULL;
    if ((IG && (!baseline || !baseline_rows)) || (DLL && (!mu || !sigma2))) return SP_ENULL;
    if (R < 1 || T < 1 || Hm < 1 || Wm < 1 || S < 1 || ncol < 2 || (DLL && ncol < 3)) return SP_EINVAL;
    if ((int64_t)Hm * Wm > MAXCELLS || (int64_t)R * T > (int64_t)INT32_MAX) return SP_EINVAL;
    if (!(frame_w > 0) || !(frame_w < INFINITY) || !(frame_h > 0) || !(frame_h < INFINITY)) return SP_EINVAL;
    if (!(uniform_mix >= 0) || !(uniform_mix < 1)) return SP_EINVAL;
    const LikArgs a{probs, mu, sigma2, baseline, baseline_rows, fix, start, count, row_first, row_n, order, R, T, Hm, Wm, ncol,
                    frame_w, frame_h, uniform_mix, LL, IG, NSS, AUC, DLL, CONT, TERM, dropped};
    hipLaunchKernelGGL(scan_likelihood_kernel, dim3((unsigned)sp_cdiv((int64_t)R * T, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
