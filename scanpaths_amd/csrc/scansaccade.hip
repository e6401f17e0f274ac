// Saccade statistics: how a scanpath moves.  A fixation is read as the action-map cell it falls in (the pixel rule of
// scan_common.h: scan_in_frame / scan_cell, the one scanlik.hip uses), a saccade is the cell displacement (dr, dc) = (row(f_{t+1}) -
// row(f_t), col(f_{t+1}) - col(f_t)), and everything is counted on ONE displacement lattice of D = (2 Hm - 1) (2 Wm - 1) entries
// (scan_lattice_index).  float64, every operation rounded on its own (the arithmetic rule of scan_common.h: contraction OFF, plain
// operators).
//
//   scan_saccade_counts_kernel: scanpaths that exist (humans, samples).  ONE WAVEFRONT PER SCANPATH, four per block, one lane per
//     fixation, read as a cell by scan_lane_cell (scan_common.h: which fixations count and which are dropped); saccade t counts iff
//     fixations t and t + 1 are both kept.  Lane t takes the cell of lane t + 1 by a shuffle and adds 1 to counts[group][entry] with an
//     INTEGER atomic add on the int64 lattice: the counts are integers, so the order in which the atomics land cannot change them.
//     scan_zero_kernel (scan_common.h) zeroes the lattice first.  A count outside [0, MAXFIX] or a group outside [0, ngroups): saccades
//     -1, dropped 0, none of its rows is read, nothing is counted.
//
//   scan_saccade_expect_kernel: the model, in closed form.  The step distributions are not conditioned on sampled fixations, so the
//     expected number of saccades of row r with displacement d is E_r[d] = sum_t A_t X_t[d], X_t[d] = sum_i c_t(i) c_{t+1}(i + d) -- a
//     cross-correlation of consecutive step maps -- with A_t the probability that the scanpath is still running at step t.
//     ONE BLOCK PER (row, tile of 256 displacements), four waves; thread k of tile j owns displacement d = 256 j + k for every step, so
//     the 64 lanes of a wave own consecutive dc of (mostly) one dr.  The block walks t serially with c_t and c_{t+1} in LDS (2 P doubles,
//     at most 32 KB, dynamic; c_{t+1} becomes the next c_t by parity).  THE ORDER OF EVERY SUM:
//       Z_t, D_t, q_t = the step normalisation of scan_common.h (scan_step_mass, scan_step_norm), shared with scanturn.hip and
//                scansearch.hip.  Every wave of the block computes it for itself (the same bits), so nothing is passed between waves;
//       c_t(i) = (double)p_t[1 + i] / D_t;
//       A_0 = 1, A_{t+1} = A_t * (1.0 - q_t);
//       X_t[d] = over the cells i = (r, c) whose partner (r + dr, c + dc) lies inside the map, in ASCENDING ROW-MAJOR i from 0.0, every
//                product rounded before it is added (rows max(0, -dr) .. min(Hm, Hm - dr) - 1, columns max(0, -dc) .. min(Wm, Wm - dc) - 1);
//       E_r[d] = sum_{t = 0}^{Tm - 2} (A_t * X_t[d]) in ascending t from 0.0, Tm = min(T, max_steps);
//       saccades[r] = sum_t A_t * ((1.0 - q_t) * (1.0 - q_{t+1})) in the same order.
//     LDS reads: for dc >= 0 the c_t(i) address is the same in all lanes of a dr (a broadcast) and the c_{t+1}(i + d) addresses are
//     consecutive doubles (ds_read_b64: 32 consecutive doubles cover the 64 banks once, no conflict); for dc < 0 the roles swap.
//     A row is BAD iff some step t < Tm is bad (scan_step_norm; the walk stops there; every wave sees the same D_t, so the exit is
//     block-uniform): bad 1, saccades NaN, the row adds nothing to its group.  row_group outside [0, ngroups): bad -1, saccades NaN,
//     nothing of the row is read.  Tm < 2: no pair, E_r = 0 and saccades 0 (a bad D_0 still makes the row bad).
//     E_r goes to work [R][D] (scratch of the call: R * D doubles; 22 MB for 600 rows on 30 x 40); scan_saccade_group_kernel, one thread
//     per (group, d), then adds the rows of its group in ASCENDING ROW INDEX from 0.0, skipping bad rows -- no floating-point atomics.
// Every element of every output is written; all stores are plain vector stores.
#include "common.h"
#include "scan_common.h"

namespace {

struct CountArgs {
    const double* fix;
    const int64_t* start;
    const int *count, *group;
    int ncol, nscan, ngroups, max_steps, Hm, Wm;
    double frame_w, frame_h;
    unsigned long long* counts;
    int *saccades, *dropped;
};

__global__ __launch_bounds__(256) void scan_saccade_counts_kernel(const CountArgs a) {
    int lane;
    int64_t s;
    if (!scan_wave_item(a.nscan, lane, s)) return;
    const int n = a.count[s], g = a.group[s];
    int ns = -1, nd = 0;
    if (!scan_count_bad(n) && g >= 0 && g < a.ngroups) {              // wave-uniform
        const ScanLaneCell f = scan_lane_cell(a.fix, a.ncol, a.start, s, n, a.max_steps, lane, a.Hm, a.Wm, a.frame_w, a.frame_h);
        nd = f.dropped;
        const int rn = __shfl_down(f.row, 1, 64), cn = __shfl_down(f.col, 1, 64), kn = __shfl_down((int)f.kept, 1, 64);
        const bool sac = lane + 1 < f.m && f.kept && kn != 0;          // m <= 64: lane 63 never has a successor
        ns = __popcll(__ballot(sac));
        if (sac) {
            const int64_t D = (int64_t)(2 * a.Hm - 1) * (2 * a.Wm - 1);
            atomicAdd(a.counts + (int64_t)g * D + scan_lattice_index(rn - f.row, cn - f.col, a.Hm, a.Wm), 1ull);
        }
    }
    if (lane == 0) {
        a.saccades[s] = ns;
        a.dropped[s] = nd;
    }
}

struct ExpArgs {
    const float* probs;
    const int* row_group;
    int R, T, Tm, Hm, Wm, ngroups, min_length, ntiles;
    double *work, *E, *saccades;
    int* bad;
};

__global__ __launch_bounds__(256) void scan_saccade_expect_kernel(const ExpArgs a) {
    extern __shared__ double sh[];                                  // [2][P]: c_t in sh[(t & 1) * P ..]
    const int P = a.Hm * a.Wm, LW = 2 * a.Wm - 1, D = (2 * a.Hm - 1) * LW;
    const int r = (int)(blockIdx.x / (unsigned)a.ntiles), tile = (int)(blockIdx.x % (unsigned)a.ntiles);
    const int tid = threadIdx.x, lane = tid & 63;
    const int d = tile * 256 + tid;
    const bool writer = tile == 0 && tid == 0;
    const double nan = __builtin_nan("");
    const int g = a.row_group[r];
    if (g < 0 || g >= a.ngroups) {                                  // block-uniform: nothing of the row is read
        if (writer) {
            a.bad[r] = -1;
            a.saccades[r] = nan;
        }
        return;
    }
    int dr = 0, dc = 0, rlo = 0, rhi = 0, clo = 0, nc = 0;          // a thread beyond the lattice owns no cell pair
    if (d < D) {
        dr = d / LW - (a.Hm - 1);
        dc = d % LW - (a.Wm - 1);
        rlo = max(0, -dr);
        rhi = min(a.Hm, a.Hm - dr);
        clo = max(0, -dc);
        nc = min(a.Wm, a.Wm - dc) - clo;
    }
    double A = 1.0, E = 0.0, sac = 0.0, qprev = 0.0;
    bool isbad = false;
    for (int t = 0; t < a.Tm; ++t) {
        const float* __restrict__ p = a.probs + ((int64_t)r * a.T + t) * (int64_t)(P + 1);
        const ScanStep st = scan_step_norm(scan_step_mass(p, P, lane), p, t >= a.min_length);
        if (st.bad) {                                               // the same bits in every wave: a block-uniform exit
            isbad = true;
            break;
        }
        const double Dt = st.D, q = st.q;
        double* __restrict__ nxt = sh + (t & 1) * P;
        for (int i = tid; i < P; i += 256) nxt[i] = (double)p[1 + i] / Dt;
        __syncthreads();                                            // c_t is in LDS
        if (t > 0) {                                                // the pair (t - 1, t); A = A_{t-1}
            const double* __restrict__ cur = sh + ((t - 1) & 1) * P;
            double x = 0.0;
            for (int rr = rlo; rr < rhi; ++rr) {
                const double* __restrict__ u = cur + rr * a.Wm + clo;
                const double* __restrict__ v = nxt + (rr + dr) * a.Wm + clo + dc;
                for (int k = 0; k < nc; ++k) x = x + u[k] * v[k];
            }
            E = E + A * x;
            sac = sac + A * ((1.0 - qprev) * (1.0 - q));
            A = A * (1.0 - qprev);
        }
        qprev = q;
        __syncthreads();                                            // c_{t-1}'s buffer is free for c_{t+1}
    }
    if (!isbad && d < D) a.work[(int64_t)r * D + d] = E;
    if (writer) {
        a.bad[r] = isbad ? 1 : 0;
        a.saccades[r] = isbad ? nan : sac;
    }
}

// E[g][d] = the E_r[d] of the good rows of group g, in ascending row index from 0.0; reads bad[] as the kernel above left it
__global__ __launch_bounds__(256) void scan_saccade_group_kernel(const ExpArgs a) {
    const int D = (2 * a.Hm - 1) * (2 * a.Wm - 1);
    const int d = (int)(blockIdx.x % (unsigned)a.ntiles) * 256 + threadIdx.x, g = (int)(blockIdx.x / (unsigned)a.ntiles);
    if (d >= D) return;
    double e = 0.0;
    if (a.Tm >= 2)
        for (int r = 0; r < a.R; ++r)
            if (a.row_group[r] == g && a.bad[r] == 0) e = e + a.work[(int64_t)r * D + d];
    a.E[(int64_t)g * D + d] = e;
}

}  // namespace

extern "C" int sp_scan_saccade_counts(const double* fix, int ncol, const int64_t* start, const int* count, const int* group, int nscan,
                                      int ngroups, int max_steps, int Hm, int Wm, double frame_w, double frame_h, int64_t* counts,
                                      int* saccades, int* dropped, void* stream) {
    if (!fix || !start || !count || !group) return SP_ENULL;
    if (!counts || !saccades || !dropped) return SP_ENULL;
    if (ncol < 2 || nscan < 1 || ngroups < 1 || max_steps < 1 || !scan_map_ok(Hm, Wm) || !scan_frame_ok(frame_w, frame_h)) return SP_EINVAL;
    const int64_t total = (int64_t)ngroups * (2 * Hm - 1) * (2 * Wm - 1);
    if (sp_cdiv(total, 256) > (int64_t)INT32_MAX) return SP_EINVAL;
    const CountArgs a{fix, start, count, group, ncol, nscan, ngroups, max_steps, Hm, Wm, frame_w, frame_h, (unsigned long long*)counts,
                      saccades, dropped};
    hipLaunchKernelGGL(scan_zero_kernel<unsigned long long>, dim3((unsigned)sp_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a.counts, total);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_saccade_counts_kernel, dim3((unsigned)sp_cdiv(nscan, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_scan_saccade_expectation(const float* probs, const int* row_group, int R, int T, int Hm, int Wm, int ngroups,
                                           int min_length, int max_steps, double* work, double* E, double* saccades, int* bad,
                                           void* stream) {
    if (!probs || !row_group) return SP_ENULL;
    if (!work || !E || !saccades || !bad) return SP_ENULL;
    if (R < 1 || T < 1 || !scan_map_ok(Hm, Wm) || ngroups < 1 || min_length < 0 || max_steps < 1) return SP_EINVAL;
    const int D = (2 * Hm - 1) * (2 * Wm - 1);                       // < 4 * MAXCELLS
    const int ntiles = (int)sp_cdiv(D, 256);
    if ((int64_t)R * ntiles > (int64_t)INT32_MAX || (int64_t)ngroups * ntiles > (int64_t)INT32_MAX) return SP_EINVAL;
    const ExpArgs a{probs, row_group, R, T, T < max_steps ? T : max_steps, Hm, Wm, ngroups, min_length, ntiles, work, E, saccades, bad};
    const size_t lds = (size_t)2 * Hm * Wm * sizeof(double);
    hipLaunchKernelGGL(scan_saccade_expect_kernel, dim3((unsigned)((int64_t)R * ntiles)), dim3(256), lds, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_saccade_group_kernel, dim3((unsigned)((int64_t)ngroups * ntiles)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
