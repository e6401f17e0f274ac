// Recurrence statistics: how often a scanpath comes back to a place it has already looked at, and after how many
// fixations -- the upper-triangle auto-recurrence form of Anderson et al. 2013, on action-map cells.  Built into
// libscanpaths_amd_stats.so (include/scanpaths_amd_stats.h), NOT into libscanpaths_amd.so, whose entry points are pinned; common.h and
// scan_common.h are header-only, so the pixel rule, the prologue, the step normalisation and the arithmetic rule are the single copies.
// A fixation is read as its cell (scan_lane_cell); fixations s and t are RECURRENT iff the caller's table mask [D] of bytes, D =
// (2 Hm - 1)(2 Wm - 1), is non-zero at scan_lattice_index(dr, dc) of their cell displacement.  The table is built on the host (float64:
// sqrt(dx dx + dy dy) <= radius) and only READ here, so a displacement on the boundary lands alike for humans, samples and the model.
// The result is one table [K][K] per group, K = max_steps <= MAXFIX, read as a recurrence plot: for s < t entry [s][t] holds the
// recurrent pairs (fixation s, fixation t), entry [t][s] the pairs that exist at all, entry [t][t] the fixations t.  float64, every
// operation rounded on its own (scan_common.h: contraction OFF, plain operators).
//
//   scan_recur_counts_kernel: scanpaths that exist (humans, samples).  ONE WAVEFRONT PER SCANPATH, four per block, one lane per fixation
//     (scan_lane_cell: only the first m = min(n, K) fixations count; a dropped fixation is in no pair and breaks every line through it).
//     Row i of the m x m plot is ONE 64-bit ballot over the lanes t > i (the upper triangle, main diagonal excluded); lane t adds 1 to
//     [t][t] when kept, to [t][i] when both are kept and to [i][t] when they are recurrent, with INTEGER atomic adds on int64: exact,
//     whatever the order.  scan_zero_kernel zeroes the tables first.  Per scanpath the integers of Anderson et al. 2013, rqa [6] = N
//     (kept fixations), R (recurrent points), the points on diagonal ((i, j), (i + 1, j + 1), ..), horizontal (fixed i, consecutive j)
//     and vertical (fixed j, consecutive i) lines of at least L = min_line points, and sum (j - i) over the recurrent points, j - i in
//     original ordinals: runs along a row come from the ballot, runs along a column and along a diagonal are carried per lane (the
//     diagonal's by a shuffle from lane t - 1).  A count outside [0, MAXFIX] or a group outside [0, ngroups): points -1, dropped 0,
//     rqa -1 six times, none of its rows is read, nothing is counted.
//
//   scan_recur_expect_kernel: the model, in closed form.  The step distributions are not conditioned on sampled fixations, so given
//     the image fixations s and t of a sample are independent, and the sample reaches fixation t iff no terminate was drawn up to t.
//     ONE 256-THREAD BLOCK PER (row, t), t = 0 .. Tm - 1, Tm = min(T, max_steps).  THE ORDER OF EVERY SUM:
//       Z_u, D_u, q_u = the step normalisation of scan_common.h (scan_step_mass, scan_step_norm), the code the saccade, turn and search
//                kernels run, so bad rows agree.  Wave w computes the steps u = w, w + 4, .. <= t (a function of P alone: the same bits
//                whichever wave computes them) and leaves them in LDS;
//       c_u(i) = (double)p_u[1 + i] / D_u;
//       A_0 = 1, A_{u+1} = A_u * (1.0 - q_u);
//       G_{s,t} = prod_{s<u<t} (1.0 - q_u) in ASCENDING u from 1.0;
//       B_t(i)  = sum of c_t(j) over the cells j = i + d inside the map, d the displacements with a non-zero mask entry, in ASCENDING
//                lattice index of d -- which is ascending row-major j -- from 0.0;
//       X_{s,t} = sum_i c_s(i) * B_t(i): lane l adds the cells l, l + 64, .. in that order from 0.0, every product rounded before it is
//                added, and the 64 partial sums combine by the xor butterfly 32 .. 1 (wave_sum_d);
//       E_r[s][t] = (A_s * G_{s,t}) * X_{s,t},  E_r[t][s] = (A_s * G_{s,t}) * ((1.0 - q_s) * (1.0 - q_t)),  E_r[t][t] = A_t * (1.0 - q_t).
//     LDS (dynamic): c_t and B_t in double (2 P doubles, at most 32 KB), D, q, A of the steps (3 * 64 doubles) and their bad flags.
//     scan_recur_list_kernel has listed the mask's displacements once per call (ascending lattice index, in the call's scratch), so a
//     block's work for B_t is P times the number of 1-entries of the mask.  Thread i, i + 256, .. owns cell i of B_t; the waves share
//     out the s < t (wave w takes s = w, w + 4, ..).  E_r goes to work [R][Tm][Tm]: block (r, t) writes column t above the diagonal,
//     row t below it and [t][t], so every entry of a good row is written exactly once.
//     A row is BAD iff some step u < Tm is bad (scan_step_norm): the block of t = Tm - 1 walks every step, so it writes bad 1 and points
//     NaN; a block that meets a bad step leaves (its part of work stays unwritten and is never read; the flags come from LDS, so the exit
//     is block-uniform).  row_group outside [0, ngroups): bad -1, points NaN, nothing of the row is read.
//   scan_recur_points_kernel: one thread per good row: points[r] = sum_{s<t} E_r[s][t] in ASCENDING s, then ASCENDING t, from 0.0.
//   scan_recur_group_kernel: one thread per (group, entry): E[g] = the E_r of the good rows of g in ASCENDING ROW INDEX from 0.0;
//     entries beyond Tm are 0.
// No floating-point atomics; every element of every output is written; all stores are plain vector stores.
#include "common.h"
#include "scan_common.h"
#include "../../include/scanpaths_amd_stats.h"

namespace {

// points of a 64-bit row mask that lie on runs of at least L consecutive set bits (as scandist.hip's cross-recurrence counts them)
__device__ __forceinline__ int recur_run_points(unsigned long long mask, int L) {
    if (L > MAXFIX) return 0;
    unsigned long long s = mask;                                    // bit b: a window of L set bits starts at b
    for (int k = 1; k < L; ++k) s &= mask >> k;
    unsigned long long t = s;
    for (int k = 1; k < L; ++k) t |= s << k;
    return __popcll(t);
}

struct CountArgs {
    const double* fix;
    const int64_t* start;
    const int *count, *group;
    const uint8_t* mask;
    int ncol, nscan, ngroups, max_steps, Hm, Wm, min_line;
    double frame_w, frame_h;
    unsigned long long* counts;
    int *points, *dropped, *rqa;
};

__global__ __launch_bounds__(256) void scan_recur_counts_kernel(const CountArgs a) {
    int lane;
    int64_t s;
    if (!scan_wave_item(a.nscan, lane, s)) return;
    const int n = a.count[s], g = a.group[s];
    int N = -1, R = -1, DL = -1, HL = -1, VL = -1, corm = -1, nd = 0;
    if (!scan_count_bad(n) && g >= 0 && g < a.ngroups) {              // wave-uniform
        const ScanLaneCell f = scan_lane_cell(a.fix, a.ncol, a.start, s, n, a.max_steps, lane, a.Hm, a.Wm, a.frame_w, a.frame_h);
        const int m = f.m, L = a.min_line, K = a.max_steps;          // m <= K <= MAXFIX: lane t < m owns row and column t of the table
        unsigned long long* __restrict__ tab = a.counts + (int64_t)g * K * K;
        nd = f.dropped;
        N = __popcll(__ballot(f.kept));
        R = HL = VL = DL = corm = 0;
        int vrun = 0, drun = 0;                                      // per lane: column `lane`, the diagonal through (i, lane)
        if (f.kept) atomicAdd(tab + lane * K + lane, 1ull);
        for (int i = 0; i < m; ++i) {
            const int ri = __shfl(f.row, i, 64), ci = __shfl(f.col, i, 64), ki = __shfl((int)f.kept, i, 64);
            const bool pair = ki != 0 && f.kept && lane > i;
            const bool c = pair && a.mask[scan_lattice_index(f.row - ri, f.col - ci, a.Hm, a.Wm)] != 0;
            if (pair) atomicAdd(tab + lane * K + i, 1ull);
            if (c) atomicAdd(tab + i * K + lane, 1ull);
            const unsigned long long row = __ballot(c);
            R += __popcll(row);
            HL += recur_run_points(row, L);
            int r = __shfl_up(drun, 1, 64);                          // the run that reached (i - 1, lane - 1)
            if (lane == 0) r = 0;
            if (c) {
                ++vrun;
                drun = r + 1;
                corm += lane - i;
                if (lane == m - 1 && drun >= L) DL += drun;          // the diagonal leaves the plot on the right
            } else {
                if (vrun >= L) VL += vrun;
                vrun = 0;
                if (lane < m && r >= L) DL += r;
                drun = 0;
            }
        }
        if (vrun >= L) VL += vrun;                                   // (row m - 1 holds no point: every run has ended in the loop)
        if (lane < m - 1 && drun >= L) DL += drun;
        VL = wave_sum_i(VL);
        DL = wave_sum_i(DL);
        corm = wave_sum_i(corm);
    }
    if (lane == 0) {
        a.points[s] = R;
        a.dropped[s] = nd;
        int* __restrict__ o = a.rqa + 6 * s;
        o[0] = N; o[1] = R; o[2] = DL; o[3] = HL; o[4] = VL; o[5] = corm;
    }
}

struct ExpArgs {
    const float* probs;
    const int* row_group;
    const uint8_t* mask;
    int R, T, Tm, K, Hm, Wm, ngroups, min_length;
    double *work, *E, *points;
    int *bad, *list;
};

// list[0] = the number of non-zero mask entries, list[1 ..] = their displacements (dr << 16 | dc & 0xffff) in ascending lattice index;
// one wavefront, 64 entries per ballot
__global__ __launch_bounds__(64) void scan_recur_list_kernel(const ExpArgs a) {
    const int LW = 2 * a.Wm - 1, D = (2 * a.Hm - 1) * LW, lane = threadIdx.x;
    int n = 0;
    for (int base = 0; base < D; base += 64) {
        const int d = base + lane;
        const bool on = d < D && a.mask[d] != 0;
        const unsigned long long b = __ballot(on);
        if (on) {
            const int dr = d / LW - (a.Hm - 1), dc = d % LW - (a.Wm - 1);
            a.list[1 + n + __popcll(b & ((1ull << lane) - 1ull))] = dr * 65536 + (dc & 0xffff);
        }
        n += __popcll(b);
    }
    if (lane == 0) a.list[0] = n;
}

__global__ __launch_bounds__(256) void scan_recur_expect_kernel(const ExpArgs a) {
    extern __shared__ double sh[];                                  // c_t [P] | B_t [P] | D [64] | q [64] | A [64] | bad flags int [64]
    const int P = a.Hm * a.Wm, Tm = a.Tm;
    const int r = (int)(blockIdx.x / (unsigned)Tm), t = (int)(blockIdx.x % (unsigned)Tm);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool writer = t == Tm - 1 && tid == 0;                    // the block of the last t walks every step of the row
    const double nan = __builtin_nan("");
    const int g = a.row_group[r];
    if (g < 0 || g >= a.ngroups) {                                  // block-uniform: nothing of the row is read
        if (writer) {
            a.bad[r] = -1;
            a.points[r] = nan;
        }
        return;
    }
    double* __restrict__ ct = sh;
    double* __restrict__ Bt = sh + P;
    double* __restrict__ Dl = Bt + P;
    double* __restrict__ ql = Dl + MAXFIX;
    double* __restrict__ Al = ql + MAXFIX;
    int* __restrict__ badl = (int*)(Al + MAXFIX);
    const float* __restrict__ prow = a.probs + (int64_t)r * a.T * (int64_t)(P + 1);
    for (int u = wave; u <= t; u += 4) {
        const float* __restrict__ p = prow + (int64_t)u * (P + 1);
        const ScanStep st = scan_step_norm(scan_step_mass(p, P, lane), p, u >= a.min_length);
        if (lane == 0) {
            Dl[u] = st.D;
            ql[u] = st.q;
            badl[u] = st.bad ? 1 : 0;
        }
    }
    __syncthreads();                                                // the steps 0 .. t are in LDS
    bool isbad = false;
    for (int u = 0; u <= t; ++u) isbad = isbad || badl[u] != 0;
    if (isbad) {                                                    // read from LDS by every thread: a block-uniform exit
        if (writer) {
            a.bad[r] = 1;
            a.points[r] = nan;
        }
        return;
    }
    if (writer) a.bad[r] = 0;                                       // points[r]: scan_recur_points_kernel
    if (tid == 0) {
        double A = 1.0;
        for (int u = 0; u <= t; ++u) {
            Al[u] = A;
            A = A * (1.0 - ql[u]);
        }
    }
    const float* __restrict__ pt = prow + (int64_t)t * (P + 1);
    const double Dt = Dl[t], qt = ql[t];
    for (int i = tid; i < P; i += 256) ct[i] = (double)pt[1 + i] / Dt;
    __syncthreads();                                                // c_t and A are in LDS
    const int nlist = a.list[0];
    const int* __restrict__ disp = a.list + 1;
    for (int i = tid; i < P; i += 256) {
        const int ri = i / a.Wm, ci = i % a.Wm;
        double b = 0.0;
        for (int k = 0; k < nlist; ++k) {
            const int e = disp[k];
            const int rj = ri + (e >> 16), cj = ci + (int)(short)(e & 0xffff);
            if ((unsigned)rj < (unsigned)a.Hm && (unsigned)cj < (unsigned)a.Wm) b = b + ct[rj * a.Wm + cj];
        }
        Bt[i] = b;
    }
    __syncthreads();                                                // B_t is in LDS
    double* __restrict__ w = a.work + (int64_t)r * Tm * Tm;
    if (tid == 0) w[t * Tm + t] = Al[t] * (1.0 - qt);
    for (int s = wave; s < t; s += 4) {
        const float* __restrict__ ps = prow + (int64_t)s * (P + 1);
        const double Ds = Dl[s];
        double x = 0.0;
        for (int i = lane; i < P; i += 64) x = x + ((double)ps[1 + i] / Ds) * Bt[i];
        x = wave_sum_d(x);
        if (lane == 0) {
            double G = 1.0;
            for (int u = s + 1; u < t; ++u) G = G * (1.0 - ql[u]);
            const double AG = Al[s] * G;
            w[s * Tm + t] = AG * x;
            w[t * Tm + s] = AG * ((1.0 - ql[s]) * (1.0 - qt));
        }
    }
}

// points[r] = sum_{s<t} E_r[s][t] in ascending s, then ascending t, from 0.0; a bad row keeps the NaN the kernel above wrote
__global__ __launch_bounds__(256) void scan_recur_points_kernel(const ExpArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R || a.bad[r] != 0) return;
    const double* __restrict__ w = a.work + r * a.Tm * a.Tm;
    double p = 0.0;
    for (int s = 0; s < a.Tm; ++s)
        for (int t = s + 1; t < a.Tm; ++t) p = p + w[s * a.Tm + t];
    a.points[r] = p;
}

// E[g][x][y] = the E_r[x][y] of the good rows of group g, in ascending row index from 0.0; 0 beyond Tm
__global__ __launch_bounds__(256) void scan_recur_group_kernel(const ExpArgs a) {
    const int KK = a.K * a.K;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.ngroups * KK) return;
    const int g = (int)(i / KK), e = (int)(i % KK), x = e / a.K, y = e % a.K;
    double m = 0.0;
    if (x < a.Tm && y < a.Tm)
        for (int r = 0; r < a.R; ++r)
            if (a.row_group[r] == g && a.bad[r] == 0) m = m + a.work[((int64_t)r * a.Tm + x) * a.Tm + y];
    a.E[i] = m;
}

}  // namespace

extern "C" int sp_stats_abi_version(void) { return SP_STATS_ABI_VERSION; }
extern "C" int sp_stats_max_fixations(void) { return MAXFIX; }
extern "C" int sp_stats_max_cells(void) { return MAXCELLS; }

extern "C" int sp_stats_recurrence_counts(const double* fix, int ncol, const int64_t* start, const int* count, const int* group, int nscan,
                                          int ngroups, int max_steps, int Hm, int Wm, double frame_w, double frame_h, const uint8_t* mask,
                                          int min_line, int64_t* counts, int* points, int* dropped, int* rqa, void* stream) {
    if (!fix || !start || !count || !group || !mask) return SP_ENULL;
    if (!counts || !points || !dropped || !rqa) return SP_ENULL;
    if (ncol < 2 || nscan < 1 || ngroups < 1 || max_steps < 1 || max_steps > MAXFIX || !scan_map_ok(Hm, Wm) || !scan_frame_ok(frame_w, frame_h))
        return SP_EINVAL;
    if (min_line < 2) return SP_EINVAL;
    const int64_t total = (int64_t)ngroups * max_steps * max_steps;
    if (sp_cdiv(total, 256) > (int64_t)INT32_MAX) return SP_EINVAL;
    const CountArgs a{fix, start, count, group, mask, ncol, nscan, ngroups, max_steps, Hm, Wm, min_line, frame_w, frame_h,
                      (unsigned long long*)counts, points, dropped, rqa};
    hipLaunchKernelGGL(scan_zero_kernel<unsigned long long>, dim3((unsigned)sp_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a.counts, total);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_recur_counts_kernel, dim3((unsigned)sp_cdiv(nscan, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_stats_recurrence_expectation(const float* probs, const int* row_group, int R, int T, int Hm, int Wm, int ngroups,
                                               int min_length, int max_steps, const uint8_t* mask, double* work, double* E, double* points,
                                               int* bad, void* stream) {
    if (!probs || !row_group || !mask) return SP_ENULL;
    if (!work || !E || !points || !bad) return SP_ENULL;
    if (R < 1 || T < 1 || !scan_map_ok(Hm, Wm) || ngroups < 1 || min_length < 0 || max_steps < 1 || max_steps > MAXFIX) return SP_EINVAL;
    const int Tm = T < max_steps ? T : max_steps, P = Hm * Wm;
    if ((int64_t)R * Tm > (int64_t)INT32_MAX || sp_cdiv((int64_t)ngroups * max_steps * max_steps, 256) > (int64_t)INT32_MAX) return SP_EINVAL;
    const ExpArgs a{probs, row_group, mask, R, T, Tm, max_steps, Hm, Wm, ngroups, min_length, work, E, points, bad,
                    (int*)(work + (int64_t)R * Tm * Tm)};         // the list: at most D + 1 ints behind the rows' tables
    hipLaunchKernelGGL(scan_recur_list_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    const size_t lds = ((size_t)2 * P + 3 * MAXFIX) * sizeof(double) + MAXFIX * sizeof(int);    // at most 32,768 + 1,536 + 256 bytes
    hipLaunchKernelGGL(scan_recur_expect_kernel, dim3((unsigned)((int64_t)R * Tm)), dim3(256), lds, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_recur_points_kernel, dim3((unsigned)sp_cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_recur_group_kernel, dim3((unsigned)sp_cdiv((int64_t)ngroups * max_steps * max_steps, 256)), dim3(256), 0,
                       (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
