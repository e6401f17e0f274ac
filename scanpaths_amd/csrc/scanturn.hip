// Turning angles: how the direction of a saccade depends on the direction of the saccade before it.  Fixations are read
// as action-map cells (the pixel rule of scan_common.h), a saccade is a cell displacement, and every displacement has ONE direction
// sector: the caller's table sector [D], D = (2 Hm - 1) (2 Wm - 1), entry scan_lattice_index(dr, dc) of scan_common.h, values 0 .. n - 1 for
// the n direction sectors of §22 and n for the zero displacement ("stayed in the cell").  The table is built on the host by the float64
// rule of §22 and only READ here: the device computes no atan2, so a vector on a sector boundary cannot land differently on the two sides
// of a comparison.  A table value outside [0, n] is read as n (the index is clamped; what such a table counts is unspecified).  The
// result is the transition table M [n + 1][n + 1]: M[k][k'] = the number of consecutive saccade pairs (t -> t + 1, t + 1 -> t + 2) whose
// first saccade is in sector k and whose second is in sector k'.  float64, every operation rounded on its own (scan_common.h: contraction
// OFF, plain operators).  E = (n + 1)^2, n <= MAXDIR = 16.
//
//   scan_turn_counts_kernel: scanpaths that exist (humans, samples).  ONE WAVEFRONT PER SCANPATH, four per block, one lane per fixation,
//     read as a cell by scan_lane_cell (scan_common.h: which fixations count and which are dropped -- the code sp_scan_saccade_counts
//     runs, so dropped agrees); pair t counts iff fixations t, t + 1 and t + 2 are all kept.  Lane t takes the cells and kept-flags of
//     lanes t + 1 and t + 2 by shuffles, reads the two sectors and adds 1 to counts[group][k][k'] with an INTEGER atomic add on int64:
//     integers, so the order in which the atomics land cannot change them.  scan_zero_kernel (scan_common.h) zeroes counts first.  A
//     count outside [0, MAXFIX] or a group outside [0, ngroups): pairs -1, dropped 0, none of its rows is read, nothing is counted.
//
//   scan_turn_expect_kernel: the model, in closed form.  The step distributions are not conditioned on sampled fixations, so given the
//     middle fixation b the incoming and the outgoing saccade are independent, and the expected count of (k, k') factorises per middle
//     cell into two fans and an outer product.  ONE 256-THREAD BLOCK PER (row, t), t = 0 .. Tm - 3, Tm = min(T, max_steps) (one block per
//     row when Tm < 3: it only decides bad).  THE ORDER OF EVERY SUM:
//       Z_s, D_s, q_s = the step normalisation of scan_common.h (scan_step_mass, scan_step_norm): the code sp_scan_saccade_expectation
//                runs, so bad rows agree.  Every wave of the block recomputes steps 0 .. t + 2 for itself (the same bits), so nothing
//                is passed between waves and every exit is block-uniform;
//       c_s(i) = (double)p_s[1 + i] / D_s;
//       A_0 = 1, A_{s+1} = A_s * (1.0 - q_s);
//       in_t[b][k]   = sum over the cells a with sector(b - a) = k  of c_t(a),     a in ASCENDING ROW-MAJOR order from 0.0;
//       out_t[b][k'] = sum over the cells a with sector(a - b) = k' of c_{t+2}(a), likewise;
//       X_t[k][k']   = sum over the cells b of (c_{t+1}(b) * in_t[b][k]) * out_t[b][k'] in ASCENDING b from 0.0, each product rounded;
//       work[r][t][k][k'] = A_t * X_t[k][k'];
//       pairs[r] = sum_{t=0}^{Tm-3} A_t * (((1.0 - q_t) * (1.0 - q_{t+1})) * (1.0 - q_{t+2})) in ascending t from 0.0.
//     LDS (dynamic): the three maps c_t, c_{t+1}, c_{t+2} in double, two bin arrays [n + 1][256] in double laid out [k][thread] -- a lane's
//     bank depends on its thread index alone, whatever sector it hits, so lanes that update different k do not conflict -- and the sector
//     table as bytes.  For a batch of 256 middle cells, thread j owns cell b0 + j and walks all source cells a, adding into its own bins;
//     after a barrier thread p (p, p + 256 < E) owns one (k, k') and adds the batch's b in ascending order into an accumulator it keeps
//     across batches, so the b order is ascending overall.
//     A row is BAD iff some step s < Tm is bad (scan_step_norm): the block of t = Tm - 3 walks every step, so it writes bad 1 and pairs
//     NaN; a block that meets the bad step leaves (its slice of work stays unwritten and is never read).  row_group outside [0, ngroups):
//     bad -1, pairs NaN, nothing of the row is read.  Tm < 3: no pair, M and pairs 0 (a bad D_s, s < Tm, still makes the row bad).
//   scan_turn_rows_kernel: one thread per (row, entry): M_r = sum_t work[r][t] in ASCENDING t from 0.0, left in work[r][0].
//   scan_turn_group_kernel: one thread per (group, entry): M[g] = the M_r of the good rows of g in ASCENDING ROW INDEX from 0.0.
// No floating-point atomics; every element of every output is written; all stores are plain vector stores.
#include "common.h"
#include "scan_common.h"

namespace {

constexpr int MAXDIR = 16;        // = sp_scan_turn_max_directions(): 2 * 17 * 256 doubles of bins + three maps + the table stay under 160 KB

// a table value outside [0, n] is read as n
__device__ __forceinline__ int turn_sector(int v, int n) { return (unsigned)v > (unsigned)n ? n : v; }

struct CountArgs {
    const double* fix;
    const int64_t* start;
    const int *count, *group, *sector;
    int ncol, nscan, ngroups, max_steps, Hm, Wm, ndir;
    double frame_w, frame_h;
    unsigned long long* counts;
    int *pairs, *dropped;
};

__global__ __launch_bounds__(256) void scan_turn_counts_kernel(const CountArgs a) {
    int lane;
    int64_t s;
    if (!scan_wave_item(a.nscan, lane, s)) return;
    const int n = a.count[s], g = a.group[s];
    int np = -1, nd = 0;
    if (!scan_count_bad(n) && g >= 0 && g < a.ngroups) {              // wave-uniform
        const ScanLaneCell f = scan_lane_cell(a.fix, a.ncol, a.start, s, n, a.max_steps, lane, a.Hm, a.Wm, a.frame_w, a.frame_h);
        nd = f.dropped;
        const int r1 = __shfl_down(f.row, 1, 64), c1 = __shfl_down(f.col, 1, 64), k1 = __shfl_down((int)f.kept, 1, 64);
        const int r2 = __shfl_down(f.row, 2, 64), c2 = __shfl_down(f.col, 2, 64), k2 = __shfl_down((int)f.kept, 2, 64);
        const bool pair = lane + 2 < f.m && f.kept && k1 != 0 && k2 != 0;   // m <= 64: lanes 62 and 63 never have two successors
        np = __popcll(__ballot(pair));
        if (pair) {
            const int E1 = a.ndir + 1;
            const int k = turn_sector(a.sector[scan_lattice_index(r1 - f.row, c1 - f.col, a.Hm, a.Wm)], a.ndir);
            const int kk = turn_sector(a.sector[scan_lattice_index(r2 - r1, c2 - c1, a.Hm, a.Wm)], a.ndir);
            atomicAdd(a.counts + (int64_t)g * (E1 * E1) + k * E1 + kk, 1ull);
        }
    }
    if (lane == 0) {
        a.pairs[s] = np;
        a.dropped[s] = nd;
    }
}

struct ExpArgs {
    const float* probs;
    const int *row_group, *sector;
    int R, T, Tm, nT, Hm, Wm, ngroups, min_length, ndir;
    double *work, *M, *pairs;
    int* bad;
};

__global__ __launch_bounds__(256) void scan_turn_expect_kernel(const ExpArgs a) {
    extern __shared__ double sh[];                                  // [3][P] maps | [E1][256] in | [E1][256] out | [D] sector bytes
    const int P = a.Hm * a.Wm, LW = 2 * a.Wm - 1, D = (2 * a.Hm - 1) * LW, E1 = a.ndir + 1, E = E1 * E1;
    const int r = (int)(blockIdx.x / (unsigned)a.nT), t = (int)(blockIdx.x % (unsigned)a.nT);
    const int tid = threadIdx.x, lane = tid & 63;
    const bool writer = t == a.nT - 1 && tid == 0;                  // the block of the last t walks every step of the row
    const double nan = __builtin_nan("");
    const int g = a.row_group[r];
    if (g < 0 || g >= a.ngroups) {                                  // block-uniform: nothing of the row is read
        if (writer) {
            a.bad[r] = -1;
            a.pairs[r] = nan;
        }
        return;
    }
    const float* __restrict__ prow = a.probs + (int64_t)r * a.T * (int64_t)(P + 1);
    const int last = min(t + 2, a.Tm - 1);
    double A = 1.0, At = 1.0, Am1 = 1.0, Am2 = 1.0, qm1 = 0.0, qm2 = 0.0, pr = 0.0, Dm[3] = {1.0, 1.0, 1.0};
    for (int s = 0; s <= last; ++s) {                               // A = A_s on entry
        const float* __restrict__ p = prow + (int64_t)s * (P + 1);
        const ScanStep st = scan_step_norm(scan_step_mass(p, P, lane), p, s >= a.min_length);
        if (st.bad) {                                               // the same bits in every wave: a block-uniform exit
            if (writer) {
                a.bad[r] = 1;
                a.pairs[r] = nan;
            }
            return;
        }
        const double Ds = st.D, q = st.q;
        if (s >= 2) pr = pr + Am2 * (((1.0 - qm2) * (1.0 - qm1)) * (1.0 - q));
        if (s == t) At = A;
        if (s == t) Dm[0] = Ds;
        if (s == t + 1) Dm[1] = Ds;
        if (s == t + 2) Dm[2] = Ds;
        Am2 = Am1;
        Am1 = A;
        A = A * (1.0 - q);
        qm2 = qm1;
        qm1 = q;
    }
    if (writer) {
        a.bad[r] = 0;
        a.pairs[r] = a.Tm < 3 ? 0.0 : pr;
    }
    if (a.Tm < 3) return;
    double* __restrict__ cm = sh;                                   // c_t | c_{t+1} | c_{t+2}
    double* __restrict__ bin_in = sh + 3 * P;
    double* __restrict__ bin_out = bin_in + E1 * 256;
    unsigned char* __restrict__ sec = (unsigned char*)(bin_out + E1 * 256);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const float* __restrict__ p = prow + (int64_t)(t + u) * (P + 1);
        for (int i = tid; i < P; i += 256) cm[u * P + i] = (double)p[1 + i] / Dm[u];
    }
    for (int i = tid; i < D; i += 256) sec[i] = (unsigned char)turn_sector(a.sector[i], a.ndir);
    const int p0 = tid, p1 = tid + 256;                             // E <= 289: at most two entries per thread
    const int k0 = p0 / E1, kk0 = p0 % E1, k1 = p1 / E1, kk1 = p1 % E1;
    double acc0 = 0.0, acc1 = 0.0;
    for (int b0 = 0; b0 < P; b0 += 256) {
        __syncthreads();                                            // the maps and the table are in LDS; the last batch's bins are read
        const int b = b0 + tid;
        for (int k = 0; k < E1; ++k) {
            bin_in[k * 256 + tid] = 0.0;
            bin_out[k * 256 + tid] = 0.0;
        }
        if (b < P) {
            // sector(b - a) sits at base - (ra * LW + ca), sector(a - b) at its mirror image D - 1 - that
            int idx = scan_lattice_index(b / a.Wm, b % a.Wm, a.Hm, a.Wm);
            const double* __restrict__ ct = cm;
            const double* __restrict__ ct2 = cm + 2 * P;
            for (int ra = 0; ra < a.Hm; ++ra, idx -= LW) {
                for (int ca = 0; ca < a.Wm; ++ca) {
                    const int ki = sec[idx - ca], ko = sec[D - 1 - idx + ca];
                    double* __restrict__ bi = bin_in + ki * 256 + tid;
                    double* __restrict__ bo = bin_out + ko * 256 + tid;
                    *bi = *bi + ct[ra * a.Wm + ca];
                    *bo = *bo + ct2[ra * a.Wm + ca];
                }
            }
        }
        __syncthreads();                                            // the batch's bins are complete
        const int nb = min(256, P - b0);
        const double* __restrict__ c1 = cm + P + b0;
        if (p0 < E) {
            const double* __restrict__ u = bin_in + k0 * 256;
            const double* __restrict__ v = bin_out + kk0 * 256;
            for (int j = 0; j < nb; ++j) acc0 = acc0 + (c1[j] * u[j]) * v[j];
        }
        if (p1 < E) {
            const double* __restrict__ u = bin_in + k1 * 256;
            const double* __restrict__ v = bin_out + kk1 * 256;
            for (int j = 0; j < nb; ++j) acc1 = acc1 + (c1[j] * u[j]) * v[j];
        }
    }
    double* __restrict__ w = a.work + ((int64_t)r * a.nT + t) * E;
    if (p0 < E) w[p0] = At * acc0;
    if (p1 < E) w[p1] = At * acc1;
}

// M_r[e] = sum_t work[r][t][e] in ascending t from 0.0, left in work[r][0][e]; a bad row's slices are not read
__global__ __launch_bounds__(256) void scan_turn_rows_kernel(const ExpArgs a) {
    const int E = (a.ndir + 1) * (a.ndir + 1);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.R * E) return;
    const int r = (int)(i / E), e = (int)(i % E);
    if (a.bad[r] != 0) return;
    double* __restrict__ w = a.work + (int64_t)r * a.nT * E + e;
    double m = 0.0;
    for (int t = 0; t < a.nT; ++t) m = m + w[(int64_t)t * E];
    w[0] = m;
}

// M[g][e] = the M_r[e] of the good rows of group g, in ascending row index from 0.0; reads bad[] as the expect kernel left it
__global__ __launch_bounds__(256) void scan_turn_group_kernel(const ExpArgs a) {
    const int E = (a.ndir + 1) * (a.ndir + 1);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.ngroups * E) return;
    const int g = (int)(i / E), e = (int)(i % E);
    double m = 0.0;
    if (a.Tm >= 3)
        for (int r = 0; r < a.R; ++r)
            if (a.row_group[r] == g && a.bad[r] == 0) m = m + a.work[(int64_t)r * a.nT * E + e];
    a.M[i] = m;
}

}  // namespace

extern "C" int sp_scan_turn_max_directions(void) { return MAXDIR; }

extern "C" int sp_scan_turn_counts(const double* fix, int ncol, const int64_t* start, const int* count, const int* group, int nscan,
                                   int ngroups, int max_steps, int Hm, int Wm, double frame_w, double frame_h, const int* sector,
                                   int n_directions, int64_t* counts, int* pairs, int* dropped, void* stream) {
    if (!fix || !start || !count || !group || !sector) return SP_ENULL;
    if (!counts || !pairs || !dropped) return SP_ENULL;
    if (ncol < 2 || nscan < 1 || ngroups < 1 || max_steps < 1 || !scan_map_ok(Hm, Wm) || !scan_frame_ok(frame_w, frame_h)) return SP_EINVAL;
    if (n_directions < 1 || n_directions > MAXDIR) return SP_EINVAL;
    const int64_t total = (int64_t)ngroups * (n_directions + 1) * (n_directions + 1);
    if (sp_cdiv(total, 256) > (int64_t)INT32_MAX) return SP_EINVAL;
    const CountArgs a{fix, start, count, group, sector, ncol, nscan, ngroups, max_steps, Hm, Wm, n_directions, frame_w, frame_h,
                      (unsigned long long*)counts, pairs, dropped};
    hipLaunchKernelGGL(scan_zero_kernel<unsigned long long>, dim3((unsigned)sp_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a.counts, total);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_turn_counts_kernel, dim3((unsigned)sp_cdiv(nscan, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_scan_turn_expectation(const float* probs, const int* row_group, int R, int T, int Hm, int Wm, int ngroups,
                                        int min_length, int max_steps, const int* sector, int n_directions, double* work, double* M,
                                        double* pairs, int* bad, void* stream) {
    if (!probs || !row_group || !sector) return SP_ENULL;
    if (!work || !M || !pairs || !bad) return SP_ENULL;
    if (R < 1 || T < 1 || !scan_map_ok(Hm, Wm) || ngroups < 1 || min_length < 0 || max_steps < 1) return SP_EINVAL;
    if (n_directions < 1 || n_directions > MAXDIR) return SP_EINVAL;
    const int Tm = T < max_steps ? T : max_steps, nT = Tm < 3 ? 1 : Tm - 2;
    const int P = Hm * Wm, D = (2 * Hm - 1) * (2 * Wm - 1), E1 = n_directions + 1, E = E1 * E1;
    if ((int64_t)R * nT > (int64_t)INT32_MAX || sp_cdiv((int64_t)R * E, 256) > (int64_t)INT32_MAX ||
        sp_cdiv((int64_t)ngroups * E, 256) > (int64_t)INT32_MAX)
        return SP_EINVAL;
    const ExpArgs a{probs, row_group, sector, R, T, Tm, nT, Hm, Wm, ngroups, min_length, n_directions, work, M, pairs, bad};
    const size_t lds = ((size_t)3 * P + (size_t)2 * E1 * 256) * sizeof(double) + (size_t)D;     // at most 49,152 + 69,632 + 8,001 bytes
    constexpr int max_lds = (3 * MAXCELLS + 2 * (MAXDIR + 1) * 256) * (int)sizeof(double) + 4 * MAXCELLS;
    const int rc = sp_launch_lds<scan_turn_expect_kernel, max_lds>({(int64_t)R * nT}, 256, lds, (hipStream_t)stream, a);
    if (rc != SP_OK) return rc;
    if (Tm >= 3) {
        hipLaunchKernelGGL(scan_turn_rows_kernel, dim3((unsigned)sp_cdiv((int64_t)R * E, 256)), dim3(256), 0, (hipStream_t)stream, a);
        SP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(scan_turn_group_kernel, dim3((unsigned)sp_cdiv((int64_t)ngroups * E, 256)), dim3(256), 0, (hipStream_t)stream, a);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
