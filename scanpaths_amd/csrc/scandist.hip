// Scanpath distances the reference's copy of the VAME toolbox does not carry: dynamic time warping, the discrete
// Frechet distance (Eiter & Mannila 1994), the Hausdorff distance, Eyenalysis (Mathot et al. 2012, position only) and the four
// cross-recurrence measures REC / DET / LAM / CORM (Anderson et al. 2015), of npairs scanpath pairs in the fixation layout of
// scanmetrics.hip.  P is the first scanpath of a pair, Q the second; coordinates are divided by max_dim first;
// d(i,j) = sqrt(dx*dx + dy*dy) with every operation rounded on its own (scan_dist and the arithmetic rule of scan_common.h).
//
// One WAVEFRONT per pair, four pairs per 256-thread block; no LDS, no per-thread arrays, no atomics.  Lane j owns Q_j (and, for the
// row minima, P_j).
//   DTW / Frechet: anti-diagonal sweep, step k handles the cells i + j = k, lane j the cell (k - j, j).  Up = the lane's own value of
//     step k - 1, left = lane j - 1's value of step k - 1 (one lane shuffle per measure), diagonal = the left value the lane received
//     at step k - 1.  n + m - 1 steps.  Every cell's arithmetic is the recursion's, so the schedule does not change a bit.
//   Hausdorff / Eyenalysis: min_i d(i,j) stays in lane j while the P_i are broadcast one after the other, min_j d(i,j) stays in lane i
//     while the Q_j are broadcast (d is the same number either way round: the two differences only change sign).  The two Eyenalysis
//     sums are added serially in index order.
//   Cross-recurrence: row i of the N x N matrix is one 64-bit ballot.  R is its popcount, points on row runs >= L come from shifts of
//     the mask, column runs from a per-lane run counter, diagonal runs from a run counter that moves one lane up per row.
// The kernels guard themselves: a pair with a scanpath of more than MAXFIX (or fewer than 0) fixations gets NaN in every output and
// none of its fixations is read.
#include "common.h"
#include "scan_common.h"

namespace {

__device__ __forceinline__ double sd_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double sd_max(double a, double b) { return b > a ? b : a; }

__global__ __launch_bounds__(256) void scan_distances_kernel(const double* __restrict__ fix, int ncol, const int64_t* __restrict__ start,
                                                             const int* __restrict__ count, const int* __restrict__ pairs, int npairs,
                                                             double max_dim, double* __restrict__ dtw, double* __restrict__ frechet,
                                                             double* __restrict__ hausdorff, double* __restrict__ eyenalysis) {
    int lane;
    int64_t p;
    if (!scan_wave_item(npairs, lane, p)) return;
    const ScanPair<double> q = scan_pair(pairs, count, start, fix, ncol, p);
    const int n = q.na, m = q.nb;
    if (q.bad() || n < 1 || m < 1) {                           // beyond the kernel limit, or empty: NaN, no fixation is read
        if (lane == 0) {
            if (dtw) dtw[p] = NAN;
            if (frechet) frechet[p] = NAN;
            if (hausdorff) hausdorff[p] = NAN;
            if (eyenalysis) eyenalysis[p] = NAN;
        }
        return;
    }
    const double *fp = q.ra, *fq = q.rb;
    double px = 0.0, py = 0.0, qx = 0.0, qy = 0.0;             // P_lane, Q_lane
    if (lane < n) { px = fp[(int64_t)lane * ncol] / max_dim; py = fp[(int64_t)lane * ncol + 1] / max_dim; }
    if (lane < m) { qx = fq[(int64_t)lane * ncol] / max_dim; qy = fq[(int64_t)lane * ncol + 1] / max_dim; }

    if (dtw || frechet) {
        double dv = INFINITY, dleft = INFINITY;                // DTW: the lane's last cell, the left neighbour it last received
        double fv = INFINITY, fleft = INFINITY;                // Frechet likewise
        for (int k = 0; k < n + m - 1; ++k) {
            const int i = k - lane;
            const bool live = lane < m && i >= 0 && i < n;
            const int src = live ? i : 0;
            const double d = scan_dist(__shfl(px, src, 64) - qx, __shfl(py, src, 64) - qy);
            const double dl = __shfl_up(dv, 1, 64), fl = __shfl_up(fv, 1, 64);
            if (live) {
                const bool top = i == 0, first = lane == 0;
                if (dtw) {
                    const double best = (top && first) ? 0.0
                                                       : sd_min(sd_min((top || first) ? INFINITY : dleft, top ? INFINITY : dv),
                                                                first ? INFINITY : dl);
                    dv = best + d;
                    dleft = dl;
                }
                if (frechet) {
                    const double best = (top && first) ? 0.0
                                                       : sd_min(sd_min((top || first) ? INFINITY : fleft, top ? INFINITY : fv),
                                                                first ? INFINITY : fl);
                    fv = sd_max(best, d);
                    fleft = fl;
                }
            }
        }
        if (lane == m - 1) {                                   // its last cell is (n - 1, m - 1)
            if (dtw) dtw[p] = dv;
            if (frechet) frechet[p] = fv;
        }
    }

    if (hausdorff || eyenalysis) {
        double colmin = INFINITY, rowmin = INFINITY;           // min_i d(i, lane), min_j d(lane, j)
        for (int i = 0; i < n; ++i) colmin = sd_min(colmin, scan_dist(__shfl(px, i, 64) - qx, __shfl(py, i, 64) - qy));
        for (int j = 0; j < m; ++j) rowmin = sd_min(rowmin, scan_dist(px - __shfl(qx, j, 64), py - __shfl(qy, j, 64)));
        if (hausdorff) {
            const double h = wave_max_d(sd_max(lane < n ? rowmin : 0.0, lane < m ? colmin : 0.0));     // d >= 0
            if (lane == 0) hausdorff[p] = h;
        }
        if (eyenalysis) {
            double s = 0.0;
            for (int i = 0; i < n; ++i) s = s + __shfl(rowmin, i, 64);
            for (int j = 0; j < m; ++j) s = s + __shfl(colmin, j, 64);
            if (lane == 0) eyenalysis[p] = s / (double)max(n, m);
        }
    }
}

// points of a 64-bit row mask that lie on runs of at least L consecutive set bits
__device__ __forceinline__ int run_points(unsigned long long mask, int L) {
    if (L > MAXFIX) return 0;
    unsigned long long s = mask;                               // bit b: a window of L set bits starts at b
    for (int k = 1; k < L; ++k) s &= mask >> k;
    unsigned long long t = s;
    for (int k = 1; k < L; ++k) t |= s << k;
    return __popcll(t);
}

__global__ __launch_bounds__(256) void scan_recurrence_kernel(const double* __restrict__ fix, int ncol, const int64_t* __restrict__ start,
                                                              const int* __restrict__ count, const int* __restrict__ pairs, int npairs,
                                                              double max_dim, double radius, int L, double* __restrict__ out) {
    int lane;
    int64_t p;
    if (!scan_wave_item(npairs, lane, p)) return;
    const ScanPair<double> q = scan_pair(pairs, count, start, fix, ncol, p);
    const int N = min(q.na, q.nb);
    double* o = out + 4 * p;
    if (q.bad() || N < 1) {
        if (lane < 4) o[lane] = NAN;
        return;
    }
    const double *fp = q.ra, *fq = q.rb;
    double px = 0.0, py = 0.0, qx = 0.0, qy = 0.0;
    if (lane < N) {
        px = fp[(int64_t)lane * ncol] / max_dim; py = fp[(int64_t)lane * ncol + 1] / max_dim;
        qx = fq[(int64_t)lane * ncol] / max_dim; qy = fq[(int64_t)lane * ncol + 1] / max_dim;
    }
    int R = 0, HL = 0;                                         // wave-uniform
    int vrun = 0, VL = 0, drun = 0, DL = 0, corm = 0;          // per lane (column lane; the diagonal through (i, lane))
    for (int i = 0; i < N; ++i) {
        const bool c = lane < N && scan_dist(__shfl(px, i, 64) - qx, __shfl(py, i, 64) - qy) <= radius;
        const unsigned long long mask = __ballot(c);
        R += __popcll(mask);
        HL += run_points(mask, L);
        int r = __shfl_up(drun, 1, 64);                        // the run that reached (i - 1, lane - 1)
        if (lane == 0) r = 0;
        if (c) {
            ++vrun;
            drun = r + 1;
            corm += lane - i;
            if (lane == N - 1 && drun >= L) DL += drun;        // the diagonal leaves the matrix on the right
        } else {
            if (vrun >= L) VL += vrun;
            vrun = 0;
            if (lane < N && r >= L) DL += r;
            drun = 0;
        }
    }
    if (vrun >= L) VL += vrun;                                 // runs that reach the last row
    if (lane < N - 1 && drun >= L) DL += drun;
    VL = wave_sum_i(VL);
    DL = wave_sum_i(DL);
    corm = wave_sum_i(corm);
    if (lane == 0) {
        o[0] = 100.0 * (double)R / (double)(N * N);
        o[1] = R == 0 ? NAN : 100.0 * (double)DL / (double)R;
        o[2] = R == 0 ? NAN : 100.0 * (double)(HL + VL) / (double)(2 * R);
        o[3] = (R == 0 || N == 1) ? NAN : 100.0 * (double)corm / (double)((N - 1) * R);
    }
}

}  // namespace

extern "C" int sp_scan_distances(const double* fix, int ncol, const int64_t* start, const int* count, const int* pairs, int npairs,
                                 double max_dim, double* dtw, double* frechet, double* hausdorff, double* eyenalysis, void* stream) {
    if (!fix || !start || !count || !pairs || (!dtw && !frechet && !hausdorff && !eyenalysis)) return SP_ENULL;
    if (npairs < 1 || ncol < 2 || !(max_dim > 0)) return SP_EINVAL;
    hipLaunchKernelGGL(scan_distances_kernel, dim3((unsigned)sp_cdiv(npairs, 4)), dim3(256), 0, (hipStream_t)stream, fix, ncol, start,
                       count, pairs, npairs, max_dim, dtw, frechet, hausdorff, eyenalysis);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_scan_recurrence(const double* fix, int ncol, const int64_t* start, const int* count, const int* pairs, int npairs,
                                  double max_dim, double radius, int min_line, double* out, void* stream) {
    if (!fix || !start || !count || !pairs || !out) return SP_ENULL;
    if (npairs < 1 || ncol < 2 || !(max_dim > 0) || !(radius > 0) || min_line < 2) return SP_EINVAL;
    hipLaunchKernelGGL(scan_recurrence_kernel, dim3((unsigned)sp_cdiv(npairs, 4)), dim3(256), 0, (hipStream_t)stream, fix, ncol, start,
                       count, pairs, npairs, max_dim, radius, min_line, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
