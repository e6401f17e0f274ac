// MultiMatch scanpath simplification (Jarodzka et al. 2010, Dewhurst et al. 2012): successive saccades that point the
// same way, and successive short saccades, are merged unless the fixation between them is long, until nothing changes.  Merging
// saccades i and i + 1 DELETES fixation i + 1; the merged saccade is the difference of the two kept neighbours.  The result is an
// ordinary, shorter scanpath in the fixation layout of scanmetrics.hip.  float64, every operation rounded on its own (the arithmetic
// rule of scan_common.h: contraction OFF, plain operators).
//
// With n saccades, l_i = fixation i + 1 - fixation i and rho_i = sqrt(lx_i*lx_i + ly_i*ly_i), for 0 <= i <= n - 2:
//   direction candidate  (lx_i*lx_{i+1} + ly_i*ly_{i+1}) > cos_tdir * (rho_i * rho_{i+1})  and  duration_{i+1} < tdur
//   amplitude candidate  rho_i < tamp  and  duration_{i+1} < tdur
// One pass is greedy, left to right, on the arrays as they are at its start: a candidate i is taken and i + 1 skipped -- within
// every maximal run of candidates the ones at even offset from the run's start.  One round = a direction pass (none when
// cos_tdir >= 1), then an amplitude pass on its result; rounds repeat until one deletes nothing.  The first and the last fixation stay.
//
// One WAVEFRONT per scanpath, four per 256-thread block; no LDS, no per-thread arrays, no atomics, no barriers.  Lane l holds fixation
// l.  The candidates of a pass are one 64-bit ballot; a lane finds the start of its run from the zeros below it (one count of leading
// zeros); the kept fixations are compacted by lane shuffles: lane j pulls from the position of the j-th set bit of the keep mask, so
// lane l again holds fixation l.  The round loop is wave-uniform and bounded by a constant: every round that continues deletes at
// least one of at most 62 inner fixations.
// The kernel guards itself: a wave whose index is >= nscan leaves before reading anything, a count outside 0 .. MAXFIX gives
// count_out 0 and reads no fixation, lane l reads row l only for l < count.
#include "common.h"
#include "scan_common.h"

namespace {

constexpr int MAXROUNDS = 64;     // 62 rounds can delete something, one more finds nothing to do

// position of the j-th (from 0) set bit of mask; 63 at the most when there are fewer (callers do not use that lane)
__device__ __forceinline__ int nth_set_bit(unsigned long long mask, int j) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const int c = __popcll((mask >> pos) & ((1ull << w) - 1ull));
        if (j >= c) {
            pos += w;
            j -= c;
        }
    }
    return pos;
}

// One pass: cand = this lane's saccade is a candidate.  Deletes the chosen fixations, compacts, returns the number deleted (uniform).
__device__ __forceinline__ int simplify_pass(bool cand, int lane, int& cnt, double& x, double& y, double& d) {
    const unsigned long long mask = __ballot(cand);
    if (mask == 0ull) return 0;
    const unsigned long long zeros_below = ~mask & ((1ull << lane) - 1ull);
    const int run_start = zeros_below ? 64 - __clzll((long long)zeros_below) : 0;       // the lane above the nearest zero below
    const unsigned long long take = __ballot(cand && ((lane - run_start) & 1) == 0);
    const unsigned long long live = cnt == 64 ? ~0ull : (1ull << cnt) - 1ull;
    const unsigned long long keep = live & ~(take << 1);                                 // taking saccade i deletes fixation i + 1
    const int src = nth_set_bit(keep, lane);
    x = __shfl(x, src, 64);
    y = __shfl(y, src, 64);
    d = __shfl(d, src, 64);
    const int kept = __popcll(keep);
    const int gone = cnt - kept;
    cnt = kept;
    return gone;
}

__global__ __launch_bounds__(256) void scan_simplify_kernel(const double* __restrict__ fix, int ncol, const int64_t* __restrict__ start,
                                                            const int* __restrict__ count, int nscan, double cos_tdir, double tdur,
                                                            double tamp, double* __restrict__ fix_out, int* __restrict__ count_out) {
    int lane;
    int64_t s;
    if (!scan_wave_item(nscan, lane, s)) return;
    int cnt = count[s];
    if (scan_count_bad(cnt)) {                                 // beyond the kernel limit: no fixation is read
        if (lane == 0) count_out[s] = 0;
        return;
    }
    const int64_t base = start[s];
    double x = 0.0, y = 0.0, d = 0.0;
    if (lane < cnt) {
        const double* f = fix + (base + lane) * ncol;
        x = f[0];
        y = f[1];
        d = f[2];
    }
    const bool use_dir = cos_tdir < 1.0;
    for (int round = 0; round < MAXROUNDS; ++round) {          // wave-uniform: cnt and the masks are the same in every lane
        int gone = 0;
        if (use_dir && cnt >= 3) {
            const double lx = __shfl_down(x, 1, 64) - x, ly = __shfl_down(y, 1, 64) - y;
            const double rho = scan_dist(lx, ly);
            const double nx = __shfl_down(lx, 1, 64), ny = __shfl_down(ly, 1, 64), nrho = __shfl_down(rho, 1, 64);
            const double nd = __shfl_down(d, 1, 64);           // the duration of fixation lane + 1
            const bool cand = lane <= cnt - 3 && (lx * nx + ly * ny) > cos_tdir * (rho * nrho) && nd < tdur;
            gone += simplify_pass(cand, lane, cnt, x, y, d);
        }
        if (cnt >= 3) {
            const double lx = __shfl_down(x, 1, 64) - x, ly = __shfl_down(y, 1, 64) - y;
            const double rho = scan_dist(lx, ly);
            const double nd = __shfl_down(d, 1, 64);
            const bool cand = lane <= cnt - 3 && rho < tamp && nd < tdur;
            gone += simplify_pass(cand, lane, cnt, x, y, d);
        }
        if (gone == 0) break;
    }
    if (lane < cnt) {
        double* o = fix_out + (base + lane) * 3;
        o[0] = x;
        o[1] = y;
        o[2] = d;
    }
    if (lane == 0) count_out[s] = cnt;
}

}  // namespace

// Simplified copies of nscan scanpaths: fix [total][ncol >= 3] = (x, y, duration, ...), scanpath k = rows start[k] .. +count[k];
// fix_out [total][3] at the same starts, count_out[k] <= count[k] rows of it written
extern "C" int sp_scan_simplify(const double* fix, int ncol, const int64_t* start, const int* count, int nscan, double cos_tdir,
                                double tdur, double tamp, double* fix_out, int* count_out, void* stream) {
    if (!fix || !start || !count || !fix_out || !count_out) return SP_ENULL;
    if (nscan < 1 || ncol < 3 || !(tdur >= 0.0) || !(tdur < INFINITY) || !(tamp >= 0.0) || !(tamp < INFINITY) ||
        !(cos_tdir >= -1.0) || !(cos_tdir <= 1.0))
        return SP_EINVAL;
    hipLaunchKernelGGL(scan_simplify_kernel, dim3((unsigned)sp_cdiv(nscan, 4)), dim3(256), 0, (hipStream_t)stream, fix, ncol, start,
                       count, nscan, cos_tdir, tdur, tamp, fix_out, count_out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
