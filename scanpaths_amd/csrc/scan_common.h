// What the scanpath scorer kernels share (scanmetrics.hip, scandist.hip, seqscore.hip, scansimplify.hip, scanlik.hip, scankde.hip,
// scansearch.hip, scansaccade.hip, scanturn.hip, scanboot.hip and, in the stats and the model library, scanrecur.hip and scanexpect.hip) -- the device-side counterpart of
// utils/evaltools/_batch.py and _args.py: the fixation and the cell limit, the float64 arithmetic rule, the pixel rule that turns a
// fixation into a map cell, the prologue of a kernel that scores scanpaths or pairs of them in the layout rows [total][ncol] | start
// int64 [K] | count int32 [K] | pairs int32 [P][2], with the guard against a count the kernel cannot hold, the two wave reductions,
// and what the kernels on the displacement lattice and on the model's step distributions share (the last section).  Everything is a
// template or __forceinline__ / static inline: a file that does not use a piece emits nothing for it.  Include it after common.h.
//
// THE ARITHMETIC RULE: float64, every operation rounded on its own, in the order written -- numpy's and plain Python's arithmetic, so
// the checkers compare bit for bit.  The pragma below turns floating-point contraction OFF for the rest of the including file, and the
// kernels use the plain operators.  __dmul_rn / __dadd_rn do not give that here: the compiler's header defines them as `x * y` / `x + y`
// compiled under the default -ffp-contract=fast, so after inlining dx*dx + dy*dy becomes one v_fma_f64 -- which changes the last bit as
// soon as dx*dx is not exact (it is on integer pixel grids, which is why only off-grid data shows it).
#pragma once

#pragma clang fp contract(off)

constexpr int MAXFIX = 64;        // = sp_scan_max_fixations() = _batch.MAX_FIXATIONS: one lane, or one slot of a per-thread array, per fixation
constexpr int MAXCELLS = 2048;    // = sp_scan_likelihood_max_cells() = _args.MAX_CELLS: a step map is 32 floats per lane, two in double 32 KB of LDS

// a count the kernels cannot hold: such a scanpath reads none of its rows and gives NaN (-1 where the output is an integer)
__device__ __forceinline__ bool scan_count_bad(int n) { return n < 0 || n > MAXFIX; }

// the length of (dx, dy): three roundings and the correctly rounded root
__device__ __forceinline__ double scan_dist(double dx, double dy) { return __builtin_sqrt(dx * dx + dy * dy); }

// THE PIXEL RULE (sp_fixation_maps, sp_scan_likelihood, sp_scan_saccade_counts): a fixation counts iff both coordinates are finite and
// inside the half-open frame; its cell along an axis of n cells over `frame` pixels is floor(v * n / frame), in double
__device__ __forceinline__ bool scan_in_frame(double x, double y, double frame_w, double frame_h) {
    return isfinite(x) && isfinite(y) && x >= 0.0 && x < frame_w && y >= 0.0 && y < frame_h;
}
__device__ __forceinline__ int scan_cell(double v, int n, double frame) { return min((int)floor((v * (double)n) / frame), n - 1); }

// pair p of a launch: the two scanpath indices, their counts and their first rows (rows of ncol values of T; not to be read when bad())
template <typename T>
struct ScanPair {
    int ia, ib, na, nb;
    const T *ra, *rb;
    __device__ __forceinline__ bool bad() const { return scan_count_bad(na) || scan_count_bad(nb); }
};
template <typename T>
__device__ __forceinline__ ScanPair<T> scan_pair(const int* __restrict__ pairs, const int* __restrict__ count,
                                                 const int64_t* __restrict__ start, const T* __restrict__ rows, int ncol, int64_t p) {
    const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
    return {ia, ib, count[ia], count[ib], rows + start[ia] * ncol, rows + start[ib] * ncol};
}

// one wavefront per item, four per 256-thread block: the lane and the wave's item; false for a wave without one (it leaves whole)
__device__ __forceinline__ bool scan_wave_item(int64_t nitems, int& lane, int64_t& item) {
    lane = threadIdx.x & 63;
    item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    return item < nitems;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {      // b > a ? b : a, not fmax: the operands are never NaN and the choice is ours
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// ---- the displacement lattice and the model's step distributions (scansaccade.hip, scanturn.hip, scansearch.hip, scanrecur.hip, scanexpect.hip) -------------------------
// launcher checks: a frame of positive finite sizes; a map of Hm x Wm >= 1 x 1 and at most MAXCELLS cells
static inline bool scan_frame_ok(double frame_w, double frame_h) {
    return frame_w > 0 && frame_w < INFINITY && frame_h > 0 && frame_h < INFINITY;
}
static inline bool scan_map_ok(int Hm, int Wm) { return Hm >= 1 && Wm >= 1 && (int64_t)Hm * Wm <= MAXCELLS; }

// zeroes n 64-bit counters in stream order before a kernel that adds into them with integer atomics (a kernel, not a memset:
// common.h).  A template only so that a file which does not launch it emits nothing; unsigned long long is the one instance.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void scan_zero_kernel(T* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = T(0);
}
}  // namespace

// THE LANE'S FIXATION AS A CELL: one wavefront per scanpath, lane t holds fixation t.  Only the first m = min(n, max_steps) fixations
// count; a fixation that is not scan_in_frame is dropped -- kept false, cell (0, 0), counted in dropped (wave-uniform: every lane of
// the wave must call) -- and nothing bridges a dropped fixation: a saccade, or a pair of them, counts iff all of its fixations are kept.
struct ScanLaneCell {
    int m, row, col, dropped;
    bool kept;
};
__device__ __forceinline__ ScanLaneCell scan_lane_cell(const double* __restrict__ fix, int ncol, const int64_t* __restrict__ start,
                                                       int64_t s, int n, int max_steps, int lane, int Hm, int Wm, double frame_w,
                                                       double frame_h) {
    const int m = min(n, max_steps);
    bool kept = false;
    int row = 0, col = 0;
    if (lane < m) {
        const double* __restrict__ f = fix + (start[s] + lane) * ncol;
        const double x = f[0], y = f[1];
        kept = scan_in_frame(x, y, frame_w, frame_h);
        if (kept) {
            col = scan_cell(x, Wm, frame_w);
            row = scan_cell(y, Hm, frame_h);
        }
    }
    return {m, row, col, (int)__popcll(__ballot(lane < m && !kept)), kept};
}

// the entry of the displacement (dr, dc) on the (2 Hm - 1) x (2 Wm - 1) lattice
__device__ __forceinline__ int scan_lattice_index(int dr, int dc, int Hm, int Wm) { return (dr + Hm - 1) * (2 * Wm - 1) + (dc + Wm - 1); }

// THE STEP NORMALISATION of a row p = (p_0 = terminate, P cells) of the model's step distributions, in two pieces.
// Z: lane l adds cells l, l + 64, l + 128, .. in that order from 0.0 and the 64 partial sums combine by the xor butterfly 32 .. 1
// (wave_sum_d): a function of P alone, the same bits in every wave that computes it.
__device__ __forceinline__ double scan_step_mass(const float* __restrict__ p, int P, int lane) {
    double z = 0.0;
    for (int c = lane; c < P; c += 64) z = z + (double)p[1 + c];
    return wave_sum_d(z);
}
// (Z, p_0, stop = t >= min_length: terminate is unmasked) -> D = Z + p_0 when stop, else Z; q = p_0 / D when stop, else 0; the step is
// bad iff D is zero or not finite (q is then meaningless).  c(i) = (double)p[1 + i] / D is the caller's.
struct ScanStep {
    double D, q;
    bool bad;
};
__device__ __forceinline__ ScanStep scan_step_norm(double Z, const float* __restrict__ p, bool stop) {
    const double p0 = stop ? (double)p[0] : 0.0;
    const double D = stop ? Z + p0 : Z;
    return {D, stop ? p0 / D : 0.0, D == 0.0 || !isfinite(D)};
}
