// What the scanpath scorer kernels share (scanmetrics.hip, scandist.hip, seqscore.hip, scansimplify.hip, scanlik.hip, scansaccade.hip,
// scanturn.hip, scanboot.hip) -- the device-side counterpart of utils/evaltools/_batch.py: the fixation limit, the float64 arithmetic rule, the
// pixel rule that turns a fixation into a map cell, the prologue of a kernel
// that scores scanpaths or pairs of them in the layout rows [total][ncol] | start int64 [K] | count int32 [K] | pairs int32 [P][2],
// with the guard against a count the kernel cannot hold, and the two wave reductions.  Include it after common.h.
//
// THE ARITHMETIC RULE: float64, every operation rounded on its own, in the order written -- numpy's and plain Python's arithmetic, so
// the checkers compare bit for bit.  The pragma below turns floating-point contraction OFF for the rest of the including file, and the
// kernels use the plain operators.  __dmul_rn / __dadd_rn do not give that here: the compiler's header defines them as `x * y` / `x + y`
// compiled under the default -ffp-contract=fast, so after inlining dx*dx + dy*dy becomes one v_fma_f64 -- which changes the last bit as
// soon as dx*dx is not exact (it is on integer pixel grids, which is why only off-grid data shows it).
#pragma once

#pragma clang fp contract(off)

constexpr int MAXFIX = 64;        // = sp_scan_max_fixations() = _batch.MAX_FIXATIONS: one lane, or one slot of a per-thread array, per fixation

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
