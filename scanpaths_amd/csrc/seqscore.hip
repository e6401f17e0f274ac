// Sequence score (Yang et al. 2020) and fixation edit distance (Mondal et al. 2023) on mean-shift clusters: flat-kernel
// mean shift (Comaniciu & Meer 2002) of groups of fixations, the cluster-label strings of scanpaths under a group's centres, and the
// Needleman-Wunsch score / Levenshtein distance of pairs of such strings.  Everything is float64 and follows the definitions of §17
// operation by operation (the arithmetic rule of scan_common.h: contraction OFF, plain operators), and every sum runs left to right in
// index order.
//
//   meanshift_kernel: one 256-thread block per group.  x and y are staged once into LDS; ONE THREAD PER SEED (seeds tid, tid + 256, ..)
//     walks the points serially, which is the definition's index-order sum; all lanes read the same LDS address in the same step
//     (a broadcast), and lanes differ only in how many iterations their seed needs.  The seeds' results (k, centre) go to LDS, each
//     entry counts the entries that precede it in the order (k desc, x desc, y desc, seed asc) and writes its index at that rank; the
//     suppression is a serial walk over the ranks with the block spread over the later entries; the labels of the group's own points
//     come from the kept centres in the same launch.  No atomics, no per-thread arrays.
//   cluster_strings_kernel: one wavefront per scanpath, one lane per fixation, a loop over the group's centres.
//   sequence_kernel: one wavefront per pair, four pairs per block, the anti-diagonal sweep of scan_distances_kernel: lane l owns b[l]
//     and column l + 1 of both tables, step s handles the cells i + l = s; up = the lane's own value of step s - 1, left = lane l - 1's
//     value of step s - 1 (one lane shuffle per table), diagonal = the left value received at step s - 1.  n + m - 1 steps; every
//     cell's arithmetic is the recursion's own, so the schedule does not change a bit.
// The kernels guard themselves: a group of more than MAXPTS (or fewer than 0) points gets ncentres -1 and labels -1 and none of its
// points is read; a scanpath of more than MAXFIX (or fewer than 0) fixations gets no labels and NaN for its pairs.
#include "common.h"
#include "scan_common.h"

namespace {

constexpr int MAXPTS = 1024;      // = sp_meanshift_max_points(): x, y (16 KB) + the seeds' results (20 KB) + order and kept lists (8 KB) + flags

__device__ __forceinline__ double sq_max(double a, double b) { return b > a ? b : a; }

// does entry (ka, ax, ay, a) come before entry (kb, bx, by, b) in the order: k descending, x descending, y descending, seed ascending
__device__ __forceinline__ bool ms_before(int ka, double ax, double ay, int a, int kb, double bx, double by, int b) {
    if (ka != kb) return ka > kb;
    if (ax != bx) return ax > bx;
    if (ay != by) return ay > by;
    return a < b;
}

__global__ __launch_bounds__(256) void meanshift_kernel(const double* __restrict__ pts, int ncol, const int64_t* __restrict__ gstart,
                                                        const int* __restrict__ gcount, double bandwidth, int max_iter,
                                                        double* __restrict__ centres, int* __restrict__ ncentres, int* __restrict__ weight,
                                                        int* __restrict__ labels) {
    __shared__ double xs[MAXPTS], ys[MAXPTS];          // the group's points
    __shared__ double ecx[MAXPTS], ecy[MAXPTS];        // seed s ends at (ecx[s], ecy[s]) ..
    __shared__ int ek[MAXPTS];                         // .. with ek[s] points around the centre before it (0: the seed yields nothing)
    __shared__ int order[MAXPTS];                      // order[r] = the seed at rank r
    __shared__ int kept[MAXPTS];                       // kept[c] = the seed whose centre is cluster c
    __shared__ unsigned char gone[MAXPTS];             // suppressed by a kept entry before it
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n = gcount[g];
    const int64_t row0 = gstart[g];
    if (n < 0 || n > MAXPTS) {                         // beyond the kernel limit: nothing is read
        if (tid == 0) ncentres[g] = -1;
        if (labels)
            for (int i = tid; i < n; i += 256) labels[row0 + i] = -1;
        return;
    }
    for (int i = tid; i < n; i += 256) {
        xs[i] = pts[(row0 + i) * ncol];
        ys[i] = pts[(row0 + i) * ncol + 1];
        order[i] = 0;
        gone[i] = 0;
    }
    __syncthreads();
    const double h2 = bandwidth * bandwidth, stop = 1e-3 * bandwidth;
    for (int s = tid; s < n; s += 256) {
        double cx = xs[s], cy = ys[s];
        int k = 0;
        for (int it = 0;; ++it) {
            double sx = 0.0, sy = 0.0;
            k = 0;
            for (int i = 0; i < n; ++i) {
                const double x = xs[i], y = ys[i];
                const double dx = x - cx, dy = y - cy;
                if (dx * dx + dy * dy <= h2) {
                    sx = sx + x;
                    sy = sy + y;
                    ++k;
                }
            }
            if (k == 0) break;
            const double nx = sx / (double)k, ny = sy / (double)k;
            const double dx = nx - cx, dy = ny - cy;
            cx = nx;
            cy = ny;
            if (scan_dist(dx, dy) <= stop || it == max_iter) break;
        }
        ek[s] = k;
        ecx[s] = k ? cx : 0.0;                         // an entry without a result sorts last and ends the walk below
        ecy[s] = k ? cy : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < n; e += 256) {               // rank counting: the order is total, so the ranks are 0 .. n - 1, each once
        const int k = ek[e];
        const double cx = ecx[e], cy = ecy[e];
        int r = 0;
        for (int j = 0; j < n; ++j) r += ms_before(ek[j], ecx[j], ecy[j], j, k, cx, cy, e) ? 1 : 0;
        order[r] = e;
    }
    __syncthreads();
    int K = 0;                                         // block-uniform
    for (int r = 0; r < n; ++r) {
        const int e = order[r];
        if (ek[e] == 0) break;                         // this and every later entry yielded nothing
        if (gone[e]) continue;                         // written before the last barrier, or never
        const double cx = ecx[e], cy = ecy[e];
        if (tid == 0) {
            kept[K] = e;
            centres[(row0 + K) * 2] = cx;
            centres[(row0 + K) * 2 + 1] = cy;
            if (weight) weight[row0 + K] = ek[e];
        }
        ++K;
        for (int q = r + 1 + tid; q < n; q += 256) {
            const int f = order[q];
            const double dx = ecx[f] - cx, dy = ecy[f] - cy;
            if (dx * dx + dy * dy <= h2) gone[f] = 1;
        }
        __syncthreads();                               // gone[] and kept[K - 1] are visible to every later step
    }
    if (tid == 0) ncentres[g] = K;
    if (!labels) return;
    for (int i = tid; i < n; i += 256) {
        int lab = -1;
        if (K > 0) {
            const double x = xs[i], y = ys[i];
            double dx = x - ecx[kept[0]], dy = y - ecy[kept[0]];
            double best = dx * dx + dy * dy;
            lab = 0;
            for (int c = 1; c < K; ++c) {
                dx = x - ecx[kept[c]];
                dy = y - ecy[kept[c]];
                const double d = dx * dx + dy * dy;
                if (d < best) { best = d; lab = c; }
            }
        }
        labels[row0 + i] = lab;
    }
}

__global__ __launch_bounds__(256) void cluster_strings_kernel(const double* __restrict__ fix, int ncol, const int64_t* __restrict__ start,
                                                              const int* __restrict__ count, const int* __restrict__ group, int nscan,
                                                              const double* __restrict__ centres, const int64_t* __restrict__ gstart,
                                                              const int* __restrict__ ncentres, int* __restrict__ labels_out) {
    int lane;
    int64_t s;
    if (!scan_wave_item(nscan, lane, s)) return;
    const int n = count[s];
    if (scan_count_bad(n) || lane >= n) return;        // beyond the limit: nothing is read or written (its pairs score NaN)
    const int64_t row = start[s] + lane;
    const int g = group[s];
    const int K = ncentres[g];
    int lab = -1;
    if (K > 0) {
        const double* c = centres + gstart[g] * 2;
        const double x = fix[row * ncol], y = fix[row * ncol + 1];
        double dx = x - c[0], dy = y - c[1];
        double best = dx * dx + dy * dy;
        lab = 0;
        for (int k = 1; k < K; ++k) {
            dx = x - c[2 * k];
            dy = y - c[2 * k + 1];
            const double d = dx * dx + dy * dy;
            if (d < best) { best = d; lab = k; }
        }
    }
    labels_out[row] = lab;
}

__global__ __launch_bounds__(256) void sequence_kernel(const int* __restrict__ labels, const int64_t* __restrict__ start,
                                                       const int* __restrict__ count, const int* __restrict__ pairs, int npairs, double gap,
                                                       double* __restrict__ ss, double* __restrict__ fed) {
    int lane;
    int64_t p;
    if (!scan_wave_item(npairs, lane, p)) return;
    const ScanPair<int> q = scan_pair(pairs, count, start, labels, 1, p);      // rows of one label
    const int n = q.na, m = q.nb;
    bool bad = q.bad();                                        // beyond the kernel limit: NaN, no label is read
    int a = 0, b = 0;                                          // a[lane], b[lane]
    if (!bad) {
        if (lane < n) a = q.ra[lane];
        if (lane < m) b = q.rb[lane];
        bad = __ballot(a < 0 || b < 0) != 0ull;                // a fixation without a cluster
    }
    if (bad) {
        if (lane == 0) {
            if (ss) ss[p] = NAN;
            if (fed) fed[p] = NAN;
        }
        return;
    }
    // lane l owns column l + 1 of F (Needleman-Wunsch) and D (Levenshtein); row 0 and column 0 are the borders gap * i and i
    double fv = 0.0, fleft = 0.0;                              // the lane's last cell, the left neighbour it last received
    int dv = 0, dleft = 0;
    for (int s = 0; s < n + m - 1; ++s) {
        const int i = s - lane;                                // the cell is (i + 1, lane + 1)
        const bool live = lane < m && i >= 0 && i < n;
        const int ai = __shfl(a, live ? i : 0, 64);
        const double fl = __shfl_up(fv, 1, 64);
        const int dl = __shfl_up(dv, 1, 64);
        if (live) {
            const bool top = i == 0, first = lane == 0;
            const double fdiag = top ? gap * (double)lane : (first ? gap * (double)i : fleft);
            const double fup = top ? gap * (double)(lane + 1) : fv;
            const double flft = first ? gap * (double)(i + 1) : fl;
            fv = sq_max(sq_max(fdiag + (ai == b ? 1.0 : 0.0), fup + gap), flft + gap);
            fleft = fl;
            const int ddiag = top ? lane : (first ? i : dleft);
            const int dup = top ? lane + 1 : dv;
            const int dlft = first ? i + 1 : dl;
            dv = min(min(ddiag + (ai == b ? 0 : 1), dup + 1), dlft + 1);
            dleft = dl;
        }
    }
    const int longer = max(n, m);
    if (n == 0 || m == 0) {                                    // the border itself
        if (lane == 0) {
            if (ss) ss[p] = longer == 0 ? NAN : gap * (double)longer / (double)longer;
            if (fed) fed[p] = (double)longer;
        }
    } else if (lane == m - 1) {                                // its last cell is (n, m)
        if (ss) ss[p] = fv / (double)longer;
        if (fed) fed[p] = (double)dv;
    }
}

}  // namespace

extern "C" int sp_meanshift_max_points(void) { return MAXPTS; }

extern "C" int sp_meanshift(const double* pts, int ncol, const int64_t* gstart, const int* gcount, int ngroups, double bandwidth,
                            int max_iter, double* centres, int* ncentres, int* weight, int* labels, void* stream) {
    if (!pts || !gstart || !gcount || !centres || !ncentres) return SP_ENULL;
    if (ngroups < 1 || ncol < 2 || !(bandwidth > 0) || !(bandwidth < INFINITY) || max_iter < 1) return SP_EINVAL;
    hipLaunchKernelGGL(meanshift_kernel, dim3((unsigned)ngroups), dim3(256), 0, (hipStream_t)stream, pts, ncol, gstart, gcount, bandwidth,
                       max_iter, centres, ncentres, weight, labels);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_scan_cluster_strings(const double* fix, int ncol, const int64_t* start, const int* count, const int* group, int nscan,
                                       const double* centres, const int64_t* gstart, const int* ncentres, int* labels_out, void* stream) {
    if (!fix || !start || !count || !group || !centres || !gstart || !ncentres || !labels_out) return SP_ENULL;
    if (nscan < 1 || ncol < 2) return SP_EINVAL;
    hipLaunchKernelGGL(cluster_strings_kernel, dim3((unsigned)sp_cdiv(nscan, 4)), dim3(256), 0, (hipStream_t)stream, fix, ncol, start,
                       count, group, nscan, centres, gstart, ncentres, labels_out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_scan_sequence(const int* labels, const int64_t* start, const int* count, const int* pairs, int npairs, double gap,
                                double* ss, double* fed, void* stream) {
    if (!labels || !start || !count || !pairs || (!ss && !fed)) return SP_ENULL;
    if (npairs < 1 || !(gap <= 0) || !(gap > -INFINITY)) return SP_EINVAL;
    hipLaunchKernelGGL(sequence_kernel, dim3((unsigned)sp_cdiv(npairs, 4)), dim3(256), 0, (hipStream_t)stream, labels, start, count, pairs,
                       npairs, gap, ss, fed);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
