/*
 * scanpaths_amd_stats.h -- C ABI of libscanpaths_amd_stats.so, the descriptive scanpath statistics that came after the entry points
 * of scanpaths_amd.h were pinned.  A library of its own: it exports none of the symbols scanpaths_amd.h declares, and
 * scanpaths_amd.h declares none of these.  Conventions, return codes (SP_OK, SP_EINVAL, SP_ENULL) and the fixation layout are those of
 * scanpaths_amd.h: device pointers borrowed from the caller, `stream` a hipStream_t passed as void*, every call only enqueues work.
 * The declarations keep the forms scanpaths_amd/_abi.py reads.
 */
#ifndef SCANPATHS_AMD_STATS_H
#define SCANPATHS_AMD_STATS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_STATS_ABI_VERSION 1
int sp_stats_abi_version(void);

/* the kernels' limits: fixations per scanpath and steps per table side (64), cells per map (2048) -- the values of
 * sp_scan_max_fixations() and sp_scan_likelihood_max_cells() of the main library (one scan_common.h) */
int sp_stats_max_fixations(void);
int sp_stats_max_cells(void);

/* Recurrence: how often a scanpath comes back to a place it has looked at, and after how many fixations (Anderson et al. 2013, the
 * auto-recurrence form, on action-map cells).  A fixation is read as its cell by the pixel rule of sp_scan_saccade_counts; fixations s
 * and t are recurrent iff mask[(dr + Hm - 1) * (2 Wm - 1) + dc + Wm - 1] != 0 for their cell displacement (dr, dc) -- the caller's
 * table of (2 Hm - 1)(2 Wm - 1) bytes, only read here.  One table [max_steps][max_steps] per group, max_steps in [1, 64]; for s < t
 * entry [s][t] holds the recurrent pairs (fixation s, fixation t), entry [t][s] the pairs that exist at all and entry [t][t] the
 * fixations t.
 *
 * sp_stats_recurrence_counts (a zeroing launch, then one wavefront per scanpath): scanpaths that exist, in the layout fix [total][ncol]
 * | start | count | group of sp_scan_saccade_counts; only the first min(count, max_steps) fixations count, a fixation outside the frame
 * or with a non-finite coordinate is dropped: it is in no pair.  counts int64 [ngroups][max_steps][max_steps]: integer atomics, exact.
 * points int32 [nscan] = the scanpath's recurrent pairs, dropped int32 [nscan], rqa int32 [nscan][6] = N (kept fixations), R (= points),
 * the points on diagonal, horizontal and vertical lines of at least min_line >= 2 points of the upper triangle (main diagonal
 * excluded, lines in original ordinals: a dropped fixation breaks every line through it) and sum (t - s) over the recurrent pairs.  A
 * count outside [0, 64] or a group outside [0, ngroups): points -1, dropped 0, rqa -1 six times, no row read, nothing counted.
 *
 * sp_stats_recurrence_expectation (one launch that lists the mask's displacements, one block per (row, step), one thread per row, one
 * thread per (group, entry)): the model's step distributions probs [R][T][1 + Hm Wm] in closed form, Tm = min(T, max_steps), Z, D, q, c,
 * A as sp_scan_saccade_expectation computes them:
 *   E[s][t] = (A_s G_st) X_st,  E[t][s] = (A_s G_st) ((1 - q_s)(1 - q_t)),  E[t][t] = A_t (1 - q_t),  G_st = prod_{s<u<t} (1 - q_u),
 *   X_st = sum_i c_s(i) B_t(i),  B_t(i) = the sum of c_t over the cells within the mask of cell i
 * (the order of every sum: scanpaths_amd/csrc/scanrecur.hip).  E float64 [ngroups][max_steps][max_steps] adds the good rows of a
 * group in ascending row index (no floating-point atomics); points float64 [R] = sum_{s<t} E_r[s][t]; bad int32 [R]: 1 for a row with
 * a step t < Tm whose D_t is zero or not finite (points NaN, nothing added), -1 for a row_group outside [0, ngroups) (points NaN,
 * nothing of the row read).  work: scratch of R Tm Tm + (2 Hm - 1)(2 Wm - 1) / 2 + 1 doubles.
 * SP_ENULL for a NULL pointer, then SP_EINVAL for a scalar out of range; both before any launch. */
int sp_stats_recurrence_counts(const double* fix, int ncol, const int64_t* start, const int* count, const int* group, int nscan,
                               int ngroups, int max_steps, int Hm, int Wm, double frame_w, double frame_h, const uint8_t* mask,
                               int min_line, int64_t* counts, int* points, int* dropped, int* rqa, void* stream);
int sp_stats_recurrence_expectation(const float* probs, const int* row_group, int R, int T, int Hm, int Wm, int ngroups, int min_length,
                                    int max_steps, const uint8_t* mask, double* work, double* E, double* points, int* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
