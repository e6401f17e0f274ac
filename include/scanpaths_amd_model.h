/*
 * scanpaths_amd_model.h -- C ABI of libscanpaths_amd_model.so, the statistics of the MODEL read in closed form from its step
 * distributions.  A library of its own because the entry points of scanpaths_amd.h and of scanpaths_amd_stats.h are
 * pinned by their tests: it exports none of their symbols and they declare none of these.  THIS library is not pinned to a set of
 * entry points: the next closed-form statistic of the model goes in here, with SP_MODEL_ABI_VERSION bumped, not into a fourth library.
 * Conventions and return codes (SP_OK, SP_EINVAL, SP_ENULL) are those of scanpaths_amd.h: device pointers borrowed from the caller,
 * `stream` a hipStream_t passed as void*, every call only enqueues work.  The declarations keep the forms scanpaths_amd/_abi.py reads.
 */
#ifndef SCANPATHS_AMD_MODEL_H
#define SCANPATHS_AMD_MODEL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_MODEL_ABI_VERSION 1
int sp_model_abi_version(void);

/* the kernels' limits: steps per row that count (64), cells per map (2048) -- the values of sp_scan_max_fixations() and
 * sp_scan_likelihood_max_cells() of the main library (one scan_common.h) */
int sp_model_max_fixations(void);
int sp_model_max_cells(void);

/* The expected fixation map of the sampler's scanpaths (csrc/scanexpect.hip): probs [R][T][1 + Hm Wm] float32 are the model's step
 * distributions (action 0 = terminate), Tm = min(T, max_steps), Z, D, q, c, A as sp_scan_saccade_expectation computes them.  Fixation t
 * of a sample exists iff no terminate was drawn up to and including step t and its cell is drawn from step t's map alone:
 *   f_t = A_t * step_weight[r][t] (A_t itself when step_weight is NULL),  e_r(i) = sum_t c_t(i) f_t  (c_t(i) = p_t(i) / D_t is the
 *   probability of cell i AND no terminate at step t: the cells of a step add up to 1 - q_t),  w_t = A_t (1 - q_t),
 *   fixations[r] = sum_t w_t,  m_g(i) = the e_r(i) of the good rows of group g in ascending row index,
 *   maps[g][px] = the m_g(i) of the cells with cell_pixel[i] == px in ascending cell index
 * (the order of every sum: scanpaths_amd/csrc/scanexpect.hip; no floating-point atomics).  step_weight: NULL or float64 [R][T], the
 * weight of a fixation of step t (its mean duration for a duration-weighted map); row_group int32 [R]; cell_pixel int32 [Hm Wm]: the
 * output pixel row * W + col of every cell (several cells may share a pixel; a pixel without a cell is 0.0; an entry outside
 * [0, H W) is skipped with its mass and never stored through); maps float64 [ngroups][H][W], every element written exactly once (an
 * empty group is a zero map); fixations float64 [R]; bad int32 [R]: 1 for a row with a step t < Tm whose D_t is zero or not finite or
 * whose step_weight is not finite or negative (fixations NaN, nothing added), -1 for a row_group outside [0, ngroups) (fixations NaN,
 * nothing of the row read).  work: scratch of sp_model_fixation_expectation_workspace(R, T, Hm, Wm, ngroups, max_steps) doubles
 * (SP_EINVAL for scalars the launcher refuses).
 * SP_ENULL for a NULL pointer other than step_weight, then SP_EINVAL for a scalar out of range -- R >= 0, T >= 1, Hm, Wm >= 1 with at
 * most 2048 cells, ngroups >= 0, min_length >= 0, max_steps in [1, 64], H, W >= 1 with H W within int -- both before any launch. */
int64_t sp_model_fixation_expectation_workspace(int R, int T, int Hm, int Wm, int ngroups, int max_steps);
int sp_model_fixation_expectation(const float* probs, const double* step_weight, const int* row_group, int R, int T, int Hm, int Wm,
                                  int ngroups, int min_length, int max_steps, const int* cell_pixel, int H, int W, double* work,
                                  double* maps, double* fixations, int* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
