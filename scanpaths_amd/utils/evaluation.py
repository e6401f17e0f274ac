"""Evaluation on the host: what is scored, for whom, and how the scores of a call are grouped; the scoring itself runs on the device
(utils/evaltools/, one batched call per measure).  A map of this file:

  Reference-interface half (the functions of the reference's utils/evaluation.py, its arguments, result layouts and quirks; SURVEY.md §8
  rows f1-f3): pairs_eval_scanmatch_performance_related / gtpairs_eval_scanmatch_performance_related -- the ScanMatch reward of the RL
  (self-critical) phase --, evaluation_performance_related / human_evaluation* / evaluation / pairs_eval -- the validation and test
  tables --, pairs_eval_scanmatch.  The reference scores every (ground-truth, other) scanpath pair inside nested python loops; here the pairs of a
  whole call are collected first, scored by one device call per measure (csrc/scanmatch.hip: one wavefront per pair) and grouped exactly
  as the reference groups them.  Fixation vectors are the reference's structured arrays (start_x, start_y, duration in seconds) or
  plain [n, 3] arrays; durations become milliseconds as in the reference.  Any object with the reference's ScanMatch methods works; one that also offers
  sequences / match_pairs (the HIP ScanMatch) is driven in batched form.

  Keyed half (from predict_results_fix_vectors down): measures the reference's tables do not hold.  Every call takes scanpaths with a key
  each (a question id, an image name) and returns (means, per_key), per_key in first-appearance order of the keys.  _keyed / _key_index
  check the keys; _model_pairs / _ceiling_pairs / _pair_tables serve the pair measures (saliency_*, scanpath_distance_*,
  sequence_score_*); the model-side calls that read the model's distributions instead of samples (likelihood_*, search_efficiency_model_*,
  saccade_statistics_model_*, turn_statistics_model_*, recurrence_statistics_model_*, saliency_model_*) get their entries from _head_entries; _pool is the mean per key with its pooled sum and count, _key_means
  the mean over keys.

  Tables: LikelihoodTable, SearchEfficiencyTable, SaccadeStatisticsTable, TurnStatisticsTable, RecurrenceStatisticsTable, SaliencyModelTable merge the means of several batches (_SumTable holds the merge).

  Bootstrap: bootstrap_evaluation / bootstrap_comparison / bootstrap_information_gain_explained put intervals on any per_key table."""
from __future__ import annotations

from collections import namedtuple
from typing import List, Sequence, Tuple

import numpy as np

from .evaltools._args import (MAX_CELLS, MAX_DIRECTIONS, check_directions, check_edges, check_frame, check_map, check_map_shape, check_min_length,
                              check_steps)


def _as_ms(fv) -> np.ndarray:
    a = np.array([list(_) for _ in list(fv)], dtype=np.float64).reshape(-1, 3)
    a[:, -1] *= 1000
    return a


def _score_pairs(sm, paths: List[np.ndarray], pairs: Sequence[Tuple[int, int]]) -> np.ndarray:
    if not pairs:
        return np.zeros(0)
    if hasattr(sm, "match_pairs") and hasattr(sm, "sequences"):
        import torch
        seq, ln = sm.sequences(paths)
        return sm.match_pairs(seq, ln, seq, ln, torch.tensor(list(pairs), dtype=torch.int32)).cpu().numpy()
    seqs = [sm.fixationToSequence(p).astype(np.int32) for p in paths]
    return np.array([sm.match(seqs[i], seqs[j])[0] for i, j in pairs], dtype=np.float64)


def _group_mean(rows: np.ndarray, is_eliminating_nan: bool):
    """rows [k, 2] of one group -> (metric [2], emptied_by_nan)"""
    emptied = False
    if is_eliminating_nan and rows.shape[0] != 0:
        rows = rows[np.isnan(rows.sum(axis=1)) == False]          # noqa: E712  (as the reference)
        emptied = rows.shape[0] == 0
    if rows.shape[0] != 0:
        return np.sum(rows, axis=0) / rows.shape[0], emptied
    return np.array([np.nan] * 2), emptied


def pairs_eval_scanmatch_performance_related(gt_fix_vectors, predict_fix_vectors, ScanMatchwithDuration,
                                             ScanMatchwithoutDuration, performance, given_performance,
                                             is_eliminating_nan=True):
    """(utils/evaluation.py:361-422) per image: mean ScanMatch of the prediction against the ground-truth scanpaths whose
    performance equals ``given_performance`` (same) and against the others (diff)."""
    paths, pairs, owner = [], [], []
    for index in range(len(gt_fix_vectors)):
        pi = len(paths)
        paths.append(_as_ms(predict_fix_vectors[index]))
        for inner_index in range(len(gt_fix_vectors[index])):
            paths.append(_as_ms(gt_fix_vectors[index][inner_index]))
            pairs.append((len(paths) - 1, pi))                     # match(gt, prediction), as the reference
            owner.append((index, performance[index][inner_index] == given_performance))
    wd = _score_pairs(ScanMatchwithDuration, paths, pairs)
    wod = _score_pairs(ScanMatchwithoutDuration, paths, pairs)
    accept_flag = True
    same_out, diff_out = [], []
    for index in range(len(gt_fix_vectors)):
        same = np.array([[wod[k], wd[k]] for k, (i, s) in enumerate(owner) if i == index and s]).reshape(-1, 2)
        diff = np.array([[wod[k], wd[k]] for k, (i, s) in enumerate(owner) if i == index and not s]).reshape(-1, 2)
        m_same, e1 = _group_mean(same, is_eliminating_nan)
        m_diff, e2 = _group_mean(diff, is_eliminating_nan)
        if e1 or e2:
            accept_flag = False
        same_out.append(m_same)
        diff_out.append(m_diff)
    return np.array(same_out), np.array(diff_out), accept_flag


def gtpairs_eval_scanmatch_performance_related(gt_fix_vectors, ScanMatchwithDuration, ScanMatchwithoutDuration, performance,
                                               is_eliminating_nan=True):
    """(utils/evaluation.py:425-576) per image: mean ScanMatch among the good-performance ground-truth scanpaths, among the
    poor ones, and between the two groups (the last only when BOTH groups have more than one member, as the reference)."""
    paths, pairs, owner = [], [], []
    for index, (gt_fix_vector, performance_val) in enumerate(zip(gt_fix_vectors, performance)):
        base = len(paths)
        for fv in gt_fix_vector:
            paths.append(_as_ms(fv))
        good = [base + k for k in range(len(performance_val)) if performance_val[k] == True]       # noqa: E712
        poor = [base + k for k in range(len(performance_val)) if not performance_val[k] == True]   # noqa: E712
        for grp, tag in ((good, "good"), (poor, "poor")):
            if len(grp) > 1:
                for a in range(len(grp)):
                    for b in range(a + 1, len(grp)):
                        pairs.append((grp[a], grp[b]))
                        owner.append((index, tag))
        if len(good) > 1 and len(poor) > 1:
            for a in good:
                for b in poor:
                    pairs.append((a, b))
                    owner.append((index, "diff"))
    wd = _score_pairs(ScanMatchwithDuration, paths, pairs)
    wod = _score_pairs(ScanMatchwithoutDuration, paths, pairs)
    out = {"good": [], "poor": [], "diff": []}
    for index in range(len(gt_fix_vectors)):
        for tag in out:
            rows = np.array([[wod[k], wd[k]] for k, (i, t) in enumerate(owner) if i == index and t == tag]).reshape(-1, 2)
            out[tag].append(_group_mean(rows, is_eliminating_nan)[0])
    return np.array(out["good"]), np.array(out["poor"]), np.array(out["diff"])


# ====================================================================================================================
# Validation / test metrics: evaluation_performance_related (utils/evaluation.py:188-359) and human_evaluation (:11-186).
# The reference runs, per (ground-truth, other) scanpath pair, MultiMatch (third-party multimatch_gaze==0.1.2, sp_baseline.yml:65,
# NOT vendored), two pure-python Needleman-Wunsch ScanMatch runs, SED and STDE inside nested loops.  Here the pairs of the whole
# call are collected first, ScanMatch (x2) / SED / STDE are scored by three batched device calls, and the per-image grouping,
# means / stds and the "best SED / STDE" columns are assembled exactly as the reference does.
# MultiMatch: ``multimatch`` = a callable docomparison(fv1, fv2, screensize=[320, 240]) -> 5 values.  Default: the installed
# multimatch_gaze if importable, else utils/evaltools/multimatch.py (a restatement of the published algorithm, parity unpinned).
# ``multimatch_grouping`` (keyword only; None = the reference's call, no simplification) = (TDir degrees, TDur, TAmp pixels): MultiMatch's
# scanpath simplification first -- the device default simplifies and scores every pair of the call on the device, a
# callable is called with grouping=True, TDir=, TDur=, TAmp= (multimatch_gaze's own signature).
# Quirk kept: the dict entry "w/o duration" holds column 5 = the score WITH duration and vice versa (:292-293 append the
# with-duration score first, :323-324 label them the other way round).
# ====================================================================================================================
def _default_multimatch():
    """the installed multimatch_gaze (the reference's dependency) if the user has it; else None = the batched device restatement
    (utils/evaltools/multimatch.multimatch_pairs: every pair of the call in one launch)"""
    try:
        import multimatch_gaze as mm
        return mm.docomparison
    except Exception:
        return None


def _grouping_kwargs(multimatch_grouping):
    """None -> None; a (TDir, TDur, TAmp) triple -> the keyword arguments of docomparison / multimatch_pairs (checked here, before
    any scoring)"""
    if multimatch_grouping is None:
        return None
    from .evaltools.multimatch import _thresholds
    try:
        tdir, tdur, tamp = multimatch_grouping
    except (TypeError, ValueError):
        raise ValueError(f"multimatch_grouping is None or a (TDir, TDur, TAmp) triple: {multimatch_grouping!r}") from None
    _thresholds(tdir, tdur, tamp)
    return {"grouping": True, "TDir": float(tdir), "TDur": float(tdur), "TAmp": float(tamp)}


def _multimatch_rows(mm, candidates, grouping=None):
    """candidates: list of (fixation vectors 1, fixation vectors 2) -> list of 5-value rows (NaNs where MultiMatch cannot score).
    mm None: one device launch for all candidates; else the per-pair callable (the reference's loop).  grouping: None or the
    keyword arguments of _grouping_kwargs."""
    if not candidates:
        return []
    if mm is not None:
        if grouping is not None:
            return [list(mm(a, b, screensize=[320, 240], **grouping)) for a, b in candidates]
        return [list(mm(a, b, screensize=[320, 240])) for a, b in candidates]
    from .evaltools.multimatch import multimatch_pairs
    paths, pairs = [], []
    for a, b in candidates:
        paths.extend([a, b])
        pairs.append((len(paths) - 2, len(paths) - 1))
    if grouping is not None:
        return [list(r) for r in multimatch_pairs(paths, pairs, [320, 240], **grouping)]
    return [list(r) for r in multimatch_pairs(paths, pairs, [320, 240])]


def _rows_for_pairs(paths, pairs, sm_wd, sm_wod, mm_rows):
    """[npairs, 9] float64: 5 MultiMatch values, ScanMatch with duration, without duration, SED, STDE for (gt, other) pairs;
    sm_wd None: the pair of ScanMatch objects of _make_scanmatch"""
    from .evaltools.visual_attention_metrics import sed_stde_pairs
    if sm_wd is None:
        sm_wd, sm_wod = _make_scanmatch()
    if not pairs:
        return np.zeros((0, 9))
    wd = _score_pairs(sm_wd, paths, pairs)
    wod = _score_pairs(sm_wod, paths, pairs)
    sed, stde = sed_stde_pairs(paths, pairs, (240, 320, 3))
    out = np.empty((len(pairs), 9), dtype=np.float64)
    out[:, :5] = np.asarray(mm_rows, dtype=np.float64).reshape(-1, 5)
    out[:, 5], out[:, 6] = wd, wod
    out[:, 7], out[:, 8] = sed.cpu().numpy(), stde.cpu().numpy()
    return out


def _summarise(collect_all, collect_right, collect_wrong, mean_name):
    keep = lambda lst: [a for a in lst if len(a) != 0]
    collected = [keep(collect_all), keep(collect_right), keep(collect_wrong)]
    summary_mean, summary_std = [], []
    for specific in collected:
        rl = np.concatenate(specific, axis=0)
        mean, std = rl.mean(0), rl.std(0)
        tmp = np.concatenate([np.concatenate([[a[:, 7].min(keepdims=True), a[:, 8].max(keepdims=True)]]).transpose((1, 0))
                              for a in specific], axis=0)
        summary_mean.append(np.concatenate([mean, tmp.mean(0)], axis=0))
        summary_std.append(np.concatenate([std, tmp.std(0)], axis=0))
    out = []
    for summ in (summary_mean, summary_std):
        d = dict()
        for category, v in zip(["all", "right_answer", "wrong_answer"], summ):
            d[category] = {"MultiMatch": {"vector": v[0], "direction": v[1], "length": v[2], "position": v[3], "duration": v[4]},
                           "ScanMatch": {"w/o duration": v[5], "with duration": v[6]},
                           "VAME": {"SED": v[7], "STDE": v[8], "SED_best": v[9], "STDE_best": v[10]}}
        out.append(d)
    return out[0], out[1]


def _make_scanmatch():
    from .evaltools.scanmatch import ScanMatch
    return (ScanMatch(Xres=320, Yres=240, Xbin=16, Ybin=12, Offset=(0, 0), TempBin=50, Threshold=3.5),
            ScanMatch(Xres=320, Yres=240, Xbin=16, Ybin=12, Offset=(0, 0), Threshold=3.5))


def evaluation_performance_related(gt_fix_vectors, predict_fix_vectors, all_performances, all_allocated_performances,
                                   multimatch=None, *, multimatch_grouping=None):
    """(utils/evaluation.py:188-359)  -> cur_metrics, cur_metrics_std, scores_of_each_images"""
    mm = multimatch or _default_multimatch()
    grouping = _grouping_kwargs(multimatch_grouping)
    sm_wd, sm_wod = _make_scanmatch()
    cand = [(gt_fix_vectors[index][inner], predict_fix_vectors[index], index, inner)
            for index in range(len(gt_fix_vectors)) for inner in range(len(gt_fix_vectors[index]))]
    mm_all = _multimatch_rows(mm, [(a, b) for a, b, _, _ in cand], grouping)
    paths, pairs, mm_rows, owner = [], [], [], []
    pred_slot = {}
    for (gt, pred, index, inner_index), rlt in zip(cand, mm_all):
        if index not in pred_slot:
            pred_slot[index] = len(paths)
            paths.append(_as_ms(pred))
        if np.any(np.isnan(np.asarray(rlt, dtype=np.float64))):
            continue                                                    # (:215-217) pairs MultiMatch cannot score are dropped
        paths.append(_as_ms(gt))
        pairs.append((len(paths) - 1, pred_slot[index]))
        mm_rows.append(rlt)
        owner.append((index, inner_index))
    rows = _rows_for_pairs(paths, pairs, sm_wd, sm_wod, mm_rows)
    collect_all, collect_right, collect_wrong, scores_of_each_images = [], [], [], []
    k = 0
    for index in range(len(gt_fix_vectors)):
        sample_all, sample_right, sample_wrong = [], [], []
        while k < len(owner) and owner[k][0] == index:
            inner_index = owner[k][1]
            r = list(rows[k])
            sample_all.append(r)
            if all_performances[index][inner_index] == True and all_allocated_performances[index] == True:      # noqa: E712
                sample_right.append(r)
            elif all_performances[index][inner_index] == False and all_allocated_performances[index] == False:  # noqa: E712
                sample_wrong.append(r)
            k += 1
        collect_all.append(np.array(sample_all, dtype=np.float32))
        collect_right.append(np.array(sample_right, dtype=np.float32))
        collect_wrong.append(np.array(sample_wrong, dtype=np.float32))
        chosen = sample_right if all_allocated_performances[index] == True else sample_wrong                   # noqa: E712
        scores_of_each_images.append(list(np.array(chosen).mean(axis=0)) if chosen != [] else list(np.zeros((9,), dtype=np.float64)))
    cur_metrics, cur_metrics_std = _summarise(collect_all, collect_right, collect_wrong, "cur")
    return cur_metrics, cur_metrics_std, scores_of_each_images


def human_evaluation(dataloader, multimatch=None, *, multimatch_grouping=None):
    """(utils/evaluation.py:11-186)  every ordered pair of distinct human scanpaths of an image; dataloader yields batches with
    "fix_vectors", "performances", "question_ids"  -> human_metrics, human_metrics_std, scores_of_each_images_dict"""
    mm = multimatch or _default_multimatch()
    grouping = _grouping_kwargs(multimatch_grouping)
    sm_wd, sm_wod = _make_scanmatch()
    paths, images, gt_qid_name, cand = [], [], [], []
    for batch in dataloader:
        gt_qid_name.extend(batch["question_ids"])
        for fix_vectors, performances in zip(batch["fix_vectors"], batch["performances"]):
            img = len(images)
            images.append(performances)
            base = len(paths)
            for fv in fix_vectors:
                paths.append(_as_ms(fv))
            for index_1 in range(len(fix_vectors)):
                for index_2 in range(len(fix_vectors)):
                    if index_2 != index_1:
                        cand.append((fix_vectors[index_1], fix_vectors[index_2], base + index_1, base + index_2, (img, index_1, index_2)))
    mm_all = _multimatch_rows(mm, [(a, b) for a, b, _, _, _ in cand], grouping)
    pairs, mm_rows, owner = [], [], []
    for (_, _, p1, p2, own), rlt in zip(cand, mm_all):
        if np.any(np.isnan(np.asarray(rlt, dtype=np.float64))):
            continue
        pairs.append((p1, p2))
        mm_rows.append(rlt)
        owner.append(own)
    rows = _rows_for_pairs(paths, pairs, sm_wd, sm_wod, mm_rows)
    collect_all, collect_right, collect_wrong, good_scores, poor_scores = [], [], [], [], []
    k = 0
    for img, performances in enumerate(images):
        sample_all, sample_right, sample_wrong = [], [], []
        while k < len(owner) and owner[k][0] == img:
            _, i1, i2 = owner[k]
            r = list(rows[k])
            sample_all.append(r)
            if performances[i1] == True and performances[i2] == True:        # noqa: E712
                sample_right.append(r)
            elif performances[i1] == False and performances[i2] == False:    # noqa: E712
                sample_wrong.append(r)
            k += 1
        collect_all.append(np.array(sample_all, dtype=np.float32))
        collect_right.append(np.array(sample_right, dtype=np.float32))
        collect_wrong.append(np.array(sample_wrong, dtype=np.float32))
        good_scores.append(list(np.array(sample_right, dtype=np.float64).mean(axis=0)) if sample_right != [] else list(np.zeros((9,))))
        poor_scores.append(list(np.array(sample_wrong, dtype=np.float64).mean(axis=0)) if sample_wrong != [] else list(np.zeros((9,))))
    human_metrics, human_metrics_std = _summarise(collect_all, collect_right, collect_wrong, "human")
    scores = {name: dict([(True, g), (False, p)]) for name, g, p in zip(gt_qid_name, good_scores, poor_scores)}
    return human_metrics, human_metrics_std, scores


# ====================================================================================================================
# OSIE / COCO_Search18 forms (SURVEY.md §8 rows f2 / f3 widened).  Free-viewing / visual-search scanpaths carry no answer
# correctness, so there is no performance split: ONE metric set per call instead of all / right / wrong.
#   evaluation(gt, pred)             OSIE/utils/evaluation.py:151-282 == COCO_Search18/utils/evaluation.py:180-311 (identical code)
#   human_evaluation(loader, task=)  OSIE :11-148 (SED / STDE reshaped to [-1, n - 1]: equal scanpath counts; MultiMatch NaN rows NOT
#                                    eliminated) / COCO_Search18 :11-178 (per-image ranges: ragged counts; NaN rows eliminated)
#   pairs_eval                       OSIE :284-340  (RL reward, 11 columns)
#   pairs_eval_scanmatch             COCO_Search18 :313-352 (RL reward, 2 columns)
# As above: the pairs of a whole call are scored by batched device launches (ScanMatch x2, SED / STDE, MultiMatch), the grouping and the
# statistics follow the reference line by line -- including (a) the per-pair rows hold the score WITH duration in column 5 and the one
# WITHOUT in column 6 while the dicts are labelled correctly here (unlike AiR's :323-324), (b) pairs_eval divides an image's column sums
# by the FULL number of its human scanpaths even after NaN rows were eliminated (:329), (c) pairs_eval scores ScanMatch / SED / STDE only
# for the pairs MultiMatch could score.
# ====================================================================================================================
def _flat_metrics(mm_mean, mm_std, wd, wod, sed_all, stde_all, sed_best, stde_best):
    mean = {"MultiMatch": dict(zip(("vector", "direction", "length", "position", "duration"), mm_mean)),
            "ScanMatch": {"w/o duration": np.mean(wod), "with duration": np.mean(wd)},
            "VAME": {"SED": sed_all.mean(), "STDE": stde_all.mean(), "SED_best": sed_best.mean(), "STDE_best": stde_best.mean()}}
    std = {"MultiMatch": dict(zip(("vector", "direction", "length", "position", "duration"), mm_std)),
           "ScanMatch": {"w/o duration": np.std(wod), "with duration": np.std(wd)},
           "VAME": {"SED": sed_all.std(), "STDE": stde_all.std(), "SED_best": sed_best.std(), "STDE_best": stde_best.std()}}
    return mean, std


def evaluation(gt_fix_vectors, predict_fix_vectors, is_eliminating_nan=True, multimatch=None, *, multimatch_grouping=None):
    """(OSIE/utils/evaluation.py:151-282, COCO_Search18/utils/evaluation.py:180-311) -> cur_metrics, cur_metrics_std, scores_of_each_images.
    Every (human scanpath of the image, prediction) pair; like the reference, SED / STDE are regrouped as [-1, number of human
    scanpaths of the LAST image] for the "best" columns (equal counts per image expected)."""
    mm = multimatch or _default_multimatch()
    grouping = _grouping_kwargs(multimatch_grouping)
    paths, pairs, cand, per_image = [], [], [], []
    for index in range(len(gt_fix_vectors)):
        pi = len(paths)
        paths.append(_as_ms(predict_fix_vectors[index]))
        per_image.append(len(gt_fix_vectors[index]))
        for inner in gt_fix_vectors[index]:
            paths.append(_as_ms(inner))
            pairs.append((len(paths) - 1, pi))
            cand.append((inner, predict_fix_vectors[index]))
    mm_rows = _multimatch_rows(mm, cand, grouping)
    rows = _rows_for_pairs(paths, pairs, None, None, mm_rows)
    scores_of_each_images, k = [], 0
    for n in per_image:
        scores_of_each_images.append(list(np.array([list(r) for r in rows[k:k + n]]).mean(axis=0)))
        k += n
    mmr = rows[:, :5]
    if is_eliminating_nan:
        mmr = mmr[np.isnan(mmr.sum(axis=1)) == False]          # noqa: E712
    sed = rows[:, 7].reshape(-1, per_image[-1])
    stde = rows[:, 8].reshape(-1, per_image[-1])
    mean, std = _flat_metrics(np.mean(mmr, axis=0), np.std(mmr, axis=0), rows[:, 5], rows[:, 6], sed, stde, sed.min(-1), stde.max(-1))
    return mean, std, scores_of_each_images


def human_evaluation_free_viewing(dataloader, task="OSIE", multimatch=None, *, multimatch_grouping=None):
    """human_evaluation of OSIE (:11-148) / COCO_Search18 (:11-178): every ordered pair of distinct human scanpaths of an image;
    batches carry "fix_vectors" and "img_names" -> human_metrics, human_metrics_std, {image name: mean score row of the image}"""
    assert task in ("OSIE", "COCO_Search18"), task
    mm = multimatch or _default_multimatch()
    grouping = _grouping_kwargs(multimatch_grouping)
    paths, pairs, cand, names, groups = [], [], [], [], []       # groups: per image, per first scanpath: number of pairs (n - 1)
    for batch in dataloader:
        names.extend(batch["img_names"])
        for fix_vectors in batch["fix_vectors"]:
            base = len(paths)
            for fv in fix_vectors:
                paths.append(_as_ms(fv))
            n = len(fix_vectors)
            groups.append(n)
            for i1 in range(n):
                for i2 in range(n):
                    if i2 != i1:
                        pairs.append((base + i1, base + i2))
                        cand.append((fix_vectors[i1], fix_vectors[i2]))
    rows = _rows_for_pairs(paths, pairs, None, None, _multimatch_rows(mm, cand, grouping))
    scores, k = [], 0
    for n in groups:
        cnt = n * (n - 1)
        scores.append(list(np.array([list(r) for r in rows[k:k + cnt]]).mean(axis=0)))
        k += cnt
    mmr = rows[:, :5]
    if task == "COCO_Search18":
        mmr = mmr[np.isnan(mmr.sum(axis=1)) == False]          # noqa: E712  (:79; OSIE keeps the NaN rows, its means turn NaN)
        sed_best, stde_best, k = [], [], 0
        for n in groups:                                        # (:88-125) best over ALL ordered pairs of the image
            cnt = n * (n - 1)
            sed_best.append(rows[k:k + cnt, 7].min())
            stde_best.append(rows[k:k + cnt, 8].max())
            k += cnt
        sed_all, stde_all = rows[:, 7], rows[:, 8]
        sed_best, stde_best = np.array(sed_best), np.array(stde_best)
    else:
        sed_all = rows[:, 7].reshape(-1, groups[-1] - 1)       # (:86-87) one row per first scanpath: best over its n - 1 partners
        stde_all = rows[:, 8].reshape(-1, groups[-1] - 1)
        sed_best, stde_best = sed_all.min(-1), stde_all.max(-1)
    mean, std = _flat_metrics(np.mean(mmr, axis=0), np.std(mmr, axis=0), rows[:, 5], rows[:, 6], sed_all, stde_all, sed_best, stde_best)
    return mean, std, dict(zip(names, scores))


def pairs_eval(gt_fix_vectors, predict_fix_vectors, ScanMatchwithDuration, ScanMatchwithoutDuration, is_eliminating_nan=True,
               multimatch=None):
    """(OSIE/utils/evaluation.py:284-340) RL reward of one sampled scanpath per image -> [N, 11] float: the 5 MultiMatch means, ScanMatch
    without / with duration, SED, STDE (column sums over the scorable pairs divided by the image's FULL number of human scanpaths),
    best SED (min) and best STDE (max); a NaN row where nothing was scorable (OSIE/train.py:236-238 then redraws the sample)."""
    mm = multimatch or _default_multimatch()
    cand = [(gt, predict_fix_vectors[index]) for index in range(len(gt_fix_vectors)) for gt in gt_fix_vectors[index]]
    mm_all = _multimatch_rows(mm, cand)
    paths, pairs, mm_rows, owner, k = [], [], [], [], 0
    for index in range(len(gt_fix_vectors)):
        pi = len(paths)
        paths.append(_as_ms(predict_fix_vectors[index]))
        for gt in gt_fix_vectors[index]:
            rlt = mm_all[k]
            k += 1
            if np.any(np.isnan(np.asarray(rlt, dtype=np.float64))):
                owner.append((index, None))                     # row of NaNs (:296-299): ScanMatch / SED / STDE are not run for it
                continue
            paths.append(_as_ms(gt))
            pairs.append((len(paths) - 1, pi))
            mm_rows.append(rlt)
            owner.append((index, len(pairs) - 1))
    rows = _rows_for_pairs(paths, pairs, ScanMatchwithDuration, ScanMatchwithoutDuration, mm_rows)
    out = []
    for index in range(len(gt_fix_vectors)):
        coll = []
        for i, slot in owner:
            if i != index:
                continue
            if slot is None:
                coll.append([np.nan] * 9)
            else:
                r = rows[slot]
                coll.append(list(r[:5]) + [r[6], r[5], r[7], r[8]])          # (:323) [w/o duration, with duration, SED, STDE]
        coll = np.array(coll, dtype=np.float64).reshape(-1, 9)
        if is_eliminating_nan:
            coll = coll[np.isnan(coll.sum(axis=1)) == False]   # noqa: E712
        if coll.shape[0] != 0:
            metric_mean = np.sum(coll, axis=0) / len(gt_fix_vectors[index])
            v = np.zeros((11,), dtype=np.float32)
            v[:9] = metric_mean[:9]
            v[9], v[10] = coll[:, 7].min(), coll[:, 8].max()
        else:
            v = np.array([np.nan] * 11)
        out.append(v)
    return np.array(out)


def pairs_eval_scanmatch(gt_fix_vectors, predict_fix_vectors, ScanMatchwithDuration, ScanMatchwithoutDuration, is_eliminating_nan=True):
    """(COCO_Search18/utils/evaluation.py:313-352) RL reward -> [N, 2]: per image the ScanMatch score without / with duration of the
    sampled scanpath against its human scanpaths, column sums over the non-NaN rows divided by the FULL number of human scanpaths."""
    paths, pairs, owner = [], [], []
    for index in range(len(gt_fix_vectors)):
        pi = len(paths)
        paths.append(_as_ms(predict_fix_vectors[index]))
        for gt in gt_fix_vectors[index]:
            paths.append(_as_ms(gt))
            pairs.append((len(paths) - 1, pi))
            owner.append(index)
    wd = _score_pairs(ScanMatchwithDuration, paths, pairs)
    wod = _score_pairs(ScanMatchwithoutDuration, paths, pairs)
    out = []
    for index in range(len(gt_fix_vectors)):
        coll = np.array([[wod[k], wd[k]] for k, i in enumerate(owner) if i == index], dtype=np.float64).reshape(-1, 2)
        if is_eliminating_nan:
            coll = coll[np.isnan(coll.sum(axis=1)) == False]   # noqa: E712
        out.append(np.sum(coll, axis=0) / len(gt_fix_vectors[index]) if coll.shape[0] != 0 else np.array([np.nan] * 2))
    return np.array(out)


# ---- saliency scoring of sampled scanpaths (evaltools/saliency_maps.py, csrc/fixmaps.hip) ------------------------------------------------
def predict_results_fix_vectors(predict_results):
    """the ``predict_results`` records of inference.run_test_loop (qid, X, Y in the 320x240 sampling frame, T in ms) ->
    (fixation vectors [n, 3] with the duration in seconds, keys = the records' qid): the arguments saliency_evaluation takes"""
    fvs, keys = [], []
    for r in predict_results:
        x, y, t = (np.asarray(r[k], dtype=np.float64).reshape(-1) for k in ("X", "Y", "T"))
        if not (len(x) == len(y) == len(t)):
            raise ValueError(f"record of qid {r['qid']!r}: X, Y and T differ in length")
        fvs.append(np.stack([x, y, t / 1000.0], 1))
        keys.append(r["qid"])
    return fvs, keys


def _key_index(gt_keys, image_keys):
    """keys in first-appearance order -> (index of every key, image index per key or None): one image per key, or ValueError"""
    index = {}
    for k in gt_keys:
        index.setdefault(k, len(index))
    if image_keys is None:
        return index, None
    image_keys = list(image_keys)
    if len(image_keys) != len(gt_keys):
        raise ValueError("one image key per ground-truth fixation vector is required")
    images, of_key = {}, {}
    for k, im in zip(gt_keys, image_keys):
        if of_key.setdefault(k, im) != im:
            raise ValueError(f"key {k!r} is given on two images: {of_key[k]!r} and {im!r}")
        images.setdefault(im, len(images))
    return index, [images[of_key[k]] for k in index]


def _keyed(gt_fix_vectors, gt_keys, predict_fix_vectors=None, predict_keys=None, image_keys=None):
    """the keys of a keyed call, checked: one per fixation vector, every predicted key among gt_keys -> (gt_keys, predict_keys as
    lists, and the index / images of _key_index)"""
    gt_keys, predict_keys = list(gt_keys), [] if predict_keys is None else list(predict_keys)
    if len(gt_keys) != len(gt_fix_vectors) or len(predict_keys) != (0 if predict_fix_vectors is None else len(predict_fix_vectors)):
        raise ValueError("one key per fixation vector is required")
    index, images = _key_index(gt_keys, image_keys)
    unknown = [k for k in predict_keys if k not in index]
    if unknown:
        raise ValueError(f"predicted key {unknown[0]!r} ({len(unknown)} in all) is not among gt_keys")
    return gt_keys, predict_keys, index, images


def _members(index, gt_keys):
    """per key: the positions of its human scanpaths, in their order"""
    members = [[] for _ in index]
    for i, k in enumerate(gt_keys):
        members[index[k]].append(i)
    return members


def _model_pairs(index, gt_keys, predict_keys):
    """(pairs, owner): every human scanpath i of a key against every prediction j of the key, predictions numbered behind the human
    scanpaths; owner = (key, j), the pairs of one prediction next to each other"""
    members = _members(index, gt_keys)
    pairs, owner = [], []
    for j, k in enumerate(predict_keys):
        for i in members[index[k]]:
            pairs.append((i, len(gt_keys) + j))
            owner.append((index[k], j))
    return pairs, owner


def _ceiling_pairs(index, gt_keys):
    """(pairs, owner): every ordered pair (i, j) of distinct human scanpaths of a key, j as the "prediction"; owner = (key, j)"""
    pairs, owner = [], []
    for q, mem in enumerate(_members(index, gt_keys)):
        for j in mem:
            for i in mem:
                if i != j:
                    pairs.append((i, j))
                    owner.append((q, j))
    return pairs, owner


def _nanmean(v) -> Tuple[float, int]:
    """(the mean over the values that are not NaN, NaN without one; how many are NaN)"""
    nan = np.isnan(v)
    return float(v[~nan].mean()) if (~nan).any() else float("nan"), int(nan.sum())


def _key_means(per_key, names):
    """the means of a keyed call: means[name] = the mean over the keys that did not score NaN, means[name + "_nan"] = how many did"""
    means = {}
    for m in names:
        means[m], means[m + "_nan"] = _nanmean(per_key[m])
    return means


def _pool(values, owner, G):
    """values float64 [n], or curves [n, K], of owner[n] in [0, G) -> (per_key, total, count, n_nan): the mean per owner over its values
    that are not NaN (a curve: that hold no NaN; NaN for an owner without one), their sum over all owners, their number, and how many
    were left out"""
    flat = values.ndim == 1
    ok = ~np.isnan(values) if flat else ~np.isnan(values).any(1)
    cnt = np.bincount(owner[ok], minlength=G)
    if flat:
        ksum, total = np.bincount(owner[ok], weights=values[ok], minlength=G), float(values[ok].sum())
    else:
        ksum = np.stack([values[ok & (owner == g)].sum(0) for g in range(G)]) if G else np.zeros((0, values.shape[1]))
        cnt, total = cnt[:, None], values[ok].sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_key = np.where(cnt > 0, ksum / np.maximum(cnt, 1), np.nan)
    return per_key, total, int(ok.sum()), int((~ok).sum())


def saliency_evaluation(gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, frame_size=(240, 320), *, sigma, extra_metrics=(),
                        image_keys=None, **kw):
    """Saliency metrics of predicted scanpaths against human ones, one map set per distinct key (a question id, an image name: any
    hashable), in first-appearance order of gt_keys.  gt_fix_vectors[i] belongs to gt_keys[i], predict_fix_vectors[j] to
    predict_keys[j]; a predicted key that gt_keys does not hold raises ValueError.  sigma (pixels of the output map) is required;
    **kw goes to evaltools.saliency_maps.scanpath_saliency (output_shape, mode, pred_weight, truncate, uniform_mix, baseline_sigma).
    extra_metrics: any of "sAUC", "CC", "SIM", "IG" (Bylinskii et al. 2019 on sum-normalised maps, no min-max step; "IG" needs the
    keyword uniform_mix); image_keys[i]: the image gt_fix_vectors[i] was recorded on (default: every key is its own image; one key on
    two images raises ValueError) -- the shuffled AUC's negatives and the baseline of the information gain come from the OTHER images.
    Returns (means, per_key): means[metric] = nanmean over the keys and means[metric + "_nan"] = how many keys scored NaN, for
    AUC_Judd, NSS, KLdiv and every extra; per_key = {"keys": [...], metric: float64 [G] numpy arrays, "gt_dropped" / "pred_dropped":
    int [G]}.  The same call on the human side alone: saliency_human_evaluation (ceiling), saliency_centre_prior_evaluation (floor)."""
    from .evaltools.saliency_maps import scanpath_saliency
    gt_keys, predict_keys, index, images = _keyed(gt_fix_vectors, gt_keys, predict_fix_vectors, predict_keys, image_keys)
    if extra_metrics or images is not None:
        kw = dict(kw, extra_metrics=extra_metrics, image_groups=images)
    res = scanpath_saliency(gt_fix_vectors, [index[k] for k in gt_keys], predict_fix_vectors, [index[k] for k in predict_keys],
                            frame_size, sigma, num_groups=len(index), **kw)
    per_key = {"keys": list(index)}
    per_key.update({k: v.cpu().numpy() for k, v in res.items()})
    return _key_means(per_key, ("AUC_Judd", "NSS", "KLdiv") + tuple(extra_metrics)), per_key


def saliency_centre_prior_evaluation(gt_fix_vectors, gt_keys, frame_size=(240, 320), *, sigma, extra_metrics=(), image_keys=None, **kw):
    """The centre-prior floor of saliency_evaluation: the prediction of a key is its baseline, the blur of every human fixation
    recorded on the OTHER images -- what can be said about where people look without seeing the image.  Same arguments (without
    predictions), same (means, per_key) result; the information gain over the baseline is exactly 0 for every key that has one, and a
    key without another image scores NaN."""
    return saliency_evaluation(gt_fix_vectors, [], gt_keys, [], frame_size, sigma=sigma, extra_metrics=extra_metrics,
                               image_keys=image_keys, prediction="centre_prior", **kw)


def saliency_human_evaluation(gt_fix_vectors, gt_keys, frame_size=(240, 320), *, sigma, extra_metrics=(), image_keys=None, **kw):
    """The human ceiling of saliency_evaluation: for every key with at least two human scanpaths each scanpath in turn is held out as
    the human side and the other scanpaths of the key are the prediction; the key's score is the nanmean over its held-out scanpaths.
    A key with one scanpath scores NaN and is counted in means[metric + "_nan"] (its fixations still belong to the other keys' pools
    and baselines).  All held-out folds of the call are scored together by the launches of one saliency_evaluation call; the pool of
    a fold counts the held-out maps of the other images.  Same (means, per_key) result; gt_dropped / pred_dropped are sums over the
    folds."""
    from .evaltools.saliency_maps import scanpath_saliency
    gt_keys, _, index, images = _keyed(gt_fix_vectors, gt_keys, image_keys=image_keys)
    members = _members(index, gt_keys)
    fold_key = np.array([index[k] for k in gt_keys], dtype=np.int64)           # fold i holds out scanpath i
    pred, pred_fold = [], []
    for i, k in enumerate(gt_keys):
        for j in members[index[k]]:
            if j != i:
                pred.append(gt_fix_vectors[j])
                pred_fold.append(i)
    if extra_metrics or images is not None:
        kw = dict(kw, extra_metrics=extra_metrics, image_groups=fold_key if images is None else np.asarray(images)[fold_key])
    res = scanpath_saliency(gt_fix_vectors, np.arange(len(gt_keys)), pred, pred_fold, frame_size, sigma, num_groups=len(gt_keys), **kw)
    metrics = ("AUC_Judd", "NSS", "KLdiv") + tuple(extra_metrics)
    folds = {k: v.cpu().numpy() for k, v in res.items()}
    per_key = {"keys": list(index)}
    for m in metrics:
        per_key[m] = np.full(len(index), np.nan)
    for m in ("gt_dropped", "pred_dropped"):
        per_key[m] = np.zeros(len(index), dtype=np.int64)
        np.add.at(per_key[m], fold_key, folds[m])
    for q, mem in enumerate(members):
        if len(mem) < 2:
            continue
        for m in metrics:
            v = folds[m][mem]
            if not np.isnan(v).all():
                per_key[m][q] = np.nanmean(v)
    return _key_means(per_key, metrics), per_key


# ---- DTW, Frechet, Hausdorff, Eyenalysis and cross-recurrence of sampled scanpaths (evaltools/visual_attention_metrics.py, -------------
# ---- csrc/scandist.hip): measures the reference's tables do not hold, so they get a keyed call of their own ----------------------------
_LOWER_IS_BETTER = ("DTW", "Frechet", "Hausdorff", "Eyenalysis")
_HIGHER_IS_BETTER = ("REC", "DET", "LAM")            # CORM is signed: it has no best


def _xy(fv) -> np.ndarray:
    if isinstance(fv, np.ndarray) and fv.dtype.names is None and fv.ndim == 2:
        return np.asarray(fv[:, :2], dtype=np.float64)
    a = np.array([list(_) for _ in list(fv)], dtype=np.float64)
    return a.reshape(len(a), -1)[:, :2] if len(a) else np.zeros((0, 2))


def _distance_tables(index, paths, pairs, owner, metrics, max_dim, radius, min_line):
    """pairs[p] = (human path, predicted path) -> (means, per_key) of the keyed calls below"""
    from .evaltools.visual_attention_metrics import scanpath_distances_pairs
    scores = scanpath_distances_pairs(paths, pairs, metrics=metrics, max_dim=max_dim, radius=radius, min_line=min_line)
    return _pair_tables(index, scores, owner, metrics, _LOWER_IS_BETTER, _HIGHER_IS_BETTER)


def _pair_tables(index, scores, owner, metrics, lower_is_better, higher_is_better):
    """scores[metric] [npairs], owner[p] = (key index, prediction id), the pairs of one prediction next to each other -> (means, per_key)"""
    G = len(index)
    own = np.asarray(owner, dtype=np.int64).reshape(-1, 2)
    key_of_pair, pred_of_pair = own[:, 0], own[:, 1]

    def by_key(key_of):                                  # per key: the positions that belong to it, in their order
        order = np.argsort(key_of, kind="stable")
        return np.split(order, np.cumsum(np.bincount(key_of, minlength=G))[:-1])

    seg = np.flatnonzero(np.r_[True, pred_of_pair[1:] != pred_of_pair[:-1]]) if len(own) else np.zeros(0, dtype=np.int64)
    pairs_of_key, preds_of_key = by_key(key_of_pair), by_key(key_of_pair[seg])
    per_key = {"keys": list(index)}
    names = []
    for m in metrics:
        v = scores[m]
        per_key[m] = np.array([_nanmean(v[ps])[0] for ps in pairs_of_key], dtype=np.float64)
        names.append(m)
        if m in lower_is_better or m in higher_is_better:
            # the best over each prediction's human scanpaths (fmin / fmax skip NaN; all NaN stays NaN), then the mean over the key's predictions
            best = (np.fmin if m in lower_is_better else np.fmax).reduceat(v, seg) if len(seg) else np.zeros(0)
            per_key[m + "_best"] = np.array([_nanmean(best[ps])[0] for ps in preds_of_key], dtype=np.float64)
            names.append(m + "_best")
    return _key_means(per_key, names), per_key


def scanpath_distance_evaluation(gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, *, metrics, max_dim=1.0, radius=None,
                                 min_line=2):
    """DTW / Frechet / Hausdorff / Eyenalysis / REC / DET / LAM / CORM (metrics: any of visual_attention_metrics.SCANPATH_DISTANCES;
    the recurrence measures need radius) of predicted scanpaths against human ones, grouped by key as saliency_evaluation groups them:
    gt_fix_vectors[i] belongs to gt_keys[i], predict_fix_vectors[j] to predict_keys[j], a predicted key that gt_keys does not hold
    raises ValueError.  Every (human scanpath of the key, prediction of the key) pair of the whole call is scored in one batch on the
    device.  Returns (means, per_key): per_key[metric] = nanmean over the key's pairs, per_key[metric + "_best"] = mean over the key's
    predictions of the best value over the key's human scanpaths (the smallest distance, the largest REC / DET / LAM; CORM has none),
    float64 [G] in first-appearance order of gt_keys (per_key["keys"]); a key without predictions scores NaN.  means[name] = nanmean
    over the keys, means[name + "_nan"] = how many keys scored NaN.  The ceiling: scanpath_distance_human_evaluation."""
    from .evaltools.visual_attention_metrics import _check_distance_args
    metrics, max_dim, radius, min_line = _check_distance_args(metrics, max_dim, radius, min_line)
    gt_keys, predict_keys, index, _ = _keyed(gt_fix_vectors, gt_keys, predict_fix_vectors, predict_keys)
    paths = [_xy(fv) for fv in gt_fix_vectors] + [_xy(fv) for fv in predict_fix_vectors]
    pairs, owner = _model_pairs(index, gt_keys, predict_keys)
    return _distance_tables(index, paths, pairs, owner, metrics, max_dim, radius, min_line)


def scanpath_distance_human_evaluation(gt_fix_vectors, gt_keys, *, metrics, max_dim=1.0, radius=None, min_line=2):
    """The human ceiling of scanpath_distance_evaluation: every ordered pair of distinct human scanpaths of a key, the first as the
    human side and the second as the "prediction"; a key with one scanpath scores NaN.  Same (means, per_key) result."""
    from .evaltools.visual_attention_metrics import _check_distance_args
    metrics, max_dim, radius, min_line = _check_distance_args(metrics, max_dim, radius, min_line)
    gt_keys, _, index, _ = _keyed(gt_fix_vectors, gt_keys)
    pairs, owner = _ceiling_pairs(index, gt_keys)
    return _distance_tables(index, [_xy(fv) for fv in gt_fix_vectors], pairs, owner, metrics, max_dim, radius, min_line)


# ---- sequence score and fixation edit distance on mean-shift clusters (evaltools/sequence_score.py, csrc/seqscore.hip) -----------------
def _cluster_groups(index, gt_keys, cluster_keys):
    """cluster group of every key: its own, or the one of its cluster key (several keys on one image share the image's clusters)"""
    _, images = _key_index(gt_keys, cluster_keys)
    return np.arange(len(index), dtype=np.int64) if images is None else np.asarray(images, dtype=np.int64)


def sequence_score_evaluation(gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, *, bandwidth, metrics=("SS", "FED"), gap=0.0,
                              max_iter=300, cluster_keys=None):
    """Sequence score (Yang et al. 2020) and fixation edit distance (Mondal et al. 2023) of predicted scanpaths against human ones,
    grouped by key as scanpath_distance_evaluation groups them.  All human fixations of a key are clustered by mean shift with the
    flat kernel of radius bandwidth (required; pixels of the fixations' frame), every scanpath of the key becomes the string of its
    fixations' clusters, SS = Needleman-Wunsch score (0/1 similarity, gap <= 0) / the longer length, FED = Levenshtein distance.
    cluster_keys[i] (optional): the image gt_fix_vectors[i] was recorded on -- keys that share one are clustered together (one key on
    two images raises ValueError).  Clustering, strings and every (human, prediction) pair of the whole call run as one batch on the
    device.  Returns (means, per_key) as scanpath_distance_evaluation: per_key["SS"] / ["FED"] = nanmean over the key's pairs,
    ["SS_best"] = mean over the key's predictions of the largest SS over the key's human scanpaths, ["FED_best"] of the smallest FED;
    a key without predictions scores NaN; means[name + "_nan"] counts the NaN keys.  The ceiling: sequence_score_human_evaluation."""
    from .evaltools.sequence_score import _check_cluster_args, _check_sequence_args, keyed_sequence_scores
    _check_cluster_args(bandwidth, max_iter)
    metrics, gap = _check_sequence_args(metrics, gap)
    gt_keys, predict_keys, index, _ = _keyed(gt_fix_vectors, gt_keys, predict_fix_vectors, predict_keys)
    group_of_key = _cluster_groups(index, gt_keys, cluster_keys)
    paths = [_xy(fv) for fv in gt_fix_vectors] + [_xy(fv) for fv in predict_fix_vectors]
    path_group = np.array([group_of_key[index[k]] for k in gt_keys + predict_keys], dtype=np.int64)
    human_group = np.r_[path_group[:len(gt_keys)], np.full(len(predict_keys), -1, dtype=np.int64)]
    pairs, owner = _model_pairs(index, gt_keys, predict_keys)
    scores = keyed_sequence_scores(paths, path_group, human_group, pairs, int(group_of_key.max()) + 1 if len(index) else 0,
                                   bandwidth=bandwidth, metrics=metrics, gap=gap, max_iter=max_iter)
    return _pair_tables(index, scores, owner, metrics, ("FED",), ("SS",))


def sequence_score_human_evaluation(gt_fix_vectors, gt_keys, *, bandwidth, metrics=("SS", "FED"), gap=0.0, max_iter=300,
                                    cluster_keys=None):
    """The human ceiling of sequence_score_evaluation: every ordered pair of distinct human scanpaths of a key, the first as the human
    side and the second as the "prediction", under the clusters of all human fixations of the key (the "prediction" included, as the
    published evaluation does); a key with one scanpath scores NaN.  Same (means, per_key) result."""
    from .evaltools.sequence_score import _check_cluster_args, _check_sequence_args, keyed_sequence_scores
    _check_cluster_args(bandwidth, max_iter)
    metrics, gap = _check_sequence_args(metrics, gap)
    gt_keys, _, index, _ = _keyed(gt_fix_vectors, gt_keys)
    group_of_key = _cluster_groups(index, gt_keys, cluster_keys)
    path_group = np.array([group_of_key[index[k]] for k in gt_keys], dtype=np.int64)
    pairs, owner = _ceiling_pairs(index, gt_keys)
    scores = keyed_sequence_scores([_xy(fv) for fv in gt_fix_vectors], path_group, path_group, pairs,
                                   int(group_of_key.max()) + 1 if len(index) else 0, bandwidth=bandwidth, metrics=metrics, gap=gap,
                                   max_iter=max_iter)
    return _pair_tables(index, scores, owner, metrics, ("FED",), ("SS",))


# ---- what the model-side calls share: the entries of a batch, and the sum tables that merge batches ------------------------------------
def _head_entries(predict, keys, performances, per_sample=None, outputs=("all_actions_prob",)):
    """The entries of a model-side call on ONE batch and the rows of the model's output they are read against.  Sample i has
    per_sample[i] entries (default: one per subject of performances[i], one without performances), all under the key keys[i].  Without performances every entry of sample i reads row i of the unprefixed
    outputs; with them entry k of sample i reads row i of the "good_" outputs when performances[i][k] is True and row N + i -- the "poor_"
    outputs stacked behind the good ones -- otherwise, as training assigns the heads.  Refuses a predict that lacks one of the outputs
    or does not hold N samples.  Returns (index of _key_index, rows, key_of int64 [entries], the shape of the first output, both);
    both(name) = the output the rows point into: predict[name], or the two heads' stacked."""
    import torch
    N = len(keys)
    names = [h + k for h in (("",) if performances is None else ("good_", "poor_")) for k in outputs]
    missing = [k for k in names if k not in predict]
    if missing:
        raise ValueError(f"predict lacks {missing[0]!r}" + (" (performances given: the two-head outputs are read)" if performances is not None
                                                            else ""))
    if any(predict[k].shape[0] != N for k in names):
        raise ValueError(f"predict holds {predict[names[0]].shape[0]} samples, keys {N}")
    index, _ = _key_index(keys, None)
    rows, key_of = [], []
    for i, n in enumerate(per_sample if per_sample is not None else [1] * N if performances is None else map(len, performances)):
        for k in range(n):
            rows.append(i if performances is None or performances[i][k] == True else N + i)           # noqa: E712  (as the reference)
            key_of.append(index[keys[i]])

    def both(name):
        return predict[name] if performances is None else torch.cat([predict["good_" + name], predict["poor_" + name]], 0)

    return index, rows, np.asarray(key_of, dtype=np.int64), tuple(predict[names[0]].shape), both


class _SumTable:
    """What the tables share.  add(means) sums the entries whose name is in _also or ends in one of _suffixes into parts -- and
    those of means["by_group"][label] into by_group[label]; the first array of a name is copied (as _dtype, where a table sets one), so
    that the caller's is never written to, and where the table has a shape an array of another one is refused.  _divided() = parts with
    every name that has a "_count" as its "_sum" / "_count" (NaN for a count of 0)."""
    _suffixes, _also, _dtype, _shape = (), (), None, None

    def __init__(self):
        self.parts, self.by_group = {}, {}

    def _merge(self, parts, means) -> None:
        for k, v in means.items():
            if k in self._also or k.endswith(self._suffixes):
                if self._shape is not None and isinstance(v, np.ndarray) and v.shape != self._shape:
                    raise ValueError(f"{k} of shape {v.shape}: the table's lattice is {self._shape}")
                parts[k] = parts[k] + v if k in parts else (np.array(v, dtype=self._dtype) if isinstance(v, np.ndarray) else v)

    def add(self, means) -> None:
        self._merge(self.parts, means)
        for label, m in means.get("by_group", {}).items():
            self._merge(self.by_group.setdefault(label, {}), m)

    def _divided(self) -> dict:
        out = dict(self.parts)
        for k in self.parts:
            if k.endswith("_count"):
                total, count = self.parts[k[:-len("_count")] + "_sum"], self.parts[k]
                nan = np.full(total.shape, np.nan) if isinstance(total, np.ndarray) else float("nan")
                out[k[:-len("_count")]] = total / count if count else nan
        return out


# ---- human scanpaths under the model's own step distributions (evaltools/scanpath_likelihood.py, csrc/scanlik.hip) ------
def likelihood_evaluation(predict, fix_vectors, keys, performances=None, image_keys=None, baseline=None, *, uniform_mix,
                          metrics=("LL", "NSS", "AUC"), min_length=0, frame_size=(240, 320), map_shape=None):
    """Per-fixation log-likelihood, information gain, NSS, AUC, duration log-likelihood and length log-probability (metrics: any of
    evaltools.scanpath_likelihood.METRICS) of the human scanpaths of ONE batch under the distributions the model put out for it -- no
    sampling.  predict: the model's eval-mode output on the device; fix_vectors[i]: the list of the subjects' fixation vectors of
    sample i (the reference's evaluation layout), keys[i]: its key (a question id, an image name: any hashable).  With performances
    (AiR: performances[i][k] = subject k of sample i answered correctly) predict["good_all_actions_prob"] / ["good_log_normal_*"]
    score the subjects who answered correctly and the "poor_" outputs the others, as training assigns the heads; without it the
    unprefixed outputs score everybody.  "IG": baseline [NB, P] (evaltools.scanpath_likelihood.cell_baselines) and image_keys[i] = the
    baseline row of sample i's image (default: the only row of a one-row baseline).  uniform_mix is required (0 is allowed);
    min_length: the sampler's, for "STOP".  One launch and one copy back for the whole batch.
    Returns (means, per_key): per_key[m] = the mean over the key's scored fixations ("STOP": over its scanpaths), float64 [G] in
    first-appearance order of keys (per_key["keys"]), NaN for a key without one; means[m] = the mean pooled over all scored fixations
    of the call -- bits per fixation, the convention of the papers -- with means[m + "_sum"] / [m + "_count"] = the sum and number of
    the values it is the mean of (what LikelihoodTable merges), means[m + "_nan"] = the NaN values left out (dropped fixations, NSS on
    a constant map, ...), means[m + "_nan_keys"] = the keys that scored NaN, means["dropped"] = the dropped fixations.  A value of
    -inf is a score, not a gap: it is kept and makes the means -inf."""
    from .evaltools.scanpath_likelihood import _check_args, scanpath_likelihood
    metrics, _, min_length = _check_args(metrics, uniform_mix, min_length)
    keys = list(keys)
    N = len(keys)
    if len(fix_vectors) != N:
        raise ValueError("one key per sample is required")
    if performances is not None and (len(performances) != N or any(len(p) != len(f) for p, f in zip(performances, fix_vectors))):
        raise ValueError("one performance per subject of every sample is required")
    if image_keys is not None and len(image_keys) != N:
        raise ValueError("one image key (baseline row) per sample is required")
    if "IG" in metrics and baseline is not None and image_keys is None:
        if len(baseline) != 1:
            raise ValueError(f"image_keys is required to choose among the {len(baseline)} baseline rows")
        image_keys = [0] * N
    dll = "DLL" in metrics
    subjects = [len(s) for s in fix_vectors]
    index, rows, key_of, (_, T, _), both = _head_entries(predict, keys, performances, subjects, ("all_actions_prob",) + (
        ("log_normal_mu", "log_normal_sigma2") if dll else ()))
    paths = [fv for s in fix_vectors for fv in s]
    brows = [] if image_keys is None else [image_keys[i] for i, n in enumerate(subjects) for _ in range(n)]
    res = scanpath_likelihood(both("all_actions_prob"), paths, rows, frame_size, uniform_mix=uniform_mix, metrics=metrics,
                              map_shape=map_shape, baseline=baseline, baseline_rows=brows if "IG" in metrics else None,
                              log_normal_mu=both("log_normal_mu") if dll else None,
                              log_normal_sigma2=both("log_normal_sigma2") if dll else None, min_length=min_length)
    met = np.arange(T)[None, :] < res["n"][:, None]                          # [S, T]: fixation t met a step
    fixation_key = np.broadcast_to(key_of[:, None], met.shape)[met]
    return _likelihood_tables(index, key_of, res["dropped"], [(m, res[m], key_of) if m == "STOP" else (m, res[m][met], fixation_key)
                                                              for m in metrics])


def _likelihood_tables(index, key_of, dropped, scored):
    """scored: (metric, its values, the key of every value); dropped: per scanpath, key_of its key -> (means, per_key) of the
    likelihood calls: per_key[m] and the pooled means[m] with the entries LikelihoodTable merges"""
    per_key, means = {"keys": list(index)}, {}
    for m, v, owner in scored:
        per_key[m], total, count, n_nan = _pool(v, owner, len(index))
        means.update({m: total / count if count else float("nan"), m + "_sum": total, m + "_count": count, m + "_nan": n_nan,
                      m + "_nan_keys": int(np.isnan(per_key[m]).sum())})
    per_key["dropped"] = np.bincount(key_of, weights=dropped, minlength=len(index)).astype(np.int64)
    means["dropped"] = int(dropped.sum())
    return means, per_key


def likelihood_gold_standard_evaluation(fix_vectors, keys, *, bandwidth, uniform_mix, max_length, same_step=False,
                                        frame_size=(240, 320), map_shape=(30, 40)):
    """The human gold standard of likelihood_evaluation's "LL" (evaltools/scanpath_kde.py, csrc/scankde.hip): every
    fixation of a subject is scored under the kernel density estimate of the OTHER subjects' fixations on the same sample, in bits over
    uniform -- what the people who saw the image tell about where one more of them looks.  fix_vectors[i]: the subjects' fixation
    vectors of sample i, keys[i]: its key, as likelihood_evaluation takes them; each sample is one image.  bandwidth (pixels of the
    frame; kde_bandwidth_search finds it) and uniform_mix have no defaults; max_length is required: the model's T, so that the ceiling
    is pooled over the fixations the model is scored on.  same_step=True keeps only the other subjects' fixation at the same position
    t (leave="scanpath_step"): step t against fixation t, the footing the model is scored on.  A sample with one subject scores NaN.
    Returns (means, per_key) in exactly likelihood_evaluation's format with the one metric "GOLD"; LikelihoodTable merges it."""
    from .evaltools.scanpath_kde import kde_leave_out_likelihood
    keys = list(keys)
    if len(fix_vectors) != len(keys):
        raise ValueError("one key per sample is required")
    if max_length is None:
        raise ValueError("max_length is required: the model's number of decode steps")
    index, _ = _key_index(keys, None)
    paths = [fv for subjects in fix_vectors for fv in subjects]
    sample = np.repeat(np.arange(len(keys), dtype=np.int64), [len(subjects) for subjects in fix_vectors])
    res = kde_leave_out_likelihood(paths, sample, frame_size, map_shape, bandwidth=bandwidth, uniform_mix=uniform_mix,
                                   leave="scanpath_step" if same_step else "scanpath", max_length=max_length)
    key_of = np.array([index[keys[i]] for i in sample], dtype=np.int64)
    met = np.arange(res["LL"].shape[1])[None, :] < res["n"][:, None]             # [S, Tmax]: a fixation that counts
    return _likelihood_tables(index, key_of, res["dropped"], [("GOLD", res["LL"][met], np.broadcast_to(key_of[:, None], met.shape)[met])])


def information_gain_explained(means, gold_means) -> dict:
    """The share of the explainable information a model explains (Kümmerer, Wallis & Bethge 2015): means holds "LL" and "IG" of
    likelihood_evaluation / LikelihoodTable, gold_means "GOLD" of likelihood_gold_standard_evaluation (the same dict when one table
    merged both).  "BASE" = LL - IG, the baseline's bits over uniform; "IG_gold" = GOLD - BASE, the gold standard's information gain
    over the baseline; "IGE" = IG / IG_gold; and the "LL_count" / "IG_count" / "GOLD_count" the three were pooled from (0 for a missing
    one).  NaN where an input is missing, and IGE also where IG_gold is not > 0."""
    nan = float("nan")
    ll, ig, gold = (float(m.get(k, nan)) for m, k in ((means, "LL"), (means, "IG"), (gold_means, "GOLD")))
    base = ll - ig
    ig_gold = gold - base
    return {"BASE": base, "IG_gold": ig_gold, "IGE": ig / ig_gold if ig_gold > 0 else nan, "LL_count": int(means.get("LL_count", 0)),
            "IG_count": int(means.get("IG_count", 0)), "GOLD_count": int(gold_means.get("GOLD_count", 0))}


class LikelihoodTable(_SumTable):
    """The pooled means of likelihood_evaluation over several batches, merged exactly: add(means) sums every metric's "_sum",
    "_count", "_nan" and "_nan_keys" entry and "dropped"; result() = the means dict of all batches as one call would give it (a key
    that appears in two batches counts in each for "_nan_keys")."""
    _suffixes, _also = ("_sum", "_count", "_nan", "_nan_keys"), ("dropped",)

    def result(self) -> dict:
        return self._divided()


# ---- target-search efficiency (evaltools/search_efficiency.py, csrc/scansearch.hip) --------------------------------------
def _boxes_of(index, boxes) -> np.ndarray:
    """float64 [G, 4]: the box of every key, in the index's order; a key without a box is an error, not a silent drop"""
    from .evaltools.search_efficiency import _check_boxes
    missing = [k for k in index if k not in boxes]
    if missing:
        raise ValueError(f"key {missing[0]!r} ({len(missing)} in all) has no box")
    return _check_boxes([boxes[k] for k in index])


def _hit_tables(prefix, res, key_of, G, max_steps):
    """target_hits' result of a set of scanpaths with their keys -> (means, per_key) entries under prefix: the hit curve pooled over the
    scanpaths (numerators "_sum" float64 [max_steps] -- integers, hence exact -- over "_count"), its area, and the mean scanpath ratio
    over the scanpaths that hit"""
    from .evaltools.search_efficiency import tfp_auc
    key_of = np.asarray(key_of, dtype=np.int64)
    hit = res["hit"].astype(np.int64)[:, None]
    reached = ((hit >= 0) & (hit <= np.arange(max_steps)[None, :])).astype(np.float64)       # [S, max_steps]: hit within k + 1 fixations
    curves, total, S, _ = _pool(reached, key_of, G)
    spr, ssum, nspr, _ = _pool(res["SPR"], key_of, G)
    per_key = {prefix + "TFP": curves, prefix + "TFP_AUC": curves.sum(1), prefix + "SPR": spr}
    curve = total / S if S else np.full(max_steps, np.nan)
    means = {prefix + "TFP": curve, prefix + "TFP_sum": total, prefix + "TFP_count": S, prefix + "TFP_AUC": tfp_auc(curve),
             prefix + "SPR": ssum / nspr if nspr else float("nan"), prefix + "SPR_sum": ssum, prefix + "SPR_count": nspr}
    return means, per_key


def search_efficiency_evaluation(gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, boxes, *, max_steps, image_keys=None):
    """Did the scanpaths reach the target, and how fast (Yang et al. 2020; Mondal et al. 2023): the target-fixation probability after
    1 .. max_steps fixations, its area, the scanpath ratio, and the probability mismatch against the human curve, for predicted
    scanpaths and for the human ones, grouped by key as scanpath_distance_evaluation groups them.  boxes: key -> (x_min, y_min, x_max,
    y_max), half-open, in the pixels of the fixations' frame; a key of gt_keys without a box raises ValueError.  image_keys[i]
    (optional): the image of gt_fix_vectors[i] (one key on two images raises ValueError).  max_steps has no default: only the first
    max_steps fixations of a scanpath count.  All scanpaths of the call are scored in one launch (evaltools.search_efficiency.target_hits).
    Returns (means, per_key).  means["TFP"] float64 [max_steps] = the share of ALL predicted scanpaths whose first fixation inside the
    box is among their first k + 1, ["TFP_AUC"] = its sum, ["SPR"] = the mean of |fixation 0 - box centre| / path up to the hit (not
    clipped) over the scanpaths that hit; ["human_TFP"] / ["human_TFP_AUC"] / ["human_SPR"] the same over the human scanpaths; ["PM"] =
    sum_k |TFP_k - human_TFP_k|; and the entries a table needs (SearchEfficiencyTable): [name + "_sum"] / [name + "_count"] = the
    numerator (for a curve: float64 [max_steps] of integer counts) and the number of scanpaths behind each mean.  per_key: "keys" and
    the same names per key in first-appearance order of gt_keys -- curves [G, max_steps], the rest [G]; NaN where a key has no scanpath
    (no hit, for SPR)."""
    from .evaltools.search_efficiency import probability_mismatch, target_hits
    max_steps = check_steps(max_steps)
    gt_keys, predict_keys, index, _ = _keyed(gt_fix_vectors, gt_keys, predict_fix_vectors, predict_keys, image_keys)
    box = _boxes_of(index, boxes)
    key_of = np.array([index[k] for k in gt_keys + predict_keys], dtype=np.int64)
    paths = [_xy(fv) for fv in gt_fix_vectors] + [_xy(fv) for fv in (predict_fix_vectors if predict_fix_vectors is not None else [])]
    res = target_hits(paths, box[key_of], max_steps=max_steps)
    H, G = len(gt_keys), len(index)
    means, per_key = _hit_tables("human_", {k: v[:H] for k, v in res.items()}, key_of[:H], G, max_steps)
    per_key = dict({"keys": list(index)}, **per_key)
    if predict_fix_vectors is not None:
        m, p = _hit_tables("", {k: v[H:] for k, v in res.items()}, key_of[H:], G, max_steps)
        means.update(m, PM=probability_mismatch(m["TFP"], means["human_TFP"]))
        per_key.update(p, PM=np.abs(p["TFP"] - per_key["human_TFP"]).sum(1))
    return means, per_key


def search_efficiency_human_evaluation(gt_fix_vectors, gt_keys, boxes, *, max_steps, image_keys=None):
    """The human row of search_efficiency_evaluation alone: "human_TFP", "human_TFP_AUC", "human_SPR" with their "_sum" / "_count"
    entries; means["human_TFP"] is the human_curve of search_efficiency_model_evaluation and of SearchEfficiencyTable.result."""
    return search_efficiency_evaluation(gt_fix_vectors, None, gt_keys, None, boxes, max_steps=max_steps, image_keys=image_keys)


def search_efficiency_model_evaluation(predict, keys, boxes, *, min_length, max_steps, performances=None, human_curve=None,
                                       frame_size=(240, 320), map_shape=None):
    """The model's own target-fixation probability curve of ONE batch, exactly and without sampling
    (evaltools.search_efficiency.target_hit_probability): predict is the model's eval-mode output on the device, keys[i] the key of sample
    i, boxes: key -> (x_min, y_min, x_max, y_max) in the pixels of frame_size = (height, width); a key without a box raises ValueError.
    With performances (AiR: performances[i][k] = subject k of sample i answered correctly) every subject is one entry, read against
    predict["good_all_actions_prob"] when it answered correctly and ["poor_all_actions_prob"] otherwise, exactly as likelihood_evaluation
    assigns the heads; without it every sample is one entry read against predict["all_actions_prob"].  min_length: the sampler's
    (required; terminate is masked before it).  The curve is the mean over the entries of TFP[:, :max_steps] (a curve of T < max_steps
    steps keeps its last value: the scanpath has ended); an entry whose curve holds a NaN (a step without mass) is left out and counted.
    One launch and one copy back for the batch.
    Returns (means, per_key): means["TFP"] float64 [max_steps], ["TFP_AUC"] its sum, ["PM"] = sum_k |TFP_k - human_curve_k| when
    human_curve is given, ["TFP_sum"] / ["TFP_count"] the sum of the entries' curves and their number (what SearchEfficiencyTable
    merges), ["TFP_nan"] the entries left out, ["empty_boxes"] the entries whose box holds no cell; per_key["TFP"] [G, max_steps], ["TFP_AUC"]
    [G] in first-appearance order of keys (per_key["keys"])."""
    from .evaltools.search_efficiency import probability_mismatch, target_hit_probability, tfp_auc
    max_steps, min_length = check_steps(max_steps), check_min_length(min_length)
    keys = list(keys)
    N = len(keys)
    if performances is not None and len(performances) != N:
        raise ValueError("one list of performances per sample is required")
    if human_curve is not None:
        human_curve = np.asarray(human_curve, dtype=np.float64).reshape(-1)
        if len(human_curve) != max_steps:
            raise ValueError(f"human_curve of {len(human_curve)} steps, max_steps {max_steps}")
    index, rows, key_of, _, both = _head_entries(predict, keys, performances)
    box = _boxes_of(index, boxes)
    res = target_hit_probability(both("all_actions_prob"), box[key_of], rows, frame_size, min_length=min_length, map_shape=map_shape)
    tfp = res["TFP"][:, :max_steps]
    if tfp.shape[1] < max_steps:
        tfp = np.concatenate([tfp, np.repeat(tfp[:, -1:], max_steps - tfp.shape[1], 1)], 1)
    curves, total, count, n_nan = _pool(tfp, key_of, len(index))
    per_key = {"keys": list(index), "TFP": curves, "TFP_AUC": curves.sum(1)}
    curve = total / count if count else np.full(max_steps, np.nan)
    means = {"TFP": curve, "TFP_sum": total, "TFP_count": count, "TFP_nan": n_nan, "TFP_AUC": tfp_auc(curve),
             "empty_boxes": int((res["cells"] == 0).sum())}
    if human_curve is not None:
        means["PM"] = probability_mismatch(curve, human_curve)
    return means, per_key


class SearchEfficiencyTable(_SumTable):
    """The pooled results of the search-efficiency calls over several batches, merged exactly where the numbers are counts: add(means)
    sums every "_sum" (for a curve: its numerators, float64 [max_steps]), "_count" and "_nan" entry and "empty_boxes"; result() = the
    means dict of all batches as one call on their union gives it -- every curve = its summed numerators / its summed count, "_AUC" of
    every curve, "SPR", and "PM" between "TFP" and "human_TFP" (or the human_curve passed to result, for the model's exact curve).  The
    hit curves of scanpaths merge exactly (integer numerators); sums of ratios and of probabilities merge to rounding."""
    _suffixes, _also, _dtype = ("_sum", "_count", "_nan"), ("empty_boxes",), np.float64

    def result(self, human_curve=None) -> dict:
        from .evaltools.search_efficiency import probability_mismatch, tfp_auc
        out = self._divided()
        for m in [m for m, v in out.items() if isinstance(v, np.ndarray) and m + "_count" in self.parts]:      # the curves
            out[m + "_AUC"] = tfp_auc(out[m])
        human = out.get("human_TFP") if human_curve is None else np.asarray(human_curve, dtype=np.float64).reshape(-1)
        if human is not None and "TFP" in out:
            out["PM"] = probability_mismatch(out["TFP"], human)
        return out


# ---- saccade statistics and turning angles: one array per group, counted or expected --------------------------------
def _group_labels(index, groups):
    """groups: key -> label (a task, ...) or None -> (labels in first-appearance order, label index of every key of the index); a key
    without a label is an error, not a silent drop"""
    if groups is None:
        return [], np.zeros(len(index), dtype=np.int64)
    missing = [k for k in index if k not in groups]
    if missing:
        raise ValueError(f"key {missing[0]!r} ({len(missing)} in all) has no group")
    labels = {}
    of_key = np.array([labels.setdefault(groups[k], len(labels)) for k in index], dtype=np.int64).reshape(-1)
    return list(labels), of_key


# a statistic: evaltools.<name>_statistics, the entry names of its array and of what a scanpath or row adds, the expectation's result key
_Statistic = namedtuple("_Statistic", "name array unit expected")
_SACCADES, _TURNS = _Statistic("saccade", "lattice", "saccades", "E"), _Statistic("turn", "table", "pairs", "M")
_RECURRENCE = _Statistic("recurrence", "table", "points", "E")


def _tool(stat, what):
    """evaltools.<name>_statistics.<name>_<what> (counts, expectation, summary, comparison), looked up at the call: a test may replace it"""
    from importlib import import_module
    return getattr(import_module(f"{__package__}.evaltools.{stat.name}_statistics"), f"{stat.name}_{what}")


def _derived(stat, parts, binning, human=None, label=None):
    """the summed entries of the group of label (None: the pooled one) -> the same with "summary" / "human_summary" and the comparison
    numbers against human -- one array (the pooled group's) or a dict label -> array -- else against its own "human_<array>_sum";
    binning: the further arguments of the statistic's summary and comparison"""
    mine, theirs = stat.array + "_sum", "human_" + stat.array + "_sum"
    given = human.get(label) if isinstance(human, dict) else human if label is None else None
    out = dict(parts)
    if theirs in parts:
        out["human_summary"] = _tool(stat, "summary")(parts[theirs], **binning)
    if mine in parts:
        out["summary"] = _tool(stat, "summary")(parts[mine], **binning)
        against = parts.get(theirs) if given is None else given
        if against is not None:
            out.update(_tool(stat, "comparison")(parts[mine], against, **binning))
    return out


def _by_group(entries, labels, groups, label_of) -> dict:
    """entries(i, member mask) -> the means of label i (None, everybody: pooled), under means["by_group"][label] when the call has groups"""
    means = entries(None, np.ones(len(label_of), dtype=bool))
    if groups is not None:
        means["by_group"] = {label: entries(i, label_of == i) for i, label in enumerate(labels)}
    return means


def _scanpath_statistics(stat, gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, groups, image_keys, binning, *args,
                         per_path=None, **kw):
    """(means, per_key) of scanpaths that exist: humans (side 0) and predictions of all groups in ONE counts(paths, side * NL + label,
    2 NL, *args, **kw) launch; args and kw are checked.  per_path (optional): the counts' result -> {name: float64 [S]}, scores of
    every scanpath; per_key[name] / ["human_" + name] = the mean over the key's scanpaths with a value (_pool)"""
    gt_keys, predict_keys, index, _ = _keyed(gt_fix_vectors, gt_keys, predict_fix_vectors, predict_keys, image_keys)
    labels, label_of_key = _group_labels(index, groups)
    NL = max(len(labels), 1)
    key_of = np.array([index[k] for k in gt_keys + predict_keys], dtype=np.int64)
    side = np.r_[np.zeros(len(gt_keys), dtype=np.int64), np.ones(len(predict_keys), dtype=np.int64)]
    path_label = label_of_key[key_of] if len(key_of) else key_of
    paths = [_xy(fv) for fv in gt_fix_vectors] + [_xy(fv) for fv in (predict_fix_vectors if predict_fix_vectors is not None else [])]
    res = _tool(stat, "counts")(paths, side * NL + path_label, 2 * NL, *args, **kw)
    units, drop = res[stat.unit].astype(np.int64), res["dropped"].astype(np.int64)
    sides = (("human_", 0),) + ((("", 1),) if predict_fix_vectors is not None else ())

    def entries(i, member):
        out = {}
        for prefix, s in sides:
            mine = member & (side == s)
            array = res["counts"][s * NL:(s + 1) * NL].sum(0) if i is None else res["counts"][s * NL + i]
            out.update({f"{prefix}{stat.array}_sum": array, f"{prefix}{stat.unit}_sum": int(units[mine].sum()),
                        prefix + "scanpaths_count": int(mine.sum()), prefix + "fixations_dropped": int(drop[mine].sum())})
        return _derived(stat, out, binning)

    per_key = {"keys": list(index)}
    scores = per_path(res) if per_path is not None else {}
    for prefix, s in sides:
        for name, v in ((stat.unit, units), ("dropped", drop)):
            per_key[prefix + name] = np.bincount(key_of[side == s], weights=v[side == s], minlength=len(index)).astype(np.int64)
        for name, v in scores.items():
            per_key[prefix + name] = _pool(v[side == s], key_of[side == s], len(index))[0]
    return _by_group(entries, labels, groups, path_label), per_key


def _model_statistics(stat, predict, keys, performances, groups, map_shape, human, binning, **kw):
    """(means, per_key) of the model's step distributions of ONE batch: one row per entry of _head_entries, ONE expectation(probs, the
    entries' labels, NL, map_shape=map_shape, **kw) call; kw is checked.  binning None: the bare call, no summary and no comparison."""
    keys = list(keys)
    if performances is not None and len(performances) != len(keys):
        raise ValueError("one list of performances per sample is required")
    import torch
    index, rows, key_of, shape, both = _head_entries(predict, keys, performances)
    check_map(int(shape[-1]), map_shape, max_cells=MAX_CELLS)
    labels, label_of_key = _group_labels(index, groups)
    if not len(rows):
        raise ValueError("no entry to evaluate: an empty batch (or no subject in performances)")
    probs = both("all_actions_prob")
    if performances is not None:                               # one row per entry: a head read by k subjects counts k times
        probs = probs.index_select(0, torch.as_tensor(rows, dtype=torch.int64, device=probs.device))
    res = _tool(stat, "expectation")(probs, label_of_key[key_of], max(len(labels), 1), map_shape=map_shape, **kw)
    good, arrays = res["bad"] == 0, res[stat.expected]

    def entries(i, member):
        out = {stat.array + "_sum": sum(arrays[1:], arrays[0].copy()) if i is None else arrays[i],   # ascending label: a fixed order
               stat.unit + "_sum": float(res[stat.unit][member & good].sum()), "rows_count": int((member & good).sum()),
               "rows_bad": int((member & ~good).sum())}
        return out if binning is None else _derived(stat, out, binning, human, None if i is None else labels[i])

    per_key = {"keys": list(index), stat.unit: _pool(np.where(good, res[stat.unit], np.nan), key_of, len(index))[0]}
    return _by_group(entries, labels, groups, label_of_key[key_of]), per_key


class _StatisticsTable(_SumTable):
    """what the two tables share: a table sets _stat, _shape and, where its summary needs arguments, _binning"""
    _suffixes, _binning = ("_sum", "_count", "_bad", "_dropped"), {}

    def _result(self, human) -> dict:
        out = _derived(self._stat, self.parts, self._binning, human)
        if self.by_group:
            out["by_group"] = {label: _derived(self._stat, p, self._binning, human, label) for label, p in self.by_group.items()}
        return out


# ---- saccade statistics (evaltools/saccade_statistics.py, csrc/scansaccade.hip) ------------------------------------------
def saccade_statistics_evaluation(gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, *, frame_size, map_shape, max_steps,
                                  amplitude_edges, n_directions, groups=None, image_keys=None):
    """How the scanpaths move (Le Meur & Liu 2015; Tatler & Vincent 2009): the distribution of saccade amplitudes, of saccade
    directions, their joint distribution on the displacement lattice of the action map and the share of saccades that stay in the same
    cell, for predicted scanpaths and for the human ones, keyed as search_efficiency_evaluation keys them.  frame_size = (height, width)
    of the fixations' frame, map_shape = (Hm, Wm), max_steps (only the first max_steps fixations of a scanpath count), amplitude_edges
    (pixels) and n_directions have no defaults.  groups (optional): key -> label, e.g. a task; image_keys[i] (optional): the image of
    gt_fix_vectors[i] (one key on two images raises ValueError).  Humans and predictions of all groups are counted in ONE launch
    (evaltools.saccade_statistics.saccade_counts).
    Returns (means, per_key).  means["human_lattice_sum"] / ["lattice_sum"] int64 [2 Hm - 1, 2 Wm - 1] (exact), ["human_saccades_sum"] /
    ["saccades_sum"], ["human_scanpaths_count"] / ["scanpaths_count"], ["human_fixations_dropped"] / ["fixations_dropped"] -- what
    SaccadeStatisticsTable merges -- ["human_summary"] / ["summary"] (evaltools.saccade_statistics.saccade_summary) and, against the
    human side, ["JSD_lattice"], ["JSD_amplitude"], ["JSD_direction"] (bits) and ["W1_amplitude"] (pixels).  With groups,
    means["by_group"][label] holds the same entries for the keys of that label.  per_key: "keys" and, per key in first-appearance order
    of gt_keys, the number of saccades counted and of fixations dropped ("human_saccades", "human_dropped", "saccades", "dropped", int64
    [G]) -- no lattice per key."""
    max_steps, map_shape, _ = check_steps(max_steps), check_map_shape(map_shape), check_frame(frame_size)
    binning = dict(frame_size=frame_size, amplitude_edges=check_edges(amplitude_edges), n_directions=check_directions(n_directions))
    return _scanpath_statistics(_SACCADES, gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, groups, image_keys, binning,
                                frame_size, map_shape, max_steps=max_steps)


def saccade_statistics_human_evaluation(gt_fix_vectors, gt_keys, *, frame_size, map_shape, max_steps, amplitude_edges, n_directions,
                                        groups=None, image_keys=None):
    """The human row of saccade_statistics_evaluation alone: the "human_" entries; means["human_lattice_sum"] is the human_lattice of
    saccade_statistics_model_evaluation and of SaccadeStatisticsTable.result."""
    return saccade_statistics_evaluation(gt_fix_vectors, None, gt_keys, None, frame_size=frame_size, map_shape=map_shape,
                                         max_steps=max_steps, amplitude_edges=amplitude_edges, n_directions=n_directions, groups=groups,
                                         image_keys=image_keys)


def saccade_statistics_model_evaluation(predict, keys, *, min_length, max_steps, performances=None, frame_size=(240, 320), map_shape=None,
                                        groups=None, human_lattice=None, amplitude_edges=None, n_directions=None):
    """The model's own saccade statistics of ONE batch, exactly and without sampling
    (evaltools.saccade_statistics.saccade_expectation): predict is the model's eval-mode output on the device, keys[i] the key of sample
    i.  With performances (AiR: performances[i][k] = subject k of sample i answered correctly) every subject is one entry, read against
    predict["good_all_actions_prob"] when it answered correctly and ["poor_all_actions_prob"] otherwise, exactly as
    search_efficiency_model_evaluation assigns the heads; without it every sample is one entry read against
    predict["all_actions_prob"].  min_length (the sampler's) and max_steps are required.  groups (optional): key -> label.  One
    expectation call and one copy back for the batch; an entry whose row is bad (a step without mass) adds nothing and is counted.
    Returns (means, per_key): means["lattice_sum"] float64 [2 Hm - 1, 2 Wm - 1] = the expected saccade counts summed over the entries,
    ["saccades_sum"] its total as the kernel's closed form gives it, ["rows_count"] / ["rows_bad"] the entries that count / were bad --
    what SaccadeStatisticsTable merges; with amplitude_edges and n_directions (the summary cannot be binned without them)
    ["summary"] and, when human_lattice is given, ["JSD_lattice"], ["JSD_amplitude"], ["JSD_direction"], ["W1_amplitude"] against it;
    with groups, means["by_group"][label] the same per label (human_lattice: one lattice for the pooled entries, or a dict label ->
    lattice with the pooled one under None).  per_key: "keys" and "saccades" float64 [G], the expected number of saccades per entry of
    the key (NaN for a key without a good entry)."""
    max_steps, min_length, _ = check_steps(max_steps), check_min_length(min_length), check_frame(frame_size)
    if (amplitude_edges is None) != (n_directions is None):
        raise ValueError("amplitude_edges and n_directions go together: the summary needs both")
    if amplitude_edges is None and human_lattice is not None:
        raise ValueError("human_lattice is compared through the summary: amplitude_edges and n_directions are required with it")
    binning = None if amplitude_edges is None else dict(frame_size=frame_size, amplitude_edges=check_edges(amplitude_edges),
                                                        n_directions=check_directions(n_directions))
    return _model_statistics(_SACCADES, predict, keys, performances, groups, map_shape, human_lattice, binning, min_length=min_length,
                             max_steps=max_steps)


class SaccadeStatisticsTable(_StatisticsTable):
    """The pooled results of the saccade-statistics calls over several batches: add(means) sums every "_sum", "_count", "_bad" and
    "_dropped" entry (also inside "by_group"); result(human_lattice=None) derives the summaries and the four comparison numbers from
    the SUMMED lattices, as one call on the union of the batches gives them.  The comparison is against "human_lattice_sum" when the
    table holds one, else against human_lattice (one lattice for the pooled entries, or a dict label -> lattice with the pooled one
    under None).  Integer lattices (scanpaths that exist) merge exactly; expectations (the model's closed form) are float64 sums and
    merge to rounding: the batches' lattices are added in the order of add, one call adds its rows in row order."""
    _stat = _SACCADES

    def __init__(self, frame_size, map_shape, amplitude_edges, n_directions):
        super().__init__()
        self.frame_size, self.map_shape = check_frame(frame_size), check_map_shape(map_shape)
        self.amplitude_edges, self.n_directions = check_edges(amplitude_edges), check_directions(n_directions)
        self._shape = (2 * self.map_shape[0] - 1, 2 * self.map_shape[1] - 1)
        self._binning = dict(frame_size=self.frame_size, amplitude_edges=self.amplitude_edges, n_directions=self.n_directions)

    def result(self, human_lattice=None) -> dict:
        return self._result(human_lattice)


# ---- turning angles (evaltools/turn_statistics.py, csrc/scanturn.hip) ------------------------------------------------------
def turn_statistics_evaluation(gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, *, frame_size, map_shape, max_steps, n_directions,
                               groups=None, image_keys=None):
    """How the direction of a saccade depends on the direction of the saccade before it (Tatler & Vincent 2009; Le Meur & Liu 2015): the
    direction-transition table and the turning-angle histogram with its forward and its return peak, for predicted scanpaths and for the
    human ones, keyed and grouped as saccade_statistics_evaluation keys and groups them.  frame_size = (height, width), map_shape =
    (Hm, Wm), max_steps and n_directions (at most 16) have no defaults.  Humans and predictions of all groups are counted in ONE launch
    (evaltools.turn_statistics.turn_counts).
    Returns (means, per_key).  means["human_table_sum"] / ["table_sum"] int64 [n + 1, n + 1] (exact; row and column n hold the stays),
    ["human_pairs_sum"] / ["pairs_sum"], ["human_scanpaths_count"] / ["scanpaths_count"], ["human_fixations_dropped"] /
    ["fixations_dropped"] -- what TurnStatisticsTable merges -- ["human_summary"] / ["summary"] (evaltools.turn_statistics.turn_summary)
    and, against the human side, ["JSD_turn"] and ["JSD_transition"] (bits).  With groups, means["by_group"][label] holds the same
    entries for the keys of that label.  per_key: "keys" and, per key in first-appearance order of gt_keys, the number of saccade pairs
    counted and of fixations dropped ("human_pairs", "human_dropped", "pairs", "dropped", int64 [G]) -- no table per key."""
    max_steps, map_shape, _ = check_steps(max_steps), check_map_shape(map_shape), check_frame(frame_size)
    n_directions = check_directions(n_directions, MAX_DIRECTIONS)
    return _scanpath_statistics(_TURNS, gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, groups, image_keys, {},
                                frame_size, map_shape, max_steps=max_steps, n_directions=n_directions)


def turn_statistics_human_evaluation(gt_fix_vectors, gt_keys, *, frame_size, map_shape, max_steps, n_directions, groups=None,
                                     image_keys=None):
    """The human row of turn_statistics_evaluation alone: the "human_" entries; means["human_table_sum"] is the human_table of
    turn_statistics_model_evaluation and of TurnStatisticsTable.result."""
    return turn_statistics_evaluation(gt_fix_vectors, None, gt_keys, None, frame_size=frame_size, map_shape=map_shape, max_steps=max_steps,
                                      n_directions=n_directions, groups=groups, image_keys=image_keys)


def turn_statistics_model_evaluation(predict, keys, *, min_length, max_steps, n_directions, performances=None, frame_size=(240, 320),
                                     map_shape=None, groups=None, human_table=None):
    """The model's own direction-transition table of ONE batch, exactly and without sampling
    (evaltools.turn_statistics.turn_expectation): predict, keys, performances and groups as in saccade_statistics_model_evaluation (the
    heads are assigned per subject in the same way).  min_length (the sampler's), max_steps and n_directions (at most 16) are required;
    frame_size gives the sectors their directions in pixels.  One expectation call and one copy back for the batch; an entry whose row
    is bad (a step without mass) adds nothing and is counted.
    Returns (means, per_key): means["table_sum"] float64 [n + 1, n + 1] = the expected pair counts summed over the entries,
    ["pairs_sum"] its total as the kernel's closed form gives it, ["rows_count"] / ["rows_bad"] the entries that count / were bad --
    what TurnStatisticsTable merges -- ["summary"] and, when human_table is given, ["JSD_turn"] and ["JSD_transition"] against it; with
    groups, means["by_group"][label] the same per label (human_table: one table for the pooled entries, or a dict label -> table with
    the pooled one under None).  per_key: "keys" and "pairs" float64 [G], the expected number of pairs per entry of the key (NaN for a
    key without a good entry)."""
    from .evaltools.turn_statistics import check_table
    max_steps, min_length = check_steps(max_steps), check_min_length(min_length)
    n_directions = check_directions(n_directions, MAX_DIRECTIONS)
    check_frame(frame_size)
    for h in (human_table.values() if isinstance(human_table, dict) else () if human_table is None else (human_table,)):
        if check_table(h).shape != (n_directions + 1, n_directions + 1):
            raise ValueError(f"human_table of shape {np.shape(h)}: [{n_directions + 1}, {n_directions + 1}] is required")
    return _model_statistics(_TURNS, predict, keys, performances, groups, map_shape, human_table, {}, min_length=min_length,
                             max_steps=max_steps, frame_size=frame_size, n_directions=n_directions)


class TurnStatisticsTable(_StatisticsTable):
    """The pooled results of the turn-statistics calls over several batches: add(means) sums every "_sum", "_count", "_bad" and
    "_dropped" entry (also inside "by_group"); result(human_table=None) derives the summaries and the two comparison numbers from the
    SUMMED tables, as one call on the union of the batches gives them.  The comparison is against "human_table_sum" when the table
    holds one, else against human_table (one table for the pooled entries, or a dict label -> table with the pooled one under None).
    Integer tables (scanpaths that exist) merge exactly; expectations (the model's closed form) are float64 sums of non-negative terms
    and merge to rounding: the batches' tables are added in the order of add, one call adds its rows in row order."""
    _stat = _TURNS

    def __init__(self, n_directions):
        super().__init__()
        self.n_directions = check_directions(n_directions, MAX_DIRECTIONS)
        self._shape = (self.n_directions + 1, self.n_directions + 1)

    def result(self, human_table=None) -> dict:
        return self._result(human_table)


# ---- recurrence (evaltools/recurrence_statistics.py, csrc/scanrecur.hip in libscanpaths_amd_stats.so) ----------------------
def _recurrence_scores(res) -> dict:
    """the four measures of every scanpath of a recurrence_counts result, float64 [S] each"""
    from .evaltools.recurrence_statistics import recurrence_measures
    return recurrence_measures(res["rqa"])


def recurrence_statistics_evaluation(gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, *, frame_size, map_shape, max_steps, radius,
                                     min_line, groups=None, image_keys=None):
    """How often a scanpath comes back to a place it has already looked at, and after how many fixations (Anderson et al. 2013, the
    auto-recurrence form on action-map cells; Klein 2000 for the reading by lag): the recurrence table, for predicted scanpaths and for
    the human ones, keyed and grouped as turn_statistics_evaluation keys and groups them.  frame_size = (height, width), map_shape =
    (Hm, Wm), max_steps (at most 64), radius (pixels) and min_line (>= 2) have no defaults.  Humans and predictions of all groups are
    counted in ONE launch (evaltools.recurrence_statistics.recurrence_counts).
    Returns (means, per_key).  means["human_table_sum"] / ["table_sum"] int64 [max_steps, max_steps] (exact; [s, t] recurrent pairs,
    [t, s] pairs, [t, t] fixations), ["human_points_sum"] / ["points_sum"], ["human_scanpaths_count"] / ["scanpaths_count"],
    ["human_fixations_dropped"] / ["fixations_dropped"] -- what RecurrenceStatisticsTable merges -- ["human_summary"] / ["summary"]
    (evaltools.recurrence_statistics.recurrence_summary) and, against the human side, ["REC_difference"], ["L1_by_lag"] and ["JSD_lag"].
    With groups, means["by_group"][label] holds the same entries for the keys of that label.  per_key: "keys" and, per key in
    first-appearance order of gt_keys, the recurrent points counted and the fixations dropped ("human_points", "human_dropped",
    "points", "dropped", int64 [G]) and float64 [G] columns "REC", "DET", "LAM", "CORM" / "human_REC", .. = the mean over the key's
    scanpaths with a defined value (evaltools.recurrence_statistics.recurrence_measures; NaN for a key without one) -- no table per
    key."""
    from .evaltools.recurrence_statistics import check_min_line, check_radius, check_table_steps
    max_steps, map_shape, _ = check_table_steps(max_steps), check_map_shape(map_shape), check_frame(frame_size)
    radius, min_line = check_radius(radius), check_min_line(min_line)
    return _scanpath_statistics(_RECURRENCE, gt_fix_vectors, predict_fix_vectors, gt_keys, predict_keys, groups, image_keys, {},
                                frame_size, map_shape, per_path=_recurrence_scores, max_steps=max_steps, radius=radius, min_line=min_line)


def recurrence_statistics_human_evaluation(gt_fix_vectors, gt_keys, *, frame_size, map_shape, max_steps, radius, min_line, groups=None,
                                           image_keys=None):
    """The human row of recurrence_statistics_evaluation alone: the "human_" entries; means["human_table_sum"] is the human_table of
    recurrence_statistics_model_evaluation and of RecurrenceStatisticsTable.result."""
    return recurrence_statistics_evaluation(gt_fix_vectors, None, gt_keys, None, frame_size=frame_size, map_shape=map_shape,
                                            max_steps=max_steps, radius=radius, min_line=min_line, groups=groups, image_keys=image_keys)


def recurrence_statistics_model_evaluation(predict, keys, *, min_length, max_steps, radius, performances=None, frame_size=(240, 320),
                                           map_shape=None, groups=None, human_table=None):
    """The model's own recurrence table of ONE batch, exactly and without sampling
    (evaltools.recurrence_statistics.recurrence_expectation): predict, keys, performances and groups as in
    turn_statistics_model_evaluation (the heads are assigned per subject in the same way).  min_length (the sampler's), max_steps (at
    most 64) and radius (pixels) are required; frame_size gives the radius its cells.  One expectation call and one copy back for the
    batch; an entry whose row is bad (a step without mass) adds nothing and is counted.  DET and LAM are line statistics without a
    closed form: they come from samples through recurrence_statistics_evaluation.
    Returns (means, per_key): means["table_sum"] float64 [max_steps, max_steps] = the expected counts summed over the entries,
    ["points_sum"] the expected recurrent points as the kernel's closed form gives them, ["rows_count"] / ["rows_bad"] the entries that
    count / were bad -- what RecurrenceStatisticsTable merges -- ["summary"] and, when human_table is given, ["REC_difference"],
    ["L1_by_lag"] and ["JSD_lag"] against it; with groups, means["by_group"][label] the same per label (human_table: one table for the
    pooled entries, or a dict label -> table with the pooled one under None).  per_key: "keys" and "points" float64 [G], the expected
    recurrent points per entry of the key (NaN for a key without a good entry)."""
    from .evaltools.recurrence_statistics import check_radius, check_table, check_table_steps
    max_steps, min_length, radius = check_table_steps(max_steps), check_min_length(min_length), check_radius(radius)
    check_frame(frame_size)
    for h in (human_table.values() if isinstance(human_table, dict) else () if human_table is None else (human_table,)):
        if check_table(h).shape != (max_steps, max_steps):
            raise ValueError(f"human_table of shape {np.shape(h)}: [{max_steps}, {max_steps}] is required")
    return _model_statistics(_RECURRENCE, predict, keys, performances, groups, map_shape, human_table, {}, min_length=min_length,
                             max_steps=max_steps, radius=radius, frame_size=frame_size)


class RecurrenceStatisticsTable(_StatisticsTable):
    """The pooled results of the recurrence-statistics calls over several batches: add(means) sums every "_sum", "_count", "_bad" and
    "_dropped" entry (also inside "by_group"); result(human_table=None) derives the summaries and the three comparison numbers from the
    SUMMED tables, as one call on the union of the batches gives them.  The comparison is against "human_table_sum" when the table
    holds one, else against human_table (one table for the pooled entries, or a dict label -> table with the pooled one under None).
    Integer tables (scanpaths that exist) merge exactly; expectations (the model's closed form) are float64 sums of non-negative terms
    and merge to rounding: the batches' tables are added in the order of add, one call adds its rows in row order."""
    _stat = _RECURRENCE

    def __init__(self, max_steps):
        from .evaltools.recurrence_statistics import check_table_steps
        super().__init__()
        self.max_steps = check_table_steps(max_steps)
        self._shape = (self.max_steps, self.max_steps)

    def result(self, human_table=None) -> dict:
        return self._result(human_table)


# ---- saliency scores of the model's own fixation density, in closed form (evaltools/saliency_maps.py, csrc/scanexpect.hip) --
def saliency_model_evaluation(predict, fix_vectors, keys, performances=None, image_keys=None, *, sigma, min_length, max_steps,
                              pred_weight="count", frame_size=(240, 320), map_shape=None, extra_metrics=(), **kw):
    """saliency_evaluation's scores of ONE batch with the model's side read exactly, without sampling: the predicted map of a key is
    the expected fixation map of the sampler's scanpaths (evaltools.saliency_maps.expected_fixation_maps), what the map of
    prediction="scanpaths" converges to as repeat_num grows.  The batch layout is likelihood_evaluation's: predict = the model's
    eval-mode output on the device, fix_vectors[i] = the list of the subjects' fixation vectors of sample i, the human side of key
    keys[i].  One model row per subject (_head_entries): a head read by k subjects counts k times; with performances the "good_" /
    "poor_" heads are read as training assigns them.  sigma (pixels of the output map), min_length (the sampler's) and max_steps (at
    most 64) have no defaults.  pred_weight "count", or "duration": every step weighs its mean duration
    (evaltools.saliency_maps.expected_durations of log_normal_mu / log_normal_sigma2); "binary" is refused: the binary map of several
    samples is a union, not an expectation.  image_keys[i]: the image of sample i, for "sAUC" and "IG" (whose pools and baselines are
    the OTHER images of THIS call: pass the whole set); extra_metrics and **kw (output_shape, mode, truncate, uniform_mix,
    baseline_sigma) as in saliency_evaluation.  One expectation call and the scoring launches; no sampler call.
    Returns (means, per_key) in saliency_evaluation's shape, so the bootstrap functions read per_key unchanged: means[metric] /
    [metric + "_nan"], and for SaliencyModelTable [metric + "_sum"] / [metric + "_count"] over the keys with a value, ["rows_count"] /
    ["rows_bad"] = the model rows that count / had a step without mass (they add nothing), ["fixations_sum"] = the expected fixations
    of the rows that count; per_key also holds "fixations" float64 [G]: the key's expected fixations per row (NaN without a good row)."""
    from .evaltools.saliency_maps import expected_durations, expected_fixation_maps, scanpath_saliency
    if pred_weight == "binary":
        raise ValueError("pred_weight 'binary' has no closed form here: the binary map of several samples is a union over samples, not "
                         "an expectation; 'count' or 'duration'")
    if pred_weight not in ("count", "duration"):
        raise ValueError(f"pred_weight {pred_weight!r}: 'count' or 'duration'")
    from .evaltools._batch import MAX_FIXATIONS
    min_length, max_steps = check_min_length(min_length), check_steps(max_steps)
    if max_steps > MAX_FIXATIONS:
        raise ValueError(f"max_steps {max_steps}: at most {MAX_FIXATIONS} steps count")
    check_frame(frame_size)
    keys = list(keys)
    N = len(keys)
    if len(fix_vectors) != N:
        raise ValueError("one key per sample is required")
    if performances is not None and (len(performances) != N or any(len(p) != len(f) for p, f in zip(performances, fix_vectors))):
        raise ValueError("one performance per subject of every sample is required")
    if image_keys is not None and len(image_keys) != N:
        raise ValueError("one image key per sample is required")
    if "prediction" in kw or "pred_maps" in kw or "num_groups" in kw:
        raise ValueError("prediction, pred_maps and num_groups are this function's to set")
    duration = pred_weight == "duration"
    subjects = [len(s) for s in fix_vectors]
    index, rows, key_of, _, both = _head_entries(predict, keys, performances, subjects, ("all_actions_prob",) + (
        ("log_normal_mu", "log_normal_sigma2") if duration else ()))
    _, images = _key_index(keys, image_keys)
    if extra_metrics or images is not None:
        kw = dict(kw, extra_metrics=extra_metrics, image_groups=images)
    G = len(index)
    probs = both("all_actions_prob")
    weight = expected_durations(both("log_normal_mu"), both("log_normal_sigma2"))[rows] if duration else None
    import torch
    res = expected_fixation_maps(probs.index_select(0, torch.as_tensor(rows, dtype=torch.int64, device=probs.device)), key_of, max(G, 1),
                                 min_length=min_length, max_steps=max_steps, frame_size=frame_size, output_shape=kw.get("output_shape"),
                                 map_shape=map_shape, step_weight=weight)
    scores = scanpath_saliency([fv for s in fix_vectors for fv in s], key_of, [], [], frame_size, sigma, num_groups=G,
                               prediction="maps", pred_maps=res["maps"][:G], **kw)
    metrics = ("AUC_Judd", "NSS", "KLdiv") + tuple(extra_metrics)
    per_key = {"keys": list(index)}
    per_key.update({k: v.cpu().numpy() for k, v in scores.items()})
    good = res["bad"] == 0
    n_good = np.bincount(key_of[good], minlength=G)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_key["fixations"] = np.where(n_good > 0, np.bincount(key_of[good], weights=res["fixations"][good], minlength=G)
                                        / np.maximum(n_good, 1), np.nan)
    means = _key_means(per_key, metrics)
    for m in metrics:
        ok = ~np.isnan(per_key[m])
        means[m + "_sum"], means[m + "_count"] = float(per_key[m][ok].sum()), int(ok.sum())
    means.update({"rows_count": int(good.sum()), "rows_bad": int((~good).sum()), "fixations_sum": float(res["fixations"][good].sum())})
    return means, per_key


class SaliencyModelTable(_SumTable):
    """The means of saliency_model_evaluation over several batches: add(means) sums every "_sum", "_count", "_nan" and "_bad" entry;
    result()[metric] = the metric's sum / count over all keys of all batches -- the mean over keys that one call on their union gives
    for the metrics that need no other image (a key that appears in two batches counts in each) -- and result()["fixations_per_row"]
    = "fixations_sum" / "rows_count"."""
    _suffixes = ("_sum", "_count", "_nan", "_bad")

    def result(self) -> dict:
        out, nan = dict(self.parts), float("nan")
        for k, count in self.parts.items():
            if k.endswith("_count") and k[:-len("_count")] + "_sum" in self.parts:
                out[k[:-len("_count")]] = self.parts[k[:-len("_count")] + "_sum"] / count if count else nan
        if "rows_count" in out:
            out["fixations_per_row"] = out["fixations_sum"] / out["rows_count"] if out["rows_count"] else nan
        return out


# ---- bootstrap intervals and paired comparisons for every keyed table (evaltools/bootstrap.py, csrc/scanboot.hip) ----------
def _score_names(per_key) -> list:
    """every float64 [G] entry of a per_key table (of the first one of a sequence)"""
    t = per_key if isinstance(per_key, dict) else list(per_key)[0]
    G = len(t["keys"])
    return [k for k, v in t.items() if k != "keys" and isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape == (G,)]


def _level_quantiles(level) -> Tuple[float, float]:
    """the two tail probabilities of a central interval, rounded to 12 decimals so that level = 0.95 gives 0.025 and not the
    0.025000000000000022 of (1 - 0.95) / 2, which would move the order statistic by one whenever 0.025 * n_valid is an integer"""
    if isinstance(level, bool) or not isinstance(level, (int, float)) or not 0.0 < level < 1.0:
        raise ValueError(f"level {level!r}: a number inside (0, 1) is required")
    lo = float(np.round((1.0 - level) / 2.0, 12))
    return lo, float(np.round(1.0 - lo, 12))


def _match_rows(keys_a, keys_b) -> np.ndarray:
    """the row of the second table for every row of the first: the t-th row of a key pairs with the t-th row of that key; a key (or an
    occurrence of it) that one table lacks raises ValueError naming it"""
    rows, seen, out = {}, {}, []
    for r, k in enumerate(keys_b):
        rows.setdefault(k, []).append(r)
    for k in keys_a:
        t = seen.get(k, 0)
        seen[k] = t + 1
        if t >= len(rows.get(k, ())):
            raise ValueError(f"key {k!r} of the first table is missing in the second: the two tables must hold the same keys")
        out.append(rows[k][t])
    extra = [k for k in rows if len(rows[k]) != seen.get(k, 0)]
    if extra:
        raise ValueError(f"key {extra[0]!r} of the second table is missing in the first: the two tables must hold the same keys")
    return np.array(out, dtype=np.int64)


def _interval(res, s) -> dict:
    return {"estimate": float(res["estimate"][s]), "se": float(res["se"][s]), "lo": float(res["quantiles"][s, 0]),
            "hi": float(res["quantiles"][s, 1]), "n_valid": int(res["n_valid"][s])}


def bootstrap_evaluation(per_key, *, names=None, cluster_keys=None, replicates, seed, level=0.95) -> dict:
    """Standard error and percentile interval of the mean over keys of a keyed evaluation's per_key table (or a sequence of them from
    several batches), by a cluster bootstrap on the device (evaltools.bootstrap.bootstrap_ratio).  names: the entries to
    bootstrap (default: every float64 [G] entry); cluster_keys: the image of every key -- a list aligned with per_key["keys"] or a
    mapping key -> image; the resampling unit is the image, because several keys of one image (AiR's questions, any dataset's
    subjects) are not independent draws.  None: every key is its own cluster.  replicates and seed have no defaults; level: the
    coverage of the central percentile interval.
    Returns {name: {"estimate", "se", "lo", "hi", "n_valid"}}: "estimate" is the nanmean over keys exactly as the family's own
    means[name] computes it (on the host, by the same expression, so the two are equal to the bit; the kernel's own point estimate adds
    in another order and may differ in the last place); "se" the standard deviation of the valid replicates; "lo" / "hi" their order
    statistics at (1 - level) / 2 and 1 - (1 - level) / 2; "n_valid" how many replicates were not NaN.
    THE LIKELIHOOD FAMILY'S means[name] is pooled over fixations, not a mean over keys: this function gives the interval of the mean
    over keys of per_key[name]; for the pooled mean call bootstrap_ratio with num = the key's sum and den = the key's count."""
    from .evaltools.bootstrap import bootstrap_ratio, key_clusters, table_columns
    names = _score_names(per_key) if names is None else list(names)
    if not names:
        raise ValueError("no entry to bootstrap: names is empty")
    q = _level_quantiles(level)
    num, den, keys = table_columns(per_key, names)
    res = bootstrap_ratio(num, den, key_clusters(keys, cluster_keys), None, replicates=replicates, seed=seed, quantiles=q)
    out = {}
    for s, name in enumerate(names):
        out[name] = _interval(res, s)
        out[name]["estimate"] = _nanmean(np.where(den[:, s] > 0, num[:, s], np.nan))[0]
    return out


def bootstrap_comparison(per_key_a, per_key_b, *, names=None, cluster_keys=None, replicates, seed, level=0.95) -> dict:
    """Paired comparison of two models scored on the same keys: the tables (or sequences of tables) are matched by key -- differing key
    sets raise ValueError naming a missing key -- and every replicate resamples the same images for both, so the between-image
    variance cancels in the difference.  A key that is NaN in either table is left out of both for that name: the difference is paired
    on the common keys.  cluster_keys (a list aligned with per_key_a["keys"] or a mapping), replicates, seed, level: bootstrap_evaluation.
    Returns {name: {"a", "b", "difference" (a - b on the common keys, the kernel's point estimates), "se", "lo", "hi" (of the
    difference), "p", "n_valid"}}; "p" = min(1, 2 (min(n_le0, n_ge0) + 1) / (n_valid + 1)): the two-sided bootstrap p-value of "no
    difference", from the integer counts of replicates <= 0 and >= 0."""
    from .evaltools.bootstrap import bootstrap_ratio, key_clusters, table_columns
    names = [n for n in _score_names(per_key_a) if n in _score_names(per_key_b)] if names is None else list(names)
    if not names:
        raise ValueError("no entry to compare: names is empty")
    q = _level_quantiles(level)
    na, da, keys = table_columns(per_key_a, names)
    nb, db, keys_b = table_columns(per_key_b, names)
    rows = _match_rows(keys, keys_b)
    both = (da > 0) & (db[rows] > 0)
    n = len(names)
    num, den = np.zeros((len(keys), 2 * n)), np.zeros((len(keys), 2 * n))
    num[:, 0::2], num[:, 1::2] = np.where(both, na, 0.0), np.where(both, nb[rows], 0.0)
    den[:, 0::2] = den[:, 1::2] = both
    con = [c for s in range(n) for c in ((2 * s, -1, -1, -1), (2 * s + 1, -1, -1, -1), (2 * s, 2 * s + 1, -1, -1))]
    res = bootstrap_ratio(num, den, key_clusters(keys, cluster_keys), con, replicates=replicates, seed=seed, quantiles=q)
    out = {}
    for s, name in enumerate(names):
        d = _interval(res, 3 * s + 2)
        tail = min(int(res["n_le0"][3 * s + 2]), int(res["n_ge0"][3 * s + 2]))
        out[name] = {"a": float(res["estimate"][3 * s]), "b": float(res["estimate"][3 * s + 1]), "difference": d["estimate"],
                     "se": d["se"], "lo": d["lo"], "hi": d["hi"], "p": min(1.0, 2.0 * (tail + 1) / (d["n_valid"] + 1)),
                     "n_valid": d["n_valid"]}
    return out


def bootstrap_information_gain_explained(per_key, gold_per_key, *, cluster_keys=None, replicates, seed, level=0.95) -> dict:
    """The interval of information_gain_explained on key means: per_key holds "LL" and "IG" of likelihood_evaluation, gold_per_key
    "GOLD" of likelihood_gold_standard_evaluation (matched by key; the same table when one holds all three).  BASE = LL - IG is built
    per key on the host, so that it stays a linear column, and IGE = IG / (GOLD - BASE) is ONE contrast of the three column means: its
    replicates are ratios of differences on the same resampled images.  A key that is NaN in any of the three (a -inf in both LL and
    IG makes BASE NaN) is left out of all of them.  Returns {"IGE", "IG_gold", "BASE"}, each {"estimate", "se", "lo", "hi", "n_valid"}
    (the kernel's point estimates: means over keys, where information_gain_explained on pooled means weighs fixations)."""
    from .evaltools.bootstrap import bootstrap_ratio, key_clusters, table_columns
    q = _level_quantiles(level)
    nm, dm, keys = table_columns(per_key, ["LL", "IG"])
    ng, dg, keys_g = table_columns(gold_per_key, ["GOLD"])
    rows = _match_rows(keys, keys_g)
    with np.errstate(invalid="ignore"):
        value = np.stack([nm[:, 1], ng[rows, 0], nm[:, 0] - nm[:, 1]], 1)                  # IG, GOLD, BASE
    ok = (dm[:, 0] > 0) & (dm[:, 1] > 0) & (dg[rows, 0] > 0) & ~np.isnan(value).any(1)
    num = np.where(ok[:, None], value, 0.0)
    den = np.repeat(ok[:, None].astype(np.float64), 3, 1)
    con = [(0, -1, 1, 2), (1, 2, -1, -1), (2, -1, -1, -1)]
    res = bootstrap_ratio(num, den, key_clusters(keys, cluster_keys), con, replicates=replicates, seed=seed, quantiles=q)
    return {name: _interval(res, s) for s, name in enumerate(("IGE", "IG_gold", "BASE"))}
