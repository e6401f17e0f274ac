"""The reference's test / validation loop (AiR/test.py:111-197, AiR/train.py:382-450) on the device.

Per batch: ONE eval-mode forward, then ``repeat_num`` x (good head, poor head) sampled scanpaths -- 2 * repeat_num
``random_sample`` + scan launches that stay on the device -- and ONE device->host copy of all fixation vectors of the batch
(the reference does 2 * repeat_num * N * T ``.cpu().numpy()`` calls, models/sampling.py:55-72).  The lists handed to
``evaluation_performance_related`` and the ``predict_results`` records have the reference's order and content:
for every trial the N good-head scanpaths (allocated performance True) followed by the N poor-head ones (False)."""
from __future__ import annotations

from typing import Dict, Iterable, List, Tuple

import numpy as np
import torch

_FV = {"names": ("start_x", "start_y", "duration"), "formats": ("f8", "f8", "f8")}


def sample_batch(predict: Dict[str, torch.Tensor], sampling, repeat_num: int, heads=("good", "poor")):
    """-> fix [repeat, len(heads), N, T, 3] float32 and nfix [repeat, len(heads), N] int32, still on the device"""
    fixs, nfs = [], []
    for _ in range(repeat_num):
        for head in heads:
            pre = head + "_" if head else ""
            s = sampling.random_sample(predict[pre + "all_actions_prob"], predict[pre + "log_normal_mu"],
                                       predict[pre + "log_normal_sigma2"])
            _, _, _, fix, nfix = sampling._scan(s["selected_actions"], s["durations"])
            fixs.append(fix)
            nfs.append(nfix)
    N, T = fixs[0].shape[0], fixs[0].shape[1]
    return torch.stack(fixs).view(repeat_num, len(heads), N, T, 3), torch.stack(nfs).view(repeat_num, len(heads), N)


def to_fix_vectors(fix_h: np.ndarray, n_h: np.ndarray) -> List[np.ndarray]:
    out = []
    for b in range(fix_h.shape[0]):
        fv = np.zeros(int(n_h[b]), dtype=_FV)
        fv["start_x"], fv["start_y"], fv["duration"] = fix_h[b, :n_h[b], 0], fix_h[b, :n_h[b], 1], fix_h[b, :n_h[b], 2]
        out.append(fv)
    return out


def _forward_batches(model, loader, ablate_attention_info: bool, with_tasks: bool):
    """what every loop below does per batch: images and attention maps to the device, the maps zeroed for the ablation, ONE eval-mode
    forward -- with batch["tasks"] (the COCO-Search18 signature) when with_tasks and the batch has them -- -> (batch, predict)"""
    model.eval()
    for batch in loader:
        images, attention_maps = batch["images"].cuda(), batch["attention_maps"].cuda()
        if ablate_attention_info:
            attention_maps = attention_maps * 0
        tasks = (batch["tasks"].cuda(),) if with_tasks and "tasks" in batch else ()
        yield batch, model(images, attention_maps, *tasks)


def _performances(batch, predict):
    """the batch's performances when the model has the two AiR heads, else None"""
    return batch["performances"] if "good_all_actions_prob" in predict else None


@torch.no_grad()
def run_test_loop(model, sampling, loader: Iterable[dict], repeat_num: int = 10, ablate_attention_info: bool = False,
                  multimatch=None) -> Tuple[dict, dict, list, list]:
    """loader yields the reference's evaluation batches: images, fix_vectors, performances, attention_maps, question_ids,
    img_names (AiR/test.py:119-123).  Returns (cur_metrics, cur_metrics_std, scores_of_each_images, predict_results)."""
    from .utils.evaluation import evaluation_performance_related
    all_gt, all_pred, all_perf, all_alloc, predict_results = [], [], [], [], []
    for batch, predict in _forward_batches(model, loader, ablate_attention_info, with_tasks=False):
        gt_fix_vectors, performances = batch["fix_vectors"], batch["performances"]
        N = batch["images"].shape[0]
        fix, nfix = sample_batch(predict, sampling, repeat_num)
        fix_h, n_h = fix.cpu().numpy().astype(np.float64), nfix.cpu().numpy()          # the batch's single device->host copy
        for trial in range(repeat_num):
            for hi, allocated in enumerate((True, False)):
                fvs = to_fix_vectors(fix_h[trial, hi], n_h[trial, hi])
                all_gt.extend(gt_fix_vectors)
                all_perf.extend(performances)
                all_alloc.extend([allocated] * N)
                all_pred.extend(fvs)
                for index in range(N):
                    arr = np.array(fvs[index].tolist()).reshape(-1, 3)
                    predict_results.append({"img_names": batch["img_names"][index], "qid": batch["question_ids"][index],
                                            "repeat_id": trial + 1, "performance": allocated, "X": list(arr[:, 0]),
                                            "Y": list(arr[:, 1]), "T": list(arr[:, 2] * 1000), "length": len(arr)})
    cur_metrics, cur_metrics_std, scores = evaluation_performance_related(all_gt, all_pred, all_perf, all_alloc, multimatch)
    return cur_metrics, cur_metrics_std, scores, predict_results


@torch.no_grad()
def run_likelihood_loop(model, loader: Iterable[dict], *, uniform_mix, metrics=("LL", "NSS", "AUC"), min_length=0, baseline=None,
                        ablate_attention_info: bool = False, frame_size=(240, 320), map_shape=None) -> Tuple[dict, List[dict]]:
    """The loop of run_test_loop without sampling: the human scanpaths of every batch are scored under the distributions the model
    puts out for it (utils.evaluation.likelihood_evaluation) -- per batch ONE eval-mode forward, ONE sp_scan_likelihood launch and ONE
    small device->host copy (the scores; the distributions stay on the device).  loader yields run_test_loop's batches; "performances"
    is read when the model has the two AiR heads ("good_all_actions_prob" in its output), and with a baseline of more than one row
    "baseline_rows" names the row of every sample's image.  The key of a sample is its question id.
    Returns (means, per_key of every batch): means = the batches' pooled means merged by utils.evaluation.LikelihoodTable.
    With the human gold standard next to it: run_likelihood_gold_loop."""
    return _likelihood_loop(model, loader, None, uniform_mix=uniform_mix, metrics=metrics, min_length=min_length, baseline=baseline,
                            ablate_attention_info=ablate_attention_info, frame_size=frame_size, map_shape=map_shape)


@torch.no_grad()
def run_likelihood_gold_loop(model, loader: Iterable[dict], *, gold_standard, uniform_mix, metrics=("LL", "NSS", "AUC"), min_length=0,
                             baseline=None, ablate_attention_info: bool = False, frame_size=(240, 320), map_shape=None
                             ) -> Tuple[dict, List[dict]]:
    """run_likelihood_loop with the ceiling: gold_standard is None (then this IS run_likelihood_loop) or a dict of the keywords of
    utils.evaluation.likelihood_gold_standard_evaluation (bandwidth, uniform_mix, max_length[, same_step, map_shape]; frame_size
    defaults to this call's).  Every batch is then also scored by it; its "GOLD" entries join the same LikelihoodTable and the batch's
    per_key ("dropped" stays the likelihood scorer's: the same fixations are not counted twice), so that
    utils.evaluation.information_gain_explained(means, means) reads the explained share off the returned means."""
    return _likelihood_loop(model, loader, gold_standard, uniform_mix=uniform_mix, metrics=metrics, min_length=min_length,
                            baseline=baseline, ablate_attention_info=ablate_attention_info, frame_size=frame_size, map_shape=map_shape)


def _likelihood_loop(model, loader, gold_standard, *, uniform_mix, metrics, min_length, baseline, ablate_attention_info, frame_size,
                     map_shape):
    from .utils.evaluation import LikelihoodTable, likelihood_evaluation, likelihood_gold_standard_evaluation
    table, per_batch = LikelihoodTable(), []
    for batch, predict in _forward_batches(model, loader, ablate_attention_info, with_tasks=False):
        means, per_key = likelihood_evaluation(predict, batch["fix_vectors"], batch["question_ids"], _performances(batch, predict),
                                               batch.get("baseline_rows"), baseline, uniform_mix=uniform_mix, metrics=metrics,
                                               min_length=min_length, frame_size=frame_size, map_shape=map_shape)
        table.add(means)
        if gold_standard is not None:
            gold, gold_keys = likelihood_gold_standard_evaluation(batch["fix_vectors"], batch["question_ids"],
                                                                  **dict({"frame_size": frame_size}, **gold_standard))
            table.add({k: v for k, v in gold.items() if k != "dropped"})
            per_key["GOLD"] = gold_keys["GOLD"]
        per_batch.append(per_key)
    return table.result(), per_batch


@torch.no_grad()
def run_search_efficiency_loop(model, loader: Iterable[dict], *, boxes, min_length, max_steps, human_curve=None,
                               ablate_attention_info: bool = False, frame_size=(240, 320), map_shape=None) -> Tuple[dict, List[dict]]:
    """The model's own target-fixation probability curve over a loader, exactly and without sampling
    (utils.evaluation.search_efficiency_model_evaluation): per batch ONE eval-mode forward, ONE sp_scan_target_mass launch and ONE small
    device->host copy (the curves; the distributions stay on the device).  loader yields run_test_loop's batches; "tasks" is passed to the
    model when the batch has it (the COCO-Search18 signature), "performances" is read when the model has the two AiR heads
    ("good_all_actions_prob" in its output).  The key of a sample is its question id; boxes: key -> (x_min, y_min, x_max, y_max) in the
    pixels of frame_size.  min_length is the sampler's and has no default; human_curve (optional, [max_steps]): for "PM".
    Returns (means, per_key of every batch): means = the batches merged by utils.evaluation.SearchEfficiencyTable."""
    from .utils.evaluation import SearchEfficiencyTable, search_efficiency_model_evaluation
    table, per_batch = SearchEfficiencyTable(), []
    for batch, predict in _forward_batches(model, loader, ablate_attention_info, with_tasks=True):
        means, per_key = search_efficiency_model_evaluation(
            predict, batch["question_ids"], boxes, min_length=min_length, max_steps=max_steps,
            performances=_performances(batch, predict), frame_size=frame_size, map_shape=map_shape)
        table.add(means)
        per_batch.append(per_key)
    return table.result(human_curve), per_batch


@torch.no_grad()
def run_saccade_statistics_loop(model, loader: Iterable[dict], *, min_length, max_steps, amplitude_edges, n_directions, human_lattice=None,
                                ablate_attention_info: bool = False, frame_size=(240, 320), map_shape=None) -> Tuple[dict, List[dict]]:
    """The model's own saccade statistics over a loader, exactly and without sampling
    (utils.evaluation.saccade_statistics_model_evaluation): per batch ONE eval-mode forward, ONE sp_scan_saccade_expectation call and ONE
    small device->host copy (the batch's lattice; the distributions stay on the device).  loader yields run_test_loop's batches; "tasks" is
    passed to the model when the batch has it, "performances" is read when the model has the two AiR heads ("good_all_actions_prob" in
    its output).  The key of a sample is its question id.  min_length is the sampler's; it, max_steps, amplitude_edges (pixels) and
    n_directions have no defaults; human_lattice (optional, utils.evaluation.saccade_statistics_human_evaluation's
    "human_lattice_sum"): for the four comparison numbers.  map_shape defaults to (30, 40) for 1201 actions only.
    Returns (means, per_key of every batch): means = the batches merged by utils.evaluation.SaccadeStatisticsTable."""
    from .utils.evaltools._args import check_directions, check_edges
    from .utils.evaluation import SaccadeStatisticsTable, saccade_statistics_model_evaluation
    amplitude_edges, n_directions = check_edges(amplitude_edges), check_directions(n_directions)

    def table(means):                                           # sized from the first batch's lattice
        LH, LW = means["lattice_sum"].shape
        return SaccadeStatisticsTable(frame_size, ((LH + 1) // 2, (LW + 1) // 2), amplitude_edges, n_directions)

    return _statistics_loop(model, loader, ablate_attention_info, table, human_lattice, saccade_statistics_model_evaluation,
                            min_length=min_length, max_steps=max_steps, frame_size=frame_size, map_shape=map_shape)


@torch.no_grad()
def run_turn_statistics_loop(model, loader: Iterable[dict], *, min_length, max_steps, n_directions, human_table=None,
                             ablate_attention_info: bool = False, frame_size=(240, 320), map_shape=None) -> Tuple[dict, List[dict]]:
    """The model's own direction-transition table over a loader, exactly and without sampling
    (utils.evaluation.turn_statistics_model_evaluation): per batch ONE eval-mode forward, ONE sp_scan_turn_expectation call and ONE small
    device->host copy (the batch's table; the distributions stay on the device).  loader, "tasks", "performances" and the keys as in
    run_saccade_statistics_loop.  min_length is the sampler's; it, max_steps and n_directions (at most 16) have no defaults;
    human_table (optional, utils.evaluation.turn_statistics_human_evaluation's "human_table_sum"): for "JSD_turn" and "JSD_transition".
    map_shape defaults to (30, 40) for 1201 actions only.
    Returns (means, per_key of every batch): means = the batches merged by utils.evaluation.TurnStatisticsTable."""
    from .utils.evaluation import TurnStatisticsTable, turn_statistics_model_evaluation
    table = TurnStatisticsTable(n_directions)
    return _statistics_loop(model, loader, ablate_attention_info, lambda means: table, human_table, turn_statistics_model_evaluation,
                            min_length=min_length, max_steps=max_steps, n_directions=n_directions, frame_size=frame_size,
                            map_shape=map_shape)


@torch.no_grad()
def run_recurrence_statistics_loop(model, loader: Iterable[dict], *, min_length, max_steps, radius, human_table=None,
                                   ablate_attention_info: bool = False, frame_size=(240, 320), map_shape=None) -> Tuple[dict, List[dict]]:
    """The model's own recurrence table over a loader, exactly and without sampling
    (utils.evaluation.recurrence_statistics_model_evaluation): per batch ONE eval-mode forward, ONE sp_stats_recurrence_expectation call
    and ONE small device->host copy (the batch's table; the distributions stay on the device).  loader, "tasks", "performances" and the
    keys as in run_saccade_statistics_loop.  min_length is the sampler's; it, max_steps (at most 64) and radius (pixels) have no
    defaults; human_table (optional, utils.evaluation.recurrence_statistics_human_evaluation's "human_table_sum"): for
    "REC_difference", "L1_by_lag" and "JSD_lag".  map_shape defaults to (30, 40) for 1201 actions only.
    Returns (means, per_key of every batch): means = the batches merged by utils.evaluation.RecurrenceStatisticsTable."""
    from .utils.evaluation import RecurrenceStatisticsTable, recurrence_statistics_model_evaluation
    table = RecurrenceStatisticsTable(max_steps)
    return _statistics_loop(model, loader, ablate_attention_info, lambda means: table, human_table, recurrence_statistics_model_evaluation,
                            min_length=min_length, max_steps=max_steps, radius=radius, frame_size=frame_size, map_shape=map_shape)


@torch.no_grad()
def run_saliency_loop(model, loader: Iterable[dict], *, sigma, min_length, max_steps, pred_weight="count", extra_metrics=(),
                      ablate_attention_info: bool = False, frame_size=(240, 320), map_shape=None, **kw) -> Tuple[dict, List[dict]]:
    """The saliency scores (AUC_Judd, NSS, KLdiv and the extras "CC", "SIM") of the model's own fixation density over a loader, exactly
    and without sampling (utils.evaluation.saliency_model_evaluation): per batch ONE eval-mode forward, ONE
    sp_model_fixation_expectation call and the scoring launches -- no sampler call, no scanpath upload for the model's side.  loader
    yields run_test_loop's batches: "fix_vectors" is the human side, the key of a sample is its question id, "tasks" is passed to the
    model when the batch has it, "performances" is read when the model has the two AiR heads.  sigma (pixels), min_length (the
    sampler's) and max_steps (at most 64) have no defaults; pred_weight "count" or "duration"; **kw goes on (output_shape, mode,
    truncate).  "sAUC" and "IG" need fixations from OTHER images and a batch is not the dataset: they are refused here -- call
    utils.evaluation.saliency_model_evaluation once over the whole set for them.
    Returns (means, per_key of every batch): means = the batches merged by utils.evaluation.SaliencyModelTable."""
    from .utils.evaluation import SaliencyModelTable, saliency_model_evaluation
    other_images = [m for m in extra_metrics if m in ("sAUC", "IG")]
    if other_images:
        raise ValueError(f"extra_metrics {other_images}: the shuffled AUC's negatives and the information gain's baseline come from the "
                         "OTHER images, and a batch is not the dataset; call utils.evaluation.saliency_model_evaluation over the whole "
                         "set")
    table, per_batch = SaliencyModelTable(), []
    for batch, predict in _forward_batches(model, loader, ablate_attention_info, with_tasks=True):
        means, per_key = saliency_model_evaluation(predict, batch["fix_vectors"], batch["question_ids"], _performances(batch, predict),
                                                   sigma=sigma, min_length=min_length, max_steps=max_steps, pred_weight=pred_weight,
                                                   frame_size=frame_size, map_shape=map_shape, extra_metrics=extra_metrics, **kw)
        table.add(means)
        per_batch.append(per_key)
    if not per_batch:
        raise ValueError("the loader yielded no batch")
    return table.result(), per_batch


def _statistics_loop(model, loader, ablate_attention_info, make_table, human, evaluate, **kw):
    """the loops above: evaluate(predict, keys, performances=..., **kw) per batch, merged by make_table(the first batch's means)
    and read against human; a loader without a batch is an error"""
    table, per_batch = None, []
    for batch, predict in _forward_batches(model, loader, ablate_attention_info, with_tasks=True):
        means, per_key = evaluate(predict, batch["question_ids"], performances=_performances(batch, predict), **kw)
        table = make_table(means) if table is None else table
        table.add(means)
        per_batch.append(per_key)
    if table is None:
        raise ValueError("the loader yielded no batch")
    return table.result(human), per_batch
