"""The cases of tests/test_keyed_tables_cpu.py and of its recording script tests/golden/make_golden_keyed_tables.py: deterministic
stand-ins for the eight device entry points under the keyed evaluation calls, the inputs, and the calls themselves.  No device and no
library is touched.  Every value a stand-in returns is a dyadic rational (an integer / 1024) drawn from a generator seeded by the
call's own arguments, so every sum the host code forms is exact in float64 and independent of the order of summation, and a stand-in
gives the same answer wherever in a run it is called.  Values read from the call's probability rows are mixed in, so that the row an
entry is scored against shows in the result.  NaN and -inf are planted on purpose (see each stand-in)."""
import zlib

import numpy as np
import torch

N, T, MAP, FRAME = 3, 4, (3, 5), (24, 40)
A = 1 + MAP[0] * MAP[1]
LATTICE = (2 * MAP[0] - 1, 2 * MAP[1] - 1)
KEYS = ["a", "b", "a"]                                           # a repeated key
LENGTHS = [[3, 6], [2], [4, 1, 5, 4]]                            # 1 to 4 subjects per sample; n < T, n == T and n > T
PERFORMANCES = [[True, False], [False], [True, True, False, True]]
ENTRIES = [[True, False], [], [False, True, True]]               # the model-side calls: any number of entries, one sample without
METRICS = ("LL", "IG", "NSS", "AUC", "DLL", "STOP")
EDGES, DIRECTIONS = [0.0, 8.0, 16.0, 64.0], 4
GROUPS = {"a": "find", "b": "count", "c": "find", "d": "count"}
BOXES = {"a": [0.0, 0.0, 8.0, 8.0], "b": [8.0, 0.0, 24.0, 16.0], "c": [-4.0, 0.0, 4.0, 8.0], "d": [0.0, 8.0, 8.0, 16.0]}
DERIVED = ("summary", "human_summary", "JSD_lattice", "JSD_amplitude", "JSD_direction", "W1_amplitude", "JSD_turn",
           "JSD_transition")                                       # log-based: compared in-process


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def _dyadic(g, shape, lo=-2048, hi=2048):
    return g.integers(lo, hi, shape) / 1024.0


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _lengths(scanpaths, limit):
    return np.minimum(np.array([len(sp) for sp in scanpaths], dtype=np.int64), limit).astype(np.int32)


# ---- stand-ins: the signatures and result layouts of the entry points they replace -------------------------------------------------------
def scanpath_likelihood(probs, scanpaths, rows, frame_size, *, uniform_mix=None, metrics=("LL", "NSS", "AUC"), map_shape=None,
                        baseline=None, baseline_rows=None, log_normal_mu=None, log_normal_sigma2=None, min_length=0):
    """"LL": -inf at [0, 0] and NaN at [3, 1]; "NSS": NaN for every scanpath of sample 1 (key "b": a key that scores NaN)"""
    p, rows = _np(probs), np.asarray(rows, dtype=np.int64)
    S, n = len(scanpaths), _lengths(scanpaths, p.shape[1])
    g = _rng("likelihood", p.shape, rows.tolist(), tuple(metrics), None if baseline_rows is None else list(baseline_rows), min_length)
    beyond = np.arange(p.shape[1])[None, :] >= n[:, None]
    res = {}
    for m in metrics:
        if m == "STOP":
            res[m] = _dyadic(g, S) + p[rows, 0, 0]
            res[m][S - 1] = -np.inf
            continue
        v = _dyadic(g, (S, p.shape[1])) + p[rows, :, 0]
        if m == "IG":
            v = v - np.asarray(baseline, dtype=np.float64)[np.asarray(baseline_rows, dtype=np.int64), 0][:, None]
        if m == "DLL":
            v = v + _np(log_normal_mu)[rows] - _np(log_normal_sigma2)[rows]
        if m == "LL":
            v[0, 0], v[3, 1] = -np.inf, np.nan
        if m == "NSS":
            v[rows % N == 1] = np.nan
        v[beyond] = np.nan
        res[m] = v
    return dict(res, n=n, dropped=g.integers(0, 3, S).astype(np.int32))


def kde_leave_out_likelihood(scanpaths, image_groups, frame_size, map_shape, *, bandwidth, uniform_mix, leave, max_length=None):
    """NaN for the one scanpath of sample 1 (nobody else saw the image) and at [2, 0]; -inf at [0, 1] when whole scanpaths are left out"""
    image = np.asarray(image_groups, dtype=np.int64)
    S, n = len(scanpaths), _lengths(scanpaths, max_length)
    g = _rng("kde", image.tolist(), n.tolist(), leave, bandwidth, uniform_mix)
    v = _dyadic(g, (S, int(n.max())))
    v[np.arange(v.shape[1])[None, :] >= n[:, None]] = np.nan
    v[np.bincount(image)[image] == 1] = np.nan
    v[2, 0] = np.nan
    if leave == "scanpath":
        v[0, 1] = -np.inf
    return dict(LL=v, others=np.zeros(v.shape, np.int32), n=n, dropped=g.integers(0, 3, S).astype(np.int32))


def target_hits(scanpaths, boxes, *, max_steps):
    """no hit for every fourth scanpath and for one whose box starts left of the frame (key "c": a key without a hit)"""
    box = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    S = len(scanpaths)
    g = _rng("hits", box.tolist(), max_steps)
    hit = g.integers(0, max_steps, S).astype(np.int32)
    hit[(box[:, 0] < 0) | (np.arange(S) % 4 == 3)] = -1
    spr, path = (np.where(hit >= 0, _dyadic(g, S, 1, 4096), np.nan) for _ in range(2))
    return {"hit": hit, "path": path, "SPR": spr, "n": _lengths(scanpaths, max_steps)}


def target_hit_probability(probs, boxes, box_rows, frame_size, *, min_length, map_shape=None):
    """the curve of box 1 is NaN from step 2 on; some boxes hold no cell"""
    p, rows = _np(probs), np.asarray(box_rows, dtype=np.int64)
    g = _rng("mass", p.shape, rows.tolist(), np.asarray(boxes).tolist(), min_length)
    hit = _dyadic(g, (len(rows), p.shape[1]), 0, 64) + p[rows, :, 0] / 16
    tfp = np.cumsum(hit, 1)
    if len(rows) > 1:
        tfp[1, 2:] = np.nan
    return {"MASS": hit.copy(), "HIT": hit, "TFP": tfp, "cells": g.integers(0, 4, len(rows)).astype(np.int32)}


def saccade_counts(scanpaths, groups, n_groups, frame_size, map_shape, *, max_steps):
    grp, S = np.asarray(groups, dtype=np.int64), len(scanpaths)
    g = _rng("counts", grp.tolist(), n_groups, tuple(map_shape), max_steps)
    counts = g.integers(0, 20, (n_groups, 2 * map_shape[0] - 1, 2 * map_shape[1] - 1)).astype(np.int64)
    counts[np.bincount(grp, minlength=n_groups) == 0] = 0
    return {"counts": counts, "saccades": g.integers(0, 9, S).astype(np.int32), "dropped": g.integers(0, 3, S).astype(np.int32)}


def saccade_expectation(probs, row_groups, n_groups, *, min_length, max_steps, map_shape=None):
    """row 1 is bad: NaN saccades, nothing added to its group"""
    p, grp = _np(probs), np.asarray(row_groups, dtype=np.int64)
    R = len(grp)
    g = _rng("expectation", p.shape, grp.tolist(), n_groups, min_length, max_steps)
    bad = np.zeros(R, dtype=np.int32)
    bad[1:2] = 1
    sacc = _dyadic(g, R, 0, 4096) + p[:, 0, 0]
    sacc[bad == 1] = np.nan
    E = np.zeros((n_groups,) + LATTICE)
    for r in range(R):
        lattice = _dyadic(g, LATTICE, 0, 2048) + p[r, 1, 0]
        if not bad[r]:
            E[grp[r]] += lattice
    return {"E": E, "saccades": sacc, "bad": bad}


def turn_counts(scanpaths, groups, n_groups, frame_size, map_shape, *, max_steps, n_directions):
    grp, S = np.asarray(groups, dtype=np.int64), len(scanpaths)
    g = _rng("turn_counts", grp.tolist(), n_groups, tuple(map_shape), max_steps, n_directions)
    counts = g.integers(0, 20, (n_groups, n_directions + 1, n_directions + 1)).astype(np.int64)
    counts[np.bincount(grp, minlength=n_groups) == 0] = 0
    return {"counts": counts, "pairs": g.integers(0, 9, S).astype(np.int32), "dropped": g.integers(0, 3, S).astype(np.int32)}


def turn_expectation(probs, row_groups, n_groups, *, min_length, max_steps, frame_size, n_directions, map_shape=None):
    """row 1 is bad: NaN pairs, nothing added to its group"""
    p, grp = _np(probs), np.asarray(row_groups, dtype=np.int64)
    R = len(grp)
    g = _rng("turn_expectation", p.shape, grp.tolist(), n_groups, min_length, max_steps, tuple(frame_size), n_directions)
    bad = np.zeros(R, dtype=np.int32)
    bad[1:2] = 1
    pairs = _dyadic(g, R, 0, 4096) + p[:, 0, 0]
    pairs[bad == 1] = np.nan
    M = np.zeros((n_groups, n_directions + 1, n_directions + 1))
    for r in range(R):
        table = _dyadic(g, M.shape[1:], 0, 2048) + p[r, 1, 0]
        if not bad[r]:
            M[grp[r]] += table
    return {"M": M, "pairs": pairs, "bad": bad}


def install(setattr_):
    """replace the eight entry points; setattr_(module, name, value): monkeypatch.setattr in the test, setattr in the recording script"""
    from scanpaths_amd.utils.evaltools import saccade_statistics, scanpath_kde, search_efficiency, turn_statistics
    from scanpaths_amd.utils.evaltools import scanpath_likelihood as lik
    setattr_(lik, "scanpath_likelihood", scanpath_likelihood)
    setattr_(scanpath_kde, "kde_leave_out_likelihood", kde_leave_out_likelihood)
    setattr_(search_efficiency, "target_hits", target_hits)
    setattr_(search_efficiency, "target_hit_probability", target_hit_probability)
    setattr_(saccade_statistics, "saccade_counts", saccade_counts)
    setattr_(saccade_statistics, "saccade_expectation", saccade_expectation)
    setattr_(turn_statistics, "turn_counts", turn_counts)
    setattr_(turn_statistics, "turn_expectation", turn_expectation)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def _paths(g, lengths):
    return [np.c_[_dyadic(g, (n, 2), 0, 24 * 1024), _dyadic(g, (n, 1), 1, 1024)] for n in lengths]


def _predict(seed, heads):
    g = _rng("predict", seed, heads)
    out = {}
    for h in (("good_", "poor_") if heads else ("",)):
        out[h + "all_actions_prob"] = torch.from_numpy(_dyadic(g, (N, T, A), 0, 2048)).to(torch.float32)
        out[h + "log_normal_mu"] = torch.from_numpy(_dyadic(g, (N, T))).to(torch.float32)
        out[h + "log_normal_sigma2"] = torch.from_numpy(_dyadic(g, (N, T), 1, 2048)).to(torch.float32)
    return out


def fix_vectors(seed=0):
    g = _rng("subjects", seed)
    return [_paths(g, lengths) for lengths in LENGTHS]


class _OnDevice:
    """a batch entry whose .cuda() is itself; multiplied by 0 it remembers that it was zeroed"""

    def __init__(self, zeroed=False):
        self.shape, self.zeroed = (N, 3, 8, 8), zeroed

    def cuda(self):
        return self

    def __mul__(self, other):
        return _OnDevice(self.zeroed or other == 0)


class _Model:
    """two AiR heads for a call without tasks, the one COCO-Search18 head with them; log: (positional arguments, maps zeroed) per call"""

    def __init__(self):
        self.log = []

    def eval(self):
        return self

    def __call__(self, *args):
        self.log.append((len(args), int(args[1].zeroed)))
        return _predict(len(self.log), heads=len(args) == 2)


def _loader(tasks):
    for seed in (1, 2):
        batch = {"images": _OnDevice(), "attention_maps": _OnDevice(), "fix_vectors": fix_vectors(seed), "performances": PERFORMANCES,
                 "question_ids": KEYS, "img_names": ["i0", "i1", "i2"], "baseline_rows": [0, 1, 0]}
        if tasks:
            batch["tasks"] = _OnDevice()
        yield batch


# ---- the calls -------------------------------------------------------------------------------------------------------------------------------
def _refusal(call, *args, **kw):
    try:
        call(*args, **kw)
    except (ValueError, TypeError) as e:
        return f"{type(e).__name__}: {e}"
    return "no refusal"


def _test_loop(res):
    return res[0], {"records": len(res[3]), "lengths": [r["length"] for r in res[3]], "performance": [r["performance"] for r in res[3]]}


def collect(setattr_):
    """every case -> {name: result}; install(setattr_) must have been called.  setattr_ also replaces the sampling and the device
    scoring of run_test_loop."""
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    out = {}
    fvs, one, two = fix_vectors(), _predict(0, False), _predict(0, True)
    g = _rng("inputs")
    base2, base1 = _dyadic(g, (2, A - 1), 1, 2048), _dyadic(g, (1, A - 1), 1, 2048)
    shape = dict(frame_size=FRAME, map_shape=MAP)

    # likelihood and its gold standard
    lkw = dict(uniform_mix=0.25, metrics=METRICS, min_length=1, **shape)
    out["lik/plain"] = E.likelihood_evaluation(one, fvs, KEYS, None, [0, 1, 0], base2, **lkw)
    out["lik/heads"] = E.likelihood_evaluation(two, fvs, KEYS, PERFORMANCES, None, base1, **lkw)
    for same in (False, True):
        out[f"gold/same_step{int(same)}"] = E.likelihood_gold_standard_evaluation(fvs, KEYS, bandwidth=8.0, uniform_mix=0.25, max_length=T,
                                                                                  same_step=same, **shape)
    table = E.LikelihoodTable()
    table.add(out["lik/plain"][0])
    table.add(out["lik/heads"][0])
    table.add({k: v for k, v in out["gold/same_step0"][0].items() if k != "dropped"})
    out["lik/table"] = table.result()

    # search efficiency: the model's curve, T > max_steps and T < max_steps (padded with the last value)
    curve = {3: [0.25, 0.5, 0.75], 6: [0.125, 0.25, 0.5, 0.5, 0.75, 1.0]}
    for name, predict, perf in (("plain", one, None), ("heads", two, ENTRIES)):
        for steps in (3, 6):
            for human in (None, curve[steps]):
                out[f"search/model/{name}/steps{steps}/human{int(human is not None)}"] = E.search_efficiency_model_evaluation(
                    predict, KEYS, BOXES, min_length=1, max_steps=steps, performances=perf, human_curve=human, **shape)
    table = E.SearchEfficiencyTable()
    table.add(out["search/model/plain/steps3/human0"][0])
    table.add(out["search/model/heads/steps3/human1"][0])
    out["search/model/table"] = table.result()
    out["search/model/table/human"] = table.result(curve[3])
    # ... and scanpaths that exist: key "d" has no prediction, key "c" no hit
    g = _rng("scanpaths")
    gt_keys, predict_keys = ["a", "b", "a", "c", "d", "c"], ["a", "a", "b", "c"]
    gt, pred = _paths(g, [3, 5, 2, 4, 7, 1]), _paths(g, [4, 2, 6, 3])
    table = E.SearchEfficiencyTable()
    for steps in (3, 6):
        out[f"search/eval/steps{steps}"] = E.search_efficiency_evaluation(gt, pred, gt_keys, predict_keys, BOXES, max_steps=steps)
        out[f"search/human/steps{steps}"] = E.search_efficiency_human_evaluation(gt, gt_keys, BOXES, max_steps=steps)
    table.add(out["search/eval/steps6"][0])
    table.add(out["search/human/steps6"][0])
    out["search/eval/table"] = table.result()

    # saccade statistics
    skw = dict(max_steps=6, amplitude_edges=EDGES, n_directions=DIRECTIONS, **shape)
    for name, groups in (("pooled", None), ("groups", GROUPS)):
        out[f"saccade/eval/{name}"] = E.saccade_statistics_evaluation(gt, pred, gt_keys, predict_keys, groups=groups, **skw)
        out[f"saccade/human/{name}"] = E.saccade_statistics_human_evaluation(gt, gt_keys, groups=groups, **skw)
    human = out["saccade/human/groups"][0]
    lattice = human["human_lattice_sum"]
    by_label = {None: lattice, "find": human["by_group"]["find"]["human_lattice_sum"]}             # "count" has none: no comparison
    mkw = dict(min_length=1, max_steps=3, **shape)
    out["saccade/model/plain/bare"] = E.saccade_statistics_model_evaluation(one, KEYS, **mkw)
    out["saccade/model/plain/lattice"] = E.saccade_statistics_model_evaluation(one, KEYS, human_lattice=lattice, amplitude_edges=EDGES,
                                                                               n_directions=DIRECTIONS, **mkw)
    for name, against in (("none", None), ("lattice", lattice), ("dict", by_label)):
        out[f"saccade/model/heads/{name}"] = E.saccade_statistics_model_evaluation(
            two, KEYS, performances=ENTRIES, groups=GROUPS, human_lattice=against, amplitude_edges=EDGES, n_directions=DIRECTIONS, **mkw)
    table = E.SaccadeStatisticsTable(FRAME, MAP, EDGES, DIRECTIONS)
    table.add(out["saccade/model/heads/none"][0])
    table.add(E.saccade_statistics_model_evaluation(one, KEYS, groups=GROUPS, **mkw)[0])
    for name, against in (("none", None), ("lattice", lattice), ("dict", by_label)):
        out[f"saccade/model/table/{name}"] = table.result(against)
    table = E.SaccadeStatisticsTable(FRAME, MAP, EDGES, DIRECTIONS)
    table.add(out["saccade/eval/groups"][0])
    table.add(out["saccade/human/groups"][0])
    out["saccade/eval/table"] = table.result()
    out["saccade/eval/table/lattice"] = table.result(lattice)

    # turning angles: every saccade case again
    ukw = dict(max_steps=6, n_directions=DIRECTIONS, **shape)
    for name, groups in (("pooled", None), ("groups", GROUPS)):
        out[f"turn/eval/{name}"] = E.turn_statistics_evaluation(gt, pred, gt_keys, predict_keys, groups=groups, **ukw)
        out[f"turn/human/{name}"] = E.turn_statistics_human_evaluation(gt, gt_keys, groups=groups, **ukw)
    human = out["turn/human/groups"][0]
    turns = human["human_table_sum"]
    turns_by_label = {None: turns, "find": human["by_group"]["find"]["human_table_sum"]}           # "count" has none: no comparison
    tkw = dict(min_length=1, max_steps=3, n_directions=DIRECTIONS, **shape)
    out["turn/model/plain/none"] = E.turn_statistics_model_evaluation(one, KEYS, **tkw)
    out["turn/model/plain/table"] = E.turn_statistics_model_evaluation(one, KEYS, human_table=turns, **tkw)
    for name, against in (("none", None), ("table", turns), ("dict", turns_by_label)):
        out[f"turn/model/heads/{name}"] = E.turn_statistics_model_evaluation(two, KEYS, performances=ENTRIES, groups=GROUPS,
                                                                             human_table=against, **tkw)
    turn_table = E.TurnStatisticsTable(DIRECTIONS)
    turn_table.add(out["turn/model/heads/none"][0])
    turn_table.add(E.turn_statistics_model_evaluation(one, KEYS, groups=GROUPS, **tkw)[0])
    for name, against in (("none", None), ("table", turns), ("dict", turns_by_label)):
        out[f"turn/model/table/{name}"] = turn_table.result(against)
    turn_table = E.TurnStatisticsTable(DIRECTIONS)
    turn_table.add(out["turn/eval/groups"][0])
    turn_table.add(out["turn/human/groups"][0])
    out["turn/eval/table"] = turn_table.result()
    out["turn/eval/table/table"] = turn_table.result(turns)

    # refusals of the model-side calls, word for word
    lik = dict(uniform_mix=0.25, **shape)
    out["refusals"] = [
        _refusal(E.likelihood_evaluation, one, fvs, KEYS, PERFORMANCES, **lik),
        _refusal(E.likelihood_evaluation, two, fvs, KEYS, **lik),
        _refusal(E.likelihood_evaluation, {"all_actions_prob": one["all_actions_prob"]}, fvs, KEYS, metrics=("DLL",), **lik),
        _refusal(E.likelihood_evaluation, one, fvs[:2], KEYS[:2], **lik),
        _refusal(E.likelihood_evaluation, two, fvs, KEYS, ENTRIES, **lik),
        _refusal(E.likelihood_evaluation, one, fvs, KEYS, None, None, base2, metrics=("IG",), **lik),
        _refusal(E.search_efficiency_model_evaluation, one, KEYS, BOXES, performances=ENTRIES, **mkw),
        _refusal(E.search_efficiency_model_evaluation, two, KEYS[:2], BOXES, performances=ENTRIES[:2], **mkw),
        _refusal(E.search_efficiency_model_evaluation, two, KEYS, BOXES, performances=ENTRIES[:2], **mkw),
        _refusal(E.search_efficiency_model_evaluation, one, ["a", "b", "z"], BOXES, **mkw),
        _refusal(E.saccade_statistics_model_evaluation, two, KEYS, **mkw),
        _refusal(E.saccade_statistics_model_evaluation, one, KEYS[:2], **mkw),
        _refusal(E.saccade_statistics_model_evaluation, two, KEYS, performances=[[], [], []], **mkw),
        _refusal(E.saccade_statistics_model_evaluation, one, KEYS, groups={"a": "find"}, **mkw),
        _refusal(E.saccade_statistics_model_evaluation, one, KEYS, human_lattice=lattice, **mkw),
        _refusal(E.saccade_statistics_model_evaluation, one, KEYS, min_length=1, max_steps=3, frame_size=FRAME, map_shape=(4, 4)),
        _refusal(table.add, {"lattice_sum": np.zeros((3, 3))}),
    ]
    out["refusals_turn"] = [
        _refusal(E.turn_statistics_model_evaluation, two, KEYS, **tkw),
        _refusal(E.turn_statistics_model_evaluation, one, KEYS[:2], **tkw),
        _refusal(E.turn_statistics_model_evaluation, two, KEYS, performances=[[], [], []], **tkw),
        _refusal(E.turn_statistics_model_evaluation, one, KEYS, groups={"a": "find"}, **tkw),
        _refusal(E.turn_statistics_model_evaluation, one, KEYS, human_table=np.zeros((3, 3)), **tkw),
        _refusal(E.turn_statistics_model_evaluation, one, KEYS, min_length=1, max_steps=3, n_directions=DIRECTIONS, frame_size=FRAME,
                 map_shape=(4, 4)),
        _refusal(E.turn_statistics_model_evaluation, one, KEYS, min_length=1, max_steps=3, n_directions=17, **shape),
        _refusal(turn_table.add, {"table_sum": np.zeros((3, 3))}),
    ]

    # the batch loops: what the model was called with, and what came back
    setattr_(inference, "sample_batch", lambda predict, sampling, repeat_num: (torch.ones(repeat_num, 2, N, T, 3),
                                                                               torch.full((repeat_num, 2, N), 2, dtype=torch.int32)))
    setattr_(E, "evaluation_performance_related", lambda gt, pred, perf, alloc, multimatch: ({"pairs": len(gt)}, {}, []))
    gold = dict(bandwidth=8.0, uniform_mix=0.25, max_length=T, map_shape=MAP)
    loops = {
        "likelihood": lambda m, ld, ab: inference.run_likelihood_loop(m, ld, uniform_mix=0.25, baseline=base2, ablate_attention_info=ab, **shape),
        "likelihood_gold": lambda m, ld, ab: inference.run_likelihood_gold_loop(m, ld, gold_standard=gold, uniform_mix=0.25, baseline=base2,
                                                                                ablate_attention_info=ab, **shape),
        "search_efficiency": lambda m, ld, ab: inference.run_search_efficiency_loop(m, ld, boxes=BOXES, min_length=1, max_steps=6,
                                                                                    human_curve=curve[6], ablate_attention_info=ab, **shape),
        "saccade_statistics": lambda m, ld, ab: inference.run_saccade_statistics_loop(
            m, ld, min_length=1, max_steps=3, amplitude_edges=EDGES, n_directions=DIRECTIONS, human_lattice=lattice, ablate_attention_info=ab,
            **shape),
        "turn_statistics": lambda m, ld, ab: inference.run_turn_statistics_loop(m, ld, human_table=turns, ablate_attention_info=ab, **tkw),
        "test": lambda m, ld, ab: _test_loop(inference.run_test_loop(m, None, ld, repeat_num=2, ablate_attention_info=ab)),
    }
    for name, run in loops.items():
        for tasks in (False, True):
            for ablate in (False, True):
                model = _Model()
                res = run(model, _loader(tasks), ablate)
                case = f"loop/{name}/tasks{int(tasks)}/ablate{int(ablate)}"
                out[case + "/forward_log"] = np.array(model.log, dtype=np.int64)
                out[case] = res
    return out


def flatten(node, path=""):
    """a nested result -> {path: array}: dicts by key, tuples and mixed lists by position, a list of strings as one array"""
    if isinstance(node, dict):
        items = [(k, v) for k, v in node.items()]
    elif isinstance(node, (tuple, list)) and not (len(node) and all(isinstance(v, str) for v in node)):
        items = list(enumerate(node))
    else:
        return {path: np.asarray(node)}
    flat = {}
    for k, v in items:
        flat.update(flatten(v, f"{path}/{k}" if path else str(k)))
    return flat


def is_derived(path) -> bool:
    return any(part in DERIVED for part in path.split("/"))


def pack(flat):
    """{path: array} -> the few arrays of the fixture file: one blob per dtype next to the paths, dtypes and shapes (a file entry per path
    would be mostly zip headers)"""
    paths = sorted(flat)
    kinds = sorted({flat[k].dtype.kind for k in paths})
    out = {"paths": np.array(paths), "dtypes": np.array([flat[k].dtype.str for k in paths]),
           "shapes": np.array(["x".join(map(str, flat[k].shape)) for k in paths])}
    for kind in kinds:
        out["values_" + kind] = np.concatenate([flat[k].reshape(-1) for k in paths if flat[k].dtype.kind == kind])
    return out


def unpack(packed):
    flat, at = {}, {}
    for path, dtype, shape in zip(packed["paths"].tolist(), packed["dtypes"].tolist(), packed["shapes"].tolist()):
        shape, kind = tuple(int(v) for v in shape.split("x") if v), np.dtype(dtype).kind
        n, lo = int(np.prod(shape, dtype=np.int64)), at.get(kind, 0)
        flat[path] = packed["values_" + kind][lo:lo + n].astype(dtype).reshape(shape)
        at[kind] = lo + n
    return flat
