"""RL (self-critical) phase on the HIP path: log-probability kernels and the reward glue against the
reference's outputs (tests/golden/rl.npz), the loss shaping against a literal torch restatement of AiR/train.py:296-342,
and one end-to-end rl_step."""
import os

import numpy as np
import pytest
import scipy.stats
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "rl.npz"))


def test_log_action_and_log_duration_match_reference():
    from scanpaths_amd.models.loss import LogAction, LogDuration
    t = lambda k: torch.from_numpy(GOLD[k]).float().to(DEV)
    p = t("la_p").requires_grad_(True)
    mu, s2 = t("ld_mu").requires_grad_(True), t("ld_s2").requires_grad_(True)
    la = LogAction(p, t("la_mask"))
    ld = LogDuration(t("ld_d"), mu, s2, t("ld_mask"))
    ((la * t("w")).sum() + (ld * t("w")).sum() * 0.5).backward()
    for got, want in ((la, "la_out"), (ld, "ld_out"), (p.grad, "la_dp"), (mu.grad, "ld_dmu"), (s2.grad, "ld_ds2")):
        ref = GOLD[want]
        err = np.abs(got.detach().cpu().double().numpy() - ref).max()
        assert err <= 2e-6 * max(1.0, np.abs(ref).max()), (want, err)          # fp32 kernel vs the fp64 reference run


def test_reward_glue_with_the_hip_scanmatch_matches_reference():
    from helpers import check_rl_glue
    from scanpaths_amd.utils.evaltools.scanmatch import ScanMatch
    cfg = dict(Xres=320, Yres=240, Xbin=16, Ybin=12, Offset=(0, 0), Threshold=3.5)
    check_rl_glue(ScanMatch(TempBin=50, **cfg), ScanMatch(**cfg))               # bit-exact, batched on the device


def test_rl_loss_matches_literal_restatement():
    """AiR/train.py:296-342 restated literally in torch (incl. the lambda_5 no-op quirk) on random rewards"""
    from scanpaths_amd.rl import rl_loss
    g = np.random.Generator(np.random.PCG64(3))
    S, N = 3, 5
    same = g.uniform(0, 1, (2 * S, N, 2)); diff = g.uniform(0, 1, (2 * S, N, 2))
    same[1, 2] = np.nan; diff[4, 0, 1] = np.nan; same[0, 3, 0] = 0.0
    gg, gp, gd = g.uniform(0, 1, (N, 2)), g.uniform(0, 1, (N, 2)), g.uniform(0, 1, (N, 2))
    gg[1] = np.nan
    nla = torch.from_numpy(g.uniform(0.1, 2, (2 * S, N))).float()
    nld = torch.from_numpy(g.uniform(0.1, 2, (2 * S, N))).float()
    # literal restatement
    s_, d_ = same.copy(), diff.copy()
    s_[np.isnan(s_)] = 0; d_[np.isnan(d_)] = 0
    st, dt = torch.tensor(s_, dtype=torch.float32), torch.tensor(d_, dtype=torch.float32)
    with np.errstate(divide="ignore"):
        sh = torch.tensor(scipy.stats.hmean(st, axis=-1)); dh = torch.tensor(scipy.stats.hmean(dt, axis=-1))
    base = sh.view(2, -1, N).mean(1, keepdim=True).expand((2, S, N)).contiguous().view(-1, N)
    a = nla.clone().requires_grad_(True); b = nld.clone().requires_grad_(True)
    ref = (a * (sh - base)).sum() + (b * (sh - base)).sum()
    ref.backward()
    ad, bd = nla.to(DEV).requires_grad_(True), nld.to(DEV).requires_grad_(True)
    loss, info = rl_loss(ad, bd, same, diff, gg, gp, gd, S, lambda_5=0.7)
    loss.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    assert (ad.grad.cpu() - a.grad).abs().max() <= 1e-6 and (bd.grad.cpu() - b.grad).abs().max() <= 1e-6
    assert info["lambda_5_terms_are_noops_in_the_reference"]


def test_rl_step_end_to_end():
    """eval-mode forward with autograd -> sampled scanpaths -> device ScanMatch rewards -> REINFORCE loss -> clip + Adam"""
    from scanpaths_amd.models.baseline_attention import baseline
    from scanpaths_amd.models.sampling import Sampling
    from scanpaths_amd.optim import FlatAdam
    from scanpaths_amd.procedural import fill_module
    from scanpaths_amd.rl import rl_step
    from scanpaths_amd.synth import make_batch
    from scanpaths_amd.utils.evaltools.scanmatch import ScanMatch
    from helpers import rl_case
    T, N = 4, 2
    m = baseline(convLSTM_length=T)
    fill_module(m, 6)
    m = m.to(DEV)
    opt = FlatAdam(m.parameters(), lr=1e-5, weight_decay=5e-5, clip=12.5)
    b = make_batch("AiR", N, 240, 320, T, seed=6)
    gt, perf, _ = rl_case()
    gt, perf = [gt[0], gt[3]], [perf[0], perf[3]]                         # two images with good and poor human scanpaths
    cfg = dict(Xres=320, Yres=240, Xbin=16, Ybin=12, Offset=(0, 0), Threshold=3.5)
    before = opt.flat_p.detach().clone()
    loss, info = rl_step(m, Sampling(convLSTM_length=T, min_length=1, map_width=40, map_height=30, width=320, height=240, seed=1),
                         opt, b["images"].to(DEV), b["attention_maps"].to(DEV), gt, perf, ScanMatch(TempBin=50, **cfg),
                         ScanMatch(**cfg), rl_sample_number=2)
    assert np.isfinite(float(loss)) and torch.isfinite(opt.flat_p).all()
    assert float(info["grad_norm"]) > 0 and not torch.equal(before, opt.flat_p)
    assert info["same_reward_hmean"].shape == (4, N) and not m.training


def test_rl_step_redraws_samples_with_non_finite_or_overlong_durations():
    """exp(eps*sigma2 + mu) is heavy-tailed; an inf duration (the reference's int(round(inf)) raises there) or one beyond
    the scorer's symbol cap must not abort the training step -- the sample is redrawn and counted in info["resamples"]"""
    from scanpaths_amd.models.baseline_attention import baseline
    from scanpaths_amd.models.sampling import Sampling
    from scanpaths_amd.optim import FlatAdam
    from scanpaths_amd.procedural import fill_module
    from scanpaths_amd.rl import rl_step
    from scanpaths_amd.synth import make_batch
    from scanpaths_amd.utils.evaltools.scanmatch import ScanMatch
    from helpers import rl_case

    class Spiky(Sampling):
        """every first draw of a head carries one absurd duration"""
        def random_sample(self, *a):
            out = super().random_sample(*a)
            self.n = getattr(self, "n", 0) + 1
            if self.n in (1, 3):
                d = out["durations"].clone()
                d[0, 0] = float("inf") if self.n == 1 else 1e7
                out["durations"] = d
                out["selected_actions"][0, 0] = 5          # make sure the fixation is kept
            return out

    T, N = 4, 2
    m = baseline(convLSTM_length=T)
    fill_module(m, 6)
    m = m.to(DEV)
    opt = FlatAdam(m.parameters(), lr=1e-5, weight_decay=5e-5, clip=12.5)
    b = make_batch("AiR", N, 240, 320, T, seed=6)
    gt, perf, _ = rl_case()
    gt, perf = [gt[0], gt[3]], [perf[0], perf[3]]
    cfg = dict(Xres=320, Yres=240, Xbin=16, Ybin=12, Offset=(0, 0), Threshold=3.5)
    loss, info = rl_step(m, Spiky(convLSTM_length=T, min_length=1, seed=1), opt, b["images"].to(DEV), b["attention_maps"].to(DEV),
                         gt, perf, ScanMatch(TempBin=50, **cfg), ScanMatch(**cfg), rl_sample_number=1)
    assert info["resamples"] >= 2 and np.isfinite(float(loss))


def test_eval_mode_backward_matches_oracle(request):
    """The RL phase differentiates the EVAL-mode forward (softmax heads, running-stat BatchNorm; AiR/train.py:244-251).  One
    decode step at 240x320: a weighted sum of the eval outputs and its parameter gradients against the fp64 oracle; bar =
    20x the fp32 oracle's own error or 1e-4 of the largest gradient norm (the bars of tests/test_model_gpu.py)."""
    from helpers import RL_EVAL_CASE, rl_eval_objective_weights, start_rl_eval_oracle
    from scanpaths_amd.synth import make_batch
    from helpers import build_model as _build
    c = RL_EVAL_CASE
    T = c["T"]
    meta = dict(task="AiR", arch="resnet50", T=T, weight_seed=c["seed"])
    b = make_batch("AiR", c["NB"], c["H"], c["W"], T, seed=c["seed"])
    w = rl_eval_objective_weights()

    def objective(pred, dt, dev):
        return sum((pred[k] * w[k].to(dt).to(dev)).sum() for k in w)

    # the oracle side (fp64 calibration pass, fp64 and fp32 eval forward + backward: ~35 s of host work) runs in a worker process,
    # started with the session when the test is part of one (tests/conftest.py)
    bo = getattr(request.config, "_rl_oracle", None)
    ex, fut = bo if bo is not None else start_rl_eval_oracle()
    calib_np, g64_np, v64, g32_np, v32 = fut.result(timeout=1500)
    if bo is None:
        ex.shutdown(wait=False)
    calib = {k: torch.from_numpy(v) for k, v in calib_np.items()}
    grads = {torch.float64: ({k: torch.from_numpy(v) for k, v in g64_np.items()}, v64),
             torch.float32: ({k: torch.from_numpy(v) for k, v in g32_np.items()}, v32)}
    model = _build(meta, 30, 40)
    model.load_state_dict({k: v.float() for k, v in calib.items()}, strict=False)
    model = model.to(DEV).eval()
    pred = model(b["images"].to(DEV), b["attention_maps"].to(DEV))
    val = objective(pred, torch.float32, DEV)
    val.backward()
    g64, v64 = grads[torch.float64]
    g32, v32 = grads[torch.float32]
    assert abs(float(val) - v64) <= max(1e-4 * abs(v64), 20 * abs(v32 - v64)), (float(val), v64, v32)
    top = max(float(v.norm()) for v in g64.values())
    bad = []
    for k, p in model.named_parameters():
        if k not in g64:
            continue
        got = p.grad.detach().cpu().double() if p.grad is not None else torch.zeros_like(g64[k])
        e, floor = float((got - g64[k]).norm()), float((g32[k].double() - g64[k]).norm())
        if not e <= max(1e-4 * top, 20 * floor):
            bad.append((k, e, floor, float(g64[k].norm())))
    assert not bad, bad[:12]


# ---- OSIE / COCO_Search18 forms of the RL step and of validation scoring (SURVEY.md §8 f2 / f3 widened) -----------
def _task_golden(key):
    return np.load(os.path.join(os.path.dirname(__file__), "golden", f"eval_{key}.npz"))


def _flat_table(d):
    from helpers import EVAL_COLUMNS
    return np.array([float(d[g][k]) for g, k in EVAL_COLUMNS], dtype=np.float64)


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    m = ~np.isnan(b)
    assert np.abs(a[m] - b[m]).max(initial=0.0) <= tol, np.abs(a[m] - b[m]).max()


@pytest.mark.parametrize("key,task", [("osie", "OSIE"), ("coco", "COCO_Search18")])
def test_single_head_validation_scoring_and_rl_reward_match_the_real_reference(key, task):
    """evaluation / human_evaluation / pairs_eval (OSIE) / pairs_eval_scanmatch (COCO_Search18) against outputs of the REAL reference
    functions (tests/golden/eval_<task>.npz from tests/golden/make_golden_eval_tasks.py: /root/reference/OSIE/utils/evaluation.py:11-340,
    /root/reference/COCO_Search18/utils/evaluation.py:11-352; deterministic MultiMatch stand-in on both sides), scored by the batched
    device kernels.  ScanMatch and SED enter bit-exact, STDE <= 4 ulp; float64 collections -> 1e-9, pairs_eval's float32 rows -> 1e-6."""
    from helpers import toy_multimatch, unpack_scanpaths
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools.scanmatch import ScanMatch
    g = _task_golden(key)
    gt = unpack_scanpaths(g["ev_gt_fix"], g["ev_gt_len"], g["ev_gt_count"])
    pred = unpack_scanpaths(g["ev_pred_fix"], g["ev_pred_len"])
    mean, std, scores = E.evaluation(gt, pred, multimatch=toy_multimatch)
    _close(_flat_table(mean), g["ev_mean"], 1e-9)
    _close(_flat_table(std), g["ev_std"], 1e-9)
    _close(np.array(scores), g["ev_scores"], 1e-9)
    assert np.array_equal(np.array(scores)[:, 5:8], g["ev_scores"][:, 5:8])                 # ScanMatch x2 and SED: bit-exact
    for tag in ("hum", "hum2"):
        fix = unpack_scanpaths(g[tag + "_fix"], g[tag + "_len"], g[tag + "_count"])
        names = [f"n{i}" for i in range(len(fix))]
        half = max(1, len(fix) // 2)
        loader = [{"fix_vectors": fix[:half], "img_names": names[:half]}, {"fix_vectors": fix[half:], "img_names": names[half:]}]
        hm, hs, hsc = E.human_evaluation_free_viewing(loader, task=task, multimatch=toy_multimatch)
        _close(_flat_table(hm), g[tag + "_mean"], 1e-9)
        _close(_flat_table(hs), g[tag + "_std"], 1e-9)
        _close(np.array([hsc[n] for n in names]), g[tag + "_scores"], 1e-9)
    cfg = dict(Xres=320, Yres=240, Xbin=16, Ybin=12, Offset=(0, 0), Threshold=3.5)
    wd, wod = ScanMatch(TempBin=50, **cfg), ScanMatch(**cfg)
    pgt = unpack_scanpaths(g["pe_gt_fix"], g["pe_gt_len"], g["pe_gt_count"])
    ppred = unpack_scanpaths(g["pe_pred_fix"], g["pe_pred_len"])
    rew = E.pairs_eval(pgt, ppred, wd, wod, multimatch=toy_multimatch) if task == "OSIE" else E.pairs_eval_scanmatch(pgt, ppred, wd, wod)
    _close(rew, g["pe_reward"], 1e-6 if task == "OSIE" else 1e-12)
    if task == "OSIE":
        assert np.isnan(rew[2]).all() and rew.shape == (6, 11)                              # the image whose only human scanpath is unscorable


@pytest.mark.parametrize("key,task", [("osie", "OSIE"), ("coco", "COCO_Search18")])
def test_single_head_rl_loss_matches_the_reference_lines(key, task):
    """reward -> harmonic mean -> per-image baseline -> loss with its gradients, against the reference's own lines (OSIE/train.py:248-258,
    COCO_Search18/train.py:269-279) executed on seeded tensors by tests/golden/make_golden_eval_tasks.py"""
    from scanpaths_amd.rl import rl_loss_single_head
    g = _task_golden(key)
    a = torch.from_numpy(g["rl_nla"]).float().to(DEV).requires_grad_(True)
    b = torch.from_numpy(g["rl_nld"]).float().to(DEV).requires_grad_(True)
    loss, info = rl_loss_single_head(a, b, g["rl_reward"], task)
    loss.backward()
    assert np.abs(info["reward_hmean"] - g["rl_hmean"]).max() <= 1e-6
    for got, want in ((loss, "rl_loss"), (info["loss_actions"], "rl_loss_actions"), (info["loss_duration"], "rl_loss_duration")):
        assert abs(float(got) - float(g[want])) <= 2e-6 * max(1.0, abs(float(g[want]))), (want, float(got), float(g[want]))
    assert np.abs(a.grad.cpu().numpy() - g["rl_dnla"]).max() <= 1e-6 and np.abs(b.grad.cpu().numpy() - g["rl_dnld"]).max() <= 1e-6


@pytest.mark.parametrize("task", ["OSIE", "COCO_Search18"])
def test_single_head_rl_step_end_to_end(task):
    """OSIE/train.py:205-262 / COCO_Search18/train.py:219-283 on the HIP path: eval-mode forward with autograd -> sampled scanpaths ->
    device-scored rewards (pairs_eval incl. MultiMatch, SED, STDE / pairs_eval_scanmatch) -> REINFORCE loss -> clip + Adam"""
    from helpers import unpack_scanpaths
    from scanpaths_amd.models.sampling import Sampling
    from scanpaths_amd.models.scanpath_model import ScanpathModel
    from scanpaths_amd.optim import FlatAdam
    from scanpaths_amd.procedural import fill_module
    from scanpaths_amd.rl import rl_step_single_head
    from scanpaths_amd.synth import make_batch
    from scanpaths_amd.utils.evaltools.scanmatch import ScanMatch
    T, N = 4, 2
    m = ScanpathModel(task, convLSTM_length=T, arch="resnet18" if task == "OSIE" else "resnet50")
    fill_module(m, 6)
    m = m.to(DEV)
    opt = FlatAdam(m.parameters(), lr=1e-5, weight_decay=5e-4, clip=12.5, conditional_params=m.has_conditional_params)
    b = make_batch(task, N, 240, 320, T, seed=6)
    g = _task_golden("osie" if task == "OSIE" else "coco")
    gt = unpack_scanpaths(g["pe_gt_fix"], g["pe_gt_len"], g["pe_gt_count"])
    gt = [gt[3], gt[1]]                                                   # two images with several scorable human scanpaths
    cfg = dict(Xres=320, Yres=240, Xbin=16, Ybin=12, Offset=(0, 0), Threshold=3.5)
    before = opt.flat_p.detach().clone()
    loss, info = rl_step_single_head(m, Sampling(convLSTM_length=T, min_length=3, map_width=40, map_height=30, width=320, height=240, seed=1),
                                     opt, b["images"].to(DEV), gt, ScanMatch(TempBin=50, **cfg), ScanMatch(**cfg), task,
                                     attention_maps=b["attention_maps"].to(DEV), tasks=b["tasks"].to(DEV) if b.get("tasks") is not None else None,
                                     rl_sample_number=3)
    assert np.isfinite(float(loss)) and torch.isfinite(opt.flat_p).all() and not m.training
    assert float(info["grad_norm"]) > 0 and not torch.equal(before, opt.flat_p)
    assert info["reward_hmean"].shape == (3, N) and info["metrics_for_reward"].shape == ((11,) if task == "OSIE" else (2,))
