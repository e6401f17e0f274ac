"""Drop-in for the supervised losses of ``models/loss.py`` (the two the train step calls, AiR/train.py:192-195).

CrossEntropyLoss(input, gt, mask)                      AiR/models/loss.py:10-14
MLPLogNormalDistribution(mu, sigma2, gt, mask)         AiR/models/loss.py:27-32
Each is computed by the fused HIP loss kernel (value + gradient in one pass).  ``supervised_loss`` is the fused
form of ``loss_actions + lambda_1 * loss_duration`` (one launch, what bench.py times).  The RL phase's LogAction / LogDuration and
the attention-supervision losses (DurationSmoothL1Loss ... KLD_question_aligment, AiR/models/loss.py:16-25,47-170; csrc/salmaps.hip)
complete the reference module's names, so its import lines work with only the package prefix changed."""
import torch
from torch.autograd.function import once_differentiable

from .. import functional as F

epsilon = 1e-7


def supervised_loss(predicts, scanpaths, durations, action_masks, duration_masks, lambda_1=1.0, mask_sums=None):
    """loss = L_actions + lambda_1 * L_duration of the supervised phase (AiR/train.py:192-197) -> (loss, L_actions, L_duration); ONE launch
    for value and gradient.  Like the two separate calls below it sends exact zeros into the predictions of masked-out steps; the decoder's
    backward pass finds those in the gradient it receives and skips what they imply (functional._OutputGate) -- nothing to switch on."""
    z = predicts["actions"] if "actions" in predicts else predicts["all_actions_prob"]
    return F.scanpath_loss(z, predicts["log_normal_mu"], predicts["log_normal_sigma2"], scanpaths, action_masks, durations,
                           duration_masks, lambda_1, mask_sums)


def CrossEntropyLoss(input, gt, mask):
    B, T, _ = input.shape
    dummy = torch.ones(B, T, device=input.device)
    zero = torch.zeros(B, T, device=input.device)
    ones2 = torch.cat([F.device_sum(mask), torch.ones(1, device=input.device)])
    _, la, _ = _both(input, dummy, dummy, gt, mask, dummy, zero, ones2)
    return la


def MLPLogNormalDistribution(log_normal_mu, log_normal_sigma2, gt, mask):
    B, T = log_normal_mu.shape
    z = torch.zeros(B, T, 4, device=gt.device)
    g = torch.zeros(B, T, 4, device=gt.device)
    zero = torch.zeros(B, T, device=gt.device)
    sums = torch.cat([torch.ones(1, device=gt.device), F.device_sum(mask)])
    _, _, ld = _both(z, log_normal_mu, log_normal_sigma2, g, zero, gt, mask, sums)
    return ld


class _Split(torch.autograd.Function):
    """expose loss_actions / loss_duration of the fused kernel as separately differentiable scalars"""
    @staticmethod
    def forward(ctx, z, mu, s2, gt, am, dur, dm, sums):
        from ..functional import _ScanpathLoss
        with torch.enable_grad():
            zz, mm, ss = z.detach().requires_grad_(True), mu.detach().requires_grad_(True), s2.detach().requires_grad_(True)
            loss, la, ld = _ScanpathLoss.apply(zz, mm, ss, gt, am, dur, dm, 1.0, sums)
            gz, gm, gs = torch.autograd.grad(loss, (zz, mm, ss))
        ctx.save_for_backward(gz, gm, gs)
        return loss.detach(), la.detach(), ld.detach()

    @staticmethod
    def backward(ctx, g0, g1, g2):
        gz, gm, gs = ctx.saved_tensors
        # dz carries only the action term, dmu/dsigma2 only the duration term (lambda_1 = 1 inside)
        ga = (g0 + g1).reshape(1).float().contiguous()
        gd = (g0 + g2).reshape(1).float().contiguous()
        from .. import hip
        outs = []
        for t, g in ((gz, ga), (gm, gd), (gs, gd)):
            o = torch.empty_like(t)
            hip.check(hip.lib().sp_scale_by(hip.ptr(t), hip.ptr(g), t.numel(), hip.ptr(o), hip.stream()), "sp_scale_by")
            outs.append(o)
        return outs[0], outs[1], outs[2], None, None, None, None, None


def _both(z, mu, s2, gt, am, dur, dm, sums):
    return _Split.apply(z, mu, s2, gt.contiguous(), am.contiguous(), dur.contiguous(), dm.contiguous(), sums)


# ---- RL (self-critical) phase: per-sample log-probabilities of sampled scanpaths, AiR/models/loss.py:34-45 ----------------
class _LogAction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, mask):
        from ..hip import check, lib, ptr, stream
        p, m = input.contiguous().float(), mask.contiguous().float()
        B, T = p.shape
        out = torch.empty(B, device=p.device)
        coef = torch.empty_like(p)
        check(lib().sp_log_action(ptr(p), ptr(m), B, T, ptr(F.device_sum(m)), ptr(out), ptr(coef), stream()), "sp_log_action")
        ctx.save_for_backward(coef)
        return out

    @staticmethod
    def backward(ctx, g):
        from ..hip import check, lib, ptr, stream
        (coef,) = ctx.saved_tensors
        B, T = coef.shape
        dp = torch.empty_like(coef)
        check(lib().sp_rowscale(ptr(coef), ptr(g.contiguous()), B, T, ptr(dp), stream()), "sp_rowscale")
        return dp, None


class _LogDuration(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, mu, sigma2, mask):
        from ..hip import check, lib, ptr, stream
        d, mu_, s2, m = (t.contiguous().float() for t in (input, mu, sigma2, mask))
        B, T = d.shape
        out = torch.empty(B, device=d.device)
        dmu, ds2 = torch.empty_like(d), torch.empty_like(d)
        check(lib().sp_log_duration(ptr(d), ptr(mu_), ptr(s2), ptr(m), B, T, ptr(F.device_sum(m)), ptr(out), ptr(dmu), ptr(ds2),
                                    stream()), "sp_log_duration")
        ctx.save_for_backward(dmu, ds2)
        return out

    @staticmethod
    def backward(ctx, g):
        from ..hip import check, lib, ptr, stream
        dmu, ds2 = ctx.saved_tensors
        B, T = dmu.shape
        g = g.contiguous()
        gmu, gs2 = torch.empty_like(dmu), torch.empty_like(ds2)
        check(lib().sp_rowscale(ptr(dmu), ptr(g), B, T, ptr(gmu), stream()), "sp_rowscale")
        check(lib().sp_rowscale(ptr(ds2), ptr(g), B, T, ptr(gs2), stream()), "sp_rowscale")
        return None, gmu, gs2, None


def LogAction(input, mask):
    """[B] = sum_t log(p + eps) * mask / mask.sum()  -- probabilities of the sampled actions (AiR/models/loss.py:34-37)"""
    return _LogAction.apply(input, mask)


def LogDuration(input, log_normal_mu, log_normal_sigma2, mask):
    """[B] = sum_t logpdf_lognormal(duration; mu, sigma2) * mask / mask.sum()  (AiR/models/loss.py:39-45); the sampled
    durations carry no gradient (the reference passes durations.data)"""
    return _LogDuration.apply(input, log_normal_mu, log_normal_sigma2, mask)


# ---- attention-supervision losses, AiR/models/loss.py:16-25, 47-170 (csrc/salmaps.hip) -------------------------------------------
# Each launch writes the value and d value / d prediction; the backward pass scales those coefficients by grad_output.  Only the
# prediction arguments are differentiable (the first argument; sigma2 for Rayleigh; both arguments of CC_MatchLoss): a target, mask or
# box that requires grad is refused rather than silently dropped, and double backward raises (once_differentiable).
_tickets = {}


def _ticket(dev):
    """a zeroed device word per (device, stream): the launch's last workgroup takes the mean over rows and puts the word back to 0"""
    key = (F.hip.device_index(dev), torch.cuda.current_stream(dev).cuda_stream)
    t = _tickets.get(key)
    if t is None:
        t = _tickets[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def _no_grad_targets(name, **targets):
    for k, v in targets.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise RuntimeError(f"{name}: no gradient is computed for `{k}` (only the prediction is differentiable); pass {k}.detach()")


def _f32(t):
    if not t.is_cuda:
        raise RuntimeError("scanpaths_amd losses run on a HIP device only (no CPU path)")
    return t.detach().float().contiguous()


def _rows(t):
    return t.reshape(t.shape[0], -1)


class _ScaledByGrad(torch.autograd.Function):
    """forward: (value, coef) from one launch -> value; backward: coef * grad_output (scalar value: sp_scale_by, one value per row of
    coef: sp_rowscale)"""
    @staticmethod
    def forward(ctx, x, value, coef):
        ctx.save_for_backward(coef)
        ctx.shape = x.shape
        ctx.mark_non_differentiable(coef)
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from ..hip import check, lib, ptr, stream
        (coef,) = ctx.saved_tensors
        g = g.detach().float().contiguous()
        out = torch.empty_like(coef)
        if g.numel() == 1:
            check(lib().sp_scale_by(ptr(coef), ptr(g), coef.numel(), ptr(out), stream()), "sp_scale_by")
        else:
            check(lib().sp_rowscale(ptr(coef), ptr(g), g.numel(), coef.numel() // g.numel(), ptr(out), stream()), "sp_rowscale")
        return out.reshape(ctx.shape), None, None


def _attach(x, value, coef):
    """the value as a function of x (coef = d value / d x, same element order as x)"""
    if x.requires_grad and torch.is_grad_enabled():
        return _ScaledByGrad.apply(x, value, coef)
    return value


def _elem_loss(entry, x, gt, mask):
    from ..hip import check, lib, ptr, stream
    xx, g, m = _f32(x), _f32(gt), _f32(mask)
    if not (xx.numel() == g.numel() == m.numel()) or xx.numel() < 1:
        raise ValueError(f"{entry}: prediction, target and mask need the same number of elements")
    out = torch.empty((), device=xx.device)
    coef = torch.empty_like(xx)
    check(getattr(lib(), entry)(ptr(xx), ptr(g), ptr(m), xx.numel(), ptr(out), ptr(coef), stream()), entry)
    return _attach(x, out, coef)


def DurationSmoothL1Loss(input, gt, mask):
    """smooth_l1(input*mask, gt*mask, beta=1, sum) / mask.sum()  (AiR/models/loss.py:16-19)"""
    _no_grad_targets("DurationSmoothL1Loss", gt=gt, mask=mask)
    return _elem_loss("sp_smooth_l1_loss", input, gt, mask)


def MLPRayleighDistribution(Rayleigh_sigma2, gt, mask):
    """-sum_{mask==1} [log(gt/sigma2 + eps) - gt^2/(2 sigma2)] / mask.sum()  (AiR/models/loss.py:21-25)"""
    _no_grad_targets("MLPRayleighDistribution", gt=gt, mask=mask)
    return _elem_loss("sp_rayleigh_loss", Rayleigh_sigma2, gt, mask)


def _map_loss(entry, input, target, mean=True):
    from ..hip import check, lib, ptr, stream
    x, y = _rows(_f32(input)), _rows(_f32(target))
    if x.shape != y.shape:
        raise ValueError(f"{entry}: prediction {tuple(input.shape)} and target {tuple(target.shape)} differ in their rows")
    R, P = x.shape
    out = torch.empty((), device=x.device) if mean else None
    rows = torch.empty(R, device=x.device)
    coef = torch.empty_like(x)
    check(getattr(lib(), entry)(ptr(x), ptr(y), R, P, ptr(out), ptr(rows), ptr(coef), ptr(_ticket(x.device)) if mean else None, stream()),
          entry)
    return _attach(input, out if mean else rows, coef)


def NSS(input, fixation):
    """mean over rows of the fixation-weighted standardised map (AiR/models/loss.py:47-55)"""
    _no_grad_targets("NSS", fixation=fixation)
    return _map_loss("sp_nss_loss", input, fixation)


def CC(input, salmap):
    """mean over rows of Pearson's r of the sum-normalised maps (AiR/models/loss.py:57-74)"""
    _no_grad_targets("CC", salmap=salmap)
    return _map_loss("sp_cc_loss", input, salmap)


def KLD(input, salmap):
    """mean over rows of sum q log(q / (p + eps) + eps) of the sum-normalised maps (AiR/models/loss.py:104-114)"""
    _no_grad_targets("KLD", salmap=salmap)
    return _map_loss("sp_kld_loss", input, salmap)


def KLD_items(input, salmap):
    """KLD per row, [rows] (AiR/models/loss.py:116-126)"""
    _no_grad_targets("KLD_items", salmap=salmap)
    return _map_loss("sp_kld_loss", input, salmap, mean=False)


class _Compacted(torch.autograd.Function):
    """value[k] = CC of row r with idx[r] == k; backward: coef[r] * g[idx[r]] (sp_rowscale_idx)"""
    @staticmethod
    def forward(ctx, x, value, coef, idx):
        ctx.save_for_backward(coef, idx)
        ctx.shape = x.shape
        ctx.mark_non_differentiable(coef, idx)
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from ..hip import check, lib, ptr, stream
        coef, idx = ctx.saved_tensors
        out = torch.empty_like(coef)
        check(lib().sp_rowscale_idx(ptr(coef), ptr(g.detach().float().contiguous()), ptr(idx), coef.shape[0], coef.shape[1], ptr(out),
                                    stream()), "sp_rowscale_idx")
        return out.reshape(ctx.shape), None, None, None


def CC_terms(input, salmap, good_duration_masks, poor_duration_masks):
    """CC of every row whose good and poor duration masks both have a non-zero sum, [n paired] in row order; the scalar 0 when there is
    none (AiR/models/loss.py:76-98).  The paired count is read on the host (the length of the result), as the reference does."""
    from ..hip import check, lib, ptr, stream
    _no_grad_targets("CC_terms", salmap=salmap, good_duration_masks=good_duration_masks, poor_duration_masks=poor_duration_masks)
    x, y = _rows(_f32(input)), _rows(_f32(salmap))
    good, poor = _rows(_f32(good_duration_masks)), _rows(_f32(poor_duration_masks))
    R, P = x.shape
    if y.shape != x.shape or good.shape != poor.shape or good.shape[0] != R:
        raise ValueError("CC_terms: input, salmap and the two duration masks need the same rows")
    out = torch.empty(R, device=x.device)
    idx = torch.empty(R, dtype=torch.int32, device=x.device)
    count = torch.empty(1, dtype=torch.int32, device=x.device)
    coef = torch.empty_like(x)
    check(lib().sp_cc_terms(ptr(x), ptr(y), ptr(good), ptr(poor), R, P, good.shape[1], ptr(out), ptr(idx), ptr(count), ptr(coef),
                            stream()), "sp_cc_terms")
    n = int(count.item())
    if n == 0:
        return torch.zeros((), device=x.device)
    if input.requires_grad and torch.is_grad_enabled():
        return _Compacted.apply(input, out[:n], coef, idx)
    return out[:n]


class _AbsDiffMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        from ..hip import check, lib, ptr, stream
        x, y = _f32(a).reshape(-1), _f32(b).reshape(-1)
        n = x.numel()
        if y.numel() != n or n < 1:
            raise ValueError("CC_MatchLoss: the two arguments need the same number (>= 1) of elements")
        out = torch.empty((), device=x.device)
        ca, cb = torch.empty_like(x), torch.empty_like(x)
        check(lib().sp_abs_diff_mean(ptr(x), ptr(y), n, ptr(out), ptr(ca), ptr(cb), stream()), "sp_abs_diff_mean")
        ctx.save_for_backward(ca, cb)
        ctx.shapes = (a.shape, b.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from ..hip import check, lib, ptr, stream
        g = g.detach().float().contiguous()
        outs = []
        for k, (c, shape) in enumerate(zip(ctx.saved_tensors, ctx.shapes)):
            if not ctx.needs_input_grad[k]:
                outs.append(None)
                continue
            o = torch.empty_like(c)
            check(lib().sp_scale_by(ptr(c), ptr(g), c.numel(), ptr(o), stream()), "sp_scale_by")
            outs.append(o.reshape(shape))
        return tuple(outs)


def CC_MatchLoss(gt_CC, pre_CC):
    """mean |gt_CC - pre_CC|; gradient to both arguments, sign(0) = 0 (AiR/models/loss.py:100-102)"""
    return _AbsDiffMean.apply(gt_CC, pre_CC)


def KLD_visual_linguistic_alignment(input, question_objects_pos, question_objects_masks, fullAnswer_objects_pos,
                                    fullAnswer_objects_masks):
    """KLD(softmax(input[B,1,H,W] over H*W), union of the masked question and answer boxes, normalised)  (AiR/models/loss.py:128-140);
    boxes channel-last [B,H,W,M], masks [B,M]"""
    from ..hip import check, lib, ptr, stream
    _no_grad_targets("KLD_visual_linguistic_alignment", question_objects_pos=question_objects_pos,
                     question_objects_masks=question_objects_masks, fullAnswer_objects_pos=fullAnswer_objects_pos,
                     fullAnswer_objects_masks=fullAnswer_objects_masks)
    B, C, H, W = input.shape
    if C != 1:
        raise ValueError(f"KLD_visual_linguistic_alignment: input [B,1,H,W] expected, got {tuple(input.shape)}")
    z = _rows(_f32(input))
    qp, qm, ap, am = (_f32(t) for t in (question_objects_pos, question_objects_masks, fullAnswer_objects_pos, fullAnswer_objects_masks))
    if qp.shape[:3] != (B, H, W) or ap.shape[:3] != (B, H, W) or qm.shape != (B, qp.shape[3]) or am.shape != (B, ap.shape[3]):
        raise ValueError("KLD_visual_linguistic_alignment: boxes [B,H,W,M] and masks [B,M] must match the input's B, H, W")
    P = H * W
    out = torch.empty((), device=z.device)
    rows = torch.empty(B, device=z.device)
    coef = torch.empty_like(z)
    check(lib().sp_kld_box_alignment(ptr(z), ptr(qp), ptr(qm), qp.shape[3], ptr(ap), ptr(am), ap.shape[3], B, P, ptr(out), ptr(rows),
                                     ptr(coef), ptr(_ticket(z.device)), stream()), "sp_kld_box_alignment")
    return _attach(input, out, coef)


def KLD_question_aligment(input, question_objects_pos, question_objects_masks, duration_masks):
    """(the reference's spelling)  softmax of every (sample, step) map of input [B,T,H,W]; for each question object m of sample b up to the
    first zero of question_objects_masks[b], the smallest KLD_items over the steps whose duration mask is non-zero; the mean over those
    (sample, object) pairs.  The gradient goes to the chosen step only.  Raises when there is no pair, as the reference does (torch.cat of
    an empty list); one device-to-host read of the pair count.  AiR/models/loss.py:142-170."""
    from ..hip import check, lib, ptr, stream
    _no_grad_targets("KLD_question_aligment", question_objects_pos=question_objects_pos, question_objects_masks=question_objects_masks,
                     duration_masks=duration_masks)
    B, T, H, W = input.shape
    z = _f32(input).reshape(B, T, H * W)
    qp, qm, dm = _f32(question_objects_pos), _f32(question_objects_masks), _f32(duration_masks)
    M = qm.shape[1] if qm.dim() == 2 else -1
    if qp.shape != (B, H, W, M) or qm.shape != (B, M) or dm.shape != (B, T):
        raise ValueError("KLD_question_aligment: question_objects_pos [B,H,W,M], question_objects_masks [B,M] and duration_masks [B,T] "
                         "must match input [B,T,H,W]")
    out = torch.empty((), device=z.device)
    npairs = torch.empty(1, dtype=torch.int32, device=z.device)
    ssum = torch.empty(B, device=z.device)
    coef = torch.empty_like(z)
    check(lib().sp_kld_question_alignment(ptr(z), ptr(qp), ptr(qm), ptr(dm), B, T, H * W, M, ptr(out), ptr(npairs), ptr(ssum), ptr(coef),
                                          ptr(_ticket(z.device)), stream()), "sp_kld_question_alignment")
    if int(npairs.item()) == 0:
        raise RuntimeError("KLD_question_aligment: no (sample, question object) pair -- every sample's first question mask is 0 "
                           "(the reference fails in torch.cat on the empty list)")
    return _attach(input, out, coef)
