"""Golden vectors for the attention-map losses and the saliency / scanpath metrics from the REAL reference
(AiR/models/loss.py:16-25, 47-170 and AiR/utils/evaltools/visual_attention_metrics.py:41-232, 332-476), CPU only:

    python tests/golden/make_golden_salmaps.py

matplotlib and tqdm are stubbed.  The cv2 shim allows only an equal-shape resize and returns a copy (what OpenCV does for an equal
size); the mismatched-shape branch is out of scope.  np.trapz is aliased to np.trapezoid where NumPy lacks it.  Every loss runs in
fp64 and in fp32 (values and autograd input gradients; a seeded weight vector turns a per-row result into a scalar for backward).
Jittered AUC-Judd calls are preceded by np.random.seed(k).  Writes tests/golden/salmaps.npz (+ shards), numeric arrays only:
False / None results of the reference are NaN with a flag array."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SCANPATHS_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
from helpers import save_npz  # noqa: E402

for name in ("matplotlib", "matplotlib.pyplot", "tqdm", "cv2"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.modules["tqdm"].tqdm = lambda x, *a, **k: x


def _resize(src, dsize, interpolation=None):
    src = np.asarray(src)
    if (src.shape[1], src.shape[0]) != tuple(dsize):
        raise NotImplementedError("cv2 shim: only an equal-shape resize")
    return src.copy()


sys.modules["cv2"].resize = _resize
sys.modules["cv2"].INTER_CUBIC = 2
if not hasattr(np, "trapz"):
    np.trapz = np.trapezoid
sys.path.insert(0, os.path.join(REF, "AiR"))
import models.loss as RL  # noqa: E402
import utils.evaltools.visual_attention_metrics as RM  # noqa: E402

def _cases(g):
    """(name, reference function, [args], indices of the differentiable args, length of the weight vector of a per-row result or 0)"""
    # inputs on a 1/256 grid: exact in fp32 (both runs see the same numbers) and small once compressed
    def pos(*shape):
        return torch.from_numpy(g.integers(13, 257, shape) / 256.0)

    def logits(*shape):
        return torch.from_numpy(g.integers(-640, 641, shape) / 256.0)

    def binary(*shape, p=0.05):
        return torch.from_numpy((g.uniform(size=shape) < p).astype(np.float64))

    def boxes(B, H, W, M):
        out = np.zeros((B, H, W, M))
        for b in range(B):
            for m in range(M):
                y0, x0 = g.integers(0, H - 4), g.integers(0, W - 4)
                out[b, y0:y0 + g.integers(3, H // 2), x0:x0 + g.integers(3, W // 2), m] = 1.0
        return torch.from_numpy(out)

    c = []
    m36 = torch.from_numpy((g.uniform(size=(3, 6)) < 0.7).astype(np.float64))
    m36[2] = 0
    m36[0, 0] = 1
    c.append(("smoothl1_3x6", RL.DurationSmoothL1Loss, [logits(3, 6), logits(3, 6), m36], [0], 0))
    c.append(("rayleigh_3x6", RL.MLPRayleighDistribution, [pos(3, 6) * 2, pos(3, 6) * 3, m36], [0], 0))
    c.append(("rayleigh_1x1", RL.MLPRayleighDistribution, [pos(1, 1), pos(1, 1), torch.ones(1, 1, dtype=torch.float64)], [0], 0))
    for tag, shape in (("1x30x40", (1, 30, 40)), ("6x30x40", (6, 30, 40)), ("3x40x64", (3, 40, 64)), ("1x240x320", (1, 240, 320))):
        fix = binary(*shape, p=0.02)
        fix.view(shape[0], -1)[:, 7] = 1.0
        c.append((f"nss_{tag}", RL.NSS, [pos(*shape), fix], [0], 0))
        c.append((f"kld_{tag}", RL.KLD, [pos(*shape), pos(*shape) * binary(*shape, p=0.5)], [0], 0))
        if shape[1] < 240:                                            # one 240x320 row each for NSS and KLD keeps the fixture small
            c.append((f"cc_{tag}", RL.CC, [pos(*shape), pos(*shape)], [0], 0))
            c.append((f"klditems_{tag}", RL.KLD_items, [pos(*shape), pos(*shape)], [0], shape[0]))
    good = torch.from_numpy((g.uniform(size=(3, 6)) < 0.6).astype(np.float64))
    poor = torch.from_numpy((g.uniform(size=(3, 6)) < 0.6).astype(np.float64))
    good[0, 0] = poor[0, 0] = good[2, 1] = poor[2, 1] = 1
    good[1] = 0                                                       # a row whose duration mask is all zero: not paired
    c.append(("ccterms_3x30x40", RL.CC_terms, [pos(3, 30, 40), pos(3, 30, 40), good, poor], [0], 2))
    c.append(("ccterms_none", RL.CC_terms, [pos(2, 30, 40), pos(2, 30, 40), torch.zeros(2, 6, dtype=torch.float64),
                                            torch.ones(2, 6, dtype=torch.float64)], [], 0))
    c.append(("ccmatch_5", RL.CC_MatchLoss, [logits(5) / 2.5, logits(5) / 2.5], [0, 1], 0))
    B, H, W, M = 3, 30, 40, 5
    qm = torch.tensor([[1, 1, 0, 1, 1], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0]], dtype=torch.float64)
    am = torch.tensor([[1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=torch.float64)
    c.append(("kldvla_3x30x40", RL.KLD_visual_linguistic_alignment, [logits(B, 1, H, W), boxes(B, H, W, M), qm, boxes(B, H, W, M), am],
              [0], 0))
    dm = torch.ones(B, 6, dtype=torch.float64)
    dm[0, 4:] = 0
    dm[2, 0] = 0
    c.append(("kldqa_3x6x30x40", RL.KLD_question_aligment, [logits(B, 6, H, W), boxes(B, H, W, M), qm, dm], [0], 0))
    c.append(("kldqa_1x1x40x64", RL.KLD_question_aligment, [logits(1, 1, 40, 64), boxes(1, 40, 64, M),
                                                            torch.tensor([[1, 1, 1, 0, 1]], dtype=torch.float64),
                                                            torch.ones(1, 1, dtype=torch.float64)], [0], 0))
    dz = dm.clone()
    dz[1] = 0                                                         # every step of sample 1 masked: its pairs are +inf
    c.append(("kldqa_inf_3x6x30x40", RL.KLD_question_aligment, [logits(B, 6, H, W), boxes(B, H, W, M), qm, dz], [0], 0))
    return c


def run_loss(fn, args, diff, nw, dtype, w):
    a = [t.to(dtype).clone().requires_grad_(i in diff) for i, t in enumerate(args)]
    out = fn(*a)
    val = out.detach().numpy().astype(np.float64)
    grads = []
    if diff:
        s = (out * w.to(dtype)).sum() if nw else out
        gs = torch.autograd.grad(s, [a[i] for i in diff])
        grads = [x.numpy().astype(np.float64) for x in gs]
    return val, grads


def losses(out):
    g = np.random.Generator(np.random.PCG64(20261016))
    for name, fn, args, diff, nw in _cases(g):
        w = torch.from_numpy(g.uniform(0.5, 1.5, nw)) if nw else torch.ones(1, dtype=torch.float64)
        for i, t in enumerate(args):
            out[f"loss/{name}/in{i}"] = t.numpy().astype(np.float32)
        out[f"loss/{name}/w"] = w.numpy()
        out[f"loss/{name}/diff"] = np.array(diff, dtype=np.int64)
        v64, g64 = run_loss(fn, args, diff, nw, torch.float64, w)
        v32, g32 = run_loss(fn, args, diff, nw, torch.float32, w)
        # the bar of a test is max(10 |ref32 - ref64|, 1e-4 |ref64|): the fp64 gradient is kept in fp32 (1e-7 relative, far below
        # that bar) and of the fp32 run only its error norm
        out[f"loss/{name}/val64"], out[f"loss/{name}/val32"] = v64, v32
        for i, a, b in zip(diff, g64, g32):
            out[f"loss/{name}/grad64_{i}"] = a.astype(np.float32)
            out[f"loss/{name}/grad64norm_{i}"] = np.float64(np.linalg.norm(a))
            out[f"loss/{name}/err32_{i}"] = np.float64(np.linalg.norm(b - a))


def metrics(out):
    g = np.random.Generator(np.random.PCG64(777))
    maps = []

    def sparse(shape, n):
        f = np.zeros(shape)
        f.reshape(-1)[g.choice(f.size, n, replace=False)] = 1.0
        return f

    maps.append((g.uniform(0, 1, (30, 40)), sparse((30, 40), 12)))
    maps.append((g.uniform(0, 1, (40, 64)) ** 3, sparse((40, 64), 30)))
    maps.append((g.uniform(0, 1, (30, 40)), np.zeros((30, 40))))                           # no fixation
    maps.append((np.full((30, 40), 0.25), sparse((30, 40), 5)))                           # constant map
    f = np.zeros((30, 40))
    f[3, 4], f[10, 20] = -1.0, -2.0
    maps.append((g.uniform(0, 1, (30, 40)), f))                                           # non-zero but no positive fixation
    f = sparse((30, 40), 20) * g.choice([0.5, 2.0], (30, 40))
    f[0, 0] = -1.0
    maps.append((g.uniform(0, 1, (30, 40)), f))                                           # non-binary fixation map
    maps.append((np.round(g.uniform(0, 4, (30, 40))), sparse((30, 40), 40)))             # many ties in the map
    maps.append((g.integers(0, 4096, (240, 320)) / 4096.0, sparse((240, 320), 3000)))                 # Nfix beyond the LDS limit
    maps.append((np.zeros((30, 40)), sparse((30, 40), 6)))                                 # all-zero map
    shapes = np.array([m[0].shape for m in maps], dtype=np.int64)
    auc_j, auc_n, nss, kld = [], [], [], []
    for k, (s, f) in enumerate(maps):
        out[f"metric/{k}/sal"], out[f"metric/{k}/fix"] = s, f
        np.random.seed(k)
        with np.errstate(all="ignore"):
            auc_j.append(RM.AUC_Judd(s, f, jitter=True))
            auc_n.append(RM.AUC_Judd(s, f, jitter=False))
            nss.append(RM.NSS(s, f))
            kld.append(RM.KLdiv(s, f))
    out["metric_shapes"] = shapes
    out["metric_auc_jitter"], out["metric_auc"] = np.array(auc_j, dtype=np.float64), np.array(auc_n, dtype=np.float64)
    out["metric_nss"], out["metric_kld"] = np.array(nss, dtype=np.float64), np.array(kld, dtype=np.float64)


def scanpaths(out):
    g = np.random.Generator(np.random.PCG64(4242))
    lens = [0, 1, 2, 3, 5, 5, 8, 12, 20, 12]
    fixs = [np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(50, 900, n)], 1) for n in lens]
    cat = np.concatenate(fixs, 0)
    off = np.zeros(len(fixs) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    out["tde_fix"], out["tde_off"] = cat, off
    n = len(fixs)
    img = np.zeros((240, 320, 3))

    def num(v):
        return np.nan if (v is False or v is None) else float(v)

    def flag(v):
        return 1 if v is False else (2 if v is None else 0)

    res = {}
    for key, f in [("eucl", lambda a, b: RM.euclidean_distance(a, b)),
                   ("tde_k1", lambda a, b: RM.time_delay_embedding_distance(a, b, k=1)),
                   ("tde_k3", lambda a, b: RM.time_delay_embedding_distance(a, b, k=3)),
                   ("tde_k3_haus", lambda a, b: RM.time_delay_embedding_distance(a, b, k=3, distance_mode='Hausdorff')),
                   ("tde_k5_haus", lambda a, b: RM.time_delay_embedding_distance(a, b, k=5, distance_mode='Hausdorff')),
                   ("tde_k2_bad", lambda a, b: RM.time_delay_embedding_distance(a, b, k=2, distance_mode='Median')),
                   ("stdd", lambda a, b: RM.scaled_time_delay_embedding_distance(a.copy(), b.copy(), img))]:
        vals = [[f(fixs[i], fixs[j]) for j in range(n)] for i in range(n)]
        res[key] = vals
        out[f"tde/{key}"] = np.array([[num(v) for v in r] for r in vals], dtype=np.float64)
        out[f"tde/{key}_flag"] = np.array([[flag(v) for v in r] for r in vals], dtype=np.int64)


def main():
    torch.set_num_threads(1)
    out = {}
    losses(out)
    metrics(out)
    scanpaths(out)
    save_npz(os.path.join(HERE, "salmaps.npz"), out)
    print(f"{len(out)} arrays; losses {sum(k.endswith('/val64') for k in out)}; AUC {out['metric_auc_jitter']}; NSS {out['metric_nss']}")


if __name__ == "__main__":
    main()
