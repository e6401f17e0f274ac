"""csrc/sampling.hip on the device against the host reference tests/sampling_ref.py: every draw of sample_rows_kernel one by one
(the generator is a public contract, so nothing here is a frequency), the durations in the log domain, the seed derivation of
Sampling.random_sample, generate_scanpath away from the 40x30 golden, and beam search at its limits."""
import math

import numpy as np
import pytest
import torch

import sampling_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

E = 2.0 ** -23                                   # one ulp of float32, relative (upper bound)
LIB_ULP = 2.0                                    # logf / sqrtf / cosf / expf of the device library: the 2-ulp figure common.h relies on
R_MAX = math.sqrt(2 * 25 * math.log(2))          # sqrt(-2 ln u) <= sqrt(-2 ln 2^-25) = 5.887: the smallest u01 is 2^-25


def log_duration_tolerance(mu, sigma2, eps):
    """Bound on |ln(duration_f32) - (eps * sigma2 + mu)| from the float32 chain of the kernel, e = 2^-23:
        L   = logf(u1)                        relative LIB_ULP e;  -2 * L is exact
        r   = sqrtf(-2 L)                     relative (LIB_ULP / 2 + LIB_ULP) e = 3 e
        th  = fl(fl(2 pi) * u2)               relative (0.23 + 0.5) e <= e, th < 2 pi: absolute 2 pi e
        c   = cosf(th)                        absolute 2 pi e (|sin| <= 1) + LIB_ULP e |c|
        eps = fl(r * c)                       absolute r * 2 pi e + (3 + LIB_ULP + 0.5) e |eps|, and r <= R_MAX
        z   = eps * sigma2 + mu               sigma2 * d_eps + 0.5 e |eps| sigma2 (product; absent when fused)
                                                + 0.5 e (|eps| sigma2 + |mu|) (sum)
        d   = expf(z)                         relative LIB_ULP e, i.e. LIB_ULP e in the log domain
    plus 1 % for the second-order terms.  With sigma2 = 0 this is (0.5 |mu| + 2) e: exp(mu) to float32 rounding."""
    d_eps = R_MAX * 2 * math.pi * E + (1.5 * LIB_ULP + LIB_ULP + 0.5) * E * np.abs(eps)
    d_z = sigma2 * d_eps + E * np.abs(eps) * sigma2 + 0.5 * E * np.abs(mu)
    return 1.01 * (d_z + LIB_ULP * E)


def _launch(p, mu, s2, min_length, seed):
    """sp_sample_actions with a raw 64-bit seed, as models/sampling.py calls it"""
    from scanpaths_amd import hip
    from scanpaths_amd.hip import check, ptr
    B, T, A = p.shape
    probs = p if torch.is_tensor(p) else torch.from_numpy(p).to(DEV)
    mu_d, s2_d = torch.from_numpy(mu).to(DEV), torch.from_numpy(s2).to(DEV)
    actions = torch.full((B, T), -7, dtype=torch.int64, device=DEV)
    aprob = torch.full((B, T), -1.0, dtype=torch.float32, device=DEV)
    dur = torch.full((B, T), float("nan"), dtype=torch.float32, device=DEV)
    check(hip.lib().sp_sample_actions(ptr(probs), ptr(mu_d), ptr(s2_d), B, T, A, int(min_length), int(seed), ptr(actions), ptr(aprob),
                                      ptr(dur), hip.stream()), "sp_sample_actions")
    torch.cuda.synchronize()
    return actions.cpu().numpy().reshape(-1), aprob.cpu().numpy().reshape(-1), dur.cpu().numpy().reshape(-1)


def _mu_s2(n, seed):
    """mu in [-3, 1], sigma2 in [0.05, 2], every 16th row sigma2 = 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    mu = rng.uniform(-3, 1, n).astype(np.float32)
    s2 = rng.uniform(0.05, 2, n).astype(np.float32)
    s2[::16] = 0
    return mu, s2


def _check_draws(p, T, min_length, seed, actions, aprob):
    """every action is one the fp64 inverse CDF accepts; the probability is p[chosen] of the UNMASKED row, bit for bit"""
    rows = p.reshape(-1, p.shape[-1])
    n = rows.shape[0]
    ok = R.acceptable_mask(rows, R.lo_of_rows(n, T, min_length), R.row_uniforms(n, seed)[0])
    assert ((actions >= 0) & (actions < rows.shape[1])).all()
    good = ok[np.arange(n), actions]
    bad = np.flatnonzero(~good)
    assert good.all(), [(int(r), int(actions[r]), np.flatnonzero(ok[r])[:4].tolist()) for r in bad[:8]]
    assert np.array_equal(aprob.view(np.uint32), rows[np.arange(n), actions].view(np.uint32))
    return float((ok.sum(1) == 1).mean())


def _check_durations(mu, s2, seed, dur):
    want, eps = R.durations(mu, s2, seed)
    assert np.isfinite(dur).all() and (dur > 0).all()
    err = np.abs(np.log(dur.astype(np.float64)) - np.log(want))
    tol = log_duration_tolerance(mu.astype(np.float64), s2.astype(np.float64), eps)
    worst = int(np.argmax(err / tol))
    print(f"durations: max |d ln| {err.max():.3e}, max err/tol {err[worst] / tol[worst]:.3f} (tol there {tol[worst]:.3e})")
    assert (err <= tol).all(), (worst, err[worst], tol[worst])
    return err, tol


@pytest.mark.parametrize("A,min_length,seed", R.parity_cases())
def test_every_draw_is_an_acceptable_inverse_cdf_answer(A, min_length, seed):
    p = R.make_case(A)
    T = p.shape[1]
    mu, s2 = _mu_s2(R.CASE_ROWS, A)
    actions, aprob, dur = _launch(p, mu, s2, min_length, seed)
    share = _check_draws(p, T, min_length, seed, actions, aprob)
    print(f"A={A} min_length={min_length} seed={seed}: single-answer share {share:.4f}")
    assert share >= 0.8
    a = actions.reshape(-1, T)
    lo = R.lo_of_rows(T, T, min_length)
    assert (a[2] == A - 1).all() and (a[3] == 1).all()           # all mass on one entry
    assert (a[5] == lo).all()                                    # no allowed mass: the first allowed action
    _check_durations(mu, s2, seed, dur)                          # finite on the rows without mass as well


def test_segment_end_draws_go_to_the_next_positive_entry():
    """The (seed, row) pairs of tests/test_sampling_ref_cpu.py, each seed in its own launch.  At these draws the serial fine scan ends
    its segment an ulp short of the target the coarse scan accepted; the draw belongs to the next positive entry (before the
    segment-end rule: the row's last positive entry, action A - 1)."""
    row = R.trap_row()
    traps = R.committed_traps()
    assert len(traps) >= 8
    B, T, A = R.TRAP_ROWS // R.TRAP_T, R.TRAP_T, R.TRAP_A
    p = np.ascontiguousarray(np.broadcast_to(row, (B, T, A)))
    p_dev = torch.from_numpy(p).to(DEV)
    mu, s2 = _mu_s2(R.TRAP_ROWS, 5)
    by_seed = {}
    for seed, r in traps:
        by_seed.setdefault(seed, []).append(r)
    wrong, launches = [], []
    for seed, rows in by_seed.items():
        actions, aprob, _ = _launch(p_dev, mu, s2, 0, seed)
        launches.append((seed, actions, aprob))
        u = R.row_uniforms(R.TRAP_ROWS, seed)[0]
        for r in rows:
            ok = R.acceptable_actions(row, r % T, 0, u[r])
            print(f"trap seed={seed} row={r}: chosen {int(actions[r])}, acceptable {ok.tolist()}")
            if int(actions[r]) not in ok:
                wrong.append((seed, r, int(actions[r]), ok.tolist()))
    print(f"{len(traps)} trap draws in {len(by_seed)} launches, {len(wrong)} wrong")
    assert not wrong, wrong
    for seed, actions, aprob in launches:                        # and every other row of each launch
        _check_draws(p, T, 0, seed, actions, aprob)


def test_durations_match_the_fp64_box_muller_reference():
    n = R.CASE_ROWS
    p = R.make_case(7)
    rng = np.random.Generator(np.random.PCG64(77))
    mu = rng.uniform(-3, 1, n).astype(np.float32)
    s2 = rng.uniform(0.05, 2, n).astype(np.float32)
    mu[:4], s2[:4] = (-3, 1, -3, 1), (0.05, 0.05, 2, 2)          # the corners of the range
    zero = np.arange(n) % 8 == 5
    s2[zero] = 0
    for seed in (9, 2 ** 64 - 1):
        _, _, dur = _launch(p, mu, s2, 1, seed)
        _check_durations(mu, s2, seed, dur)
        # sigma2 = 0: exp(mu) to float32 rounding -- 0 * eps and the sum are exact, expf alone rounds
        ref0 = np.abs(np.log(dur[zero].astype(np.float64)) - mu[zero].astype(np.float64))
        assert zero.sum() == n // 8 and (ref0 <= 1.01 * LIB_ULP * E).all(), ref0.max()


def test_random_sample_seed_derivation_and_scanpath_length():
    from scanpaths_amd.models.sampling import Sampling
    A, seed0 = 257, 12345
    p = R.make_case(A)
    B, T, _ = p.shape
    mu, s2 = _mu_s2(B * T, 1)
    probs = torch.from_numpy(p).to(DEV)
    mu_d, s2_d = torch.from_numpy(mu).view(B, T).to(DEV), torch.from_numpy(s2).view(B, T).to(DEV)
    s = Sampling(convLSTM_length=T, min_length=1, seed=seed0)
    outs = [s.random_sample(probs, mu_d, s2_d) for _ in range(2)]
    for calls, out in enumerate(outs, start=1):
        seed = (seed0 * 0x9E3779B97F4A7C15 + calls) % 2 ** 64     # rank 0
        acts = out["selected_actions"].cpu().numpy()
        assert out["selected_actions"].dtype == torch.int64 and acts.shape == (B, T)
        _check_draws(p, T, 1, seed, acts.reshape(-1), out["selected_actions_probs"].cpu().numpy().reshape(-1))
        _check_durations(mu, s2, seed, out["durations"].cpu().numpy().reshape(-1))
        ra, rp, rd = _launch(p, mu, s2, 1, seed)                  # the same launch with the seed spelled out
        assert np.array_equal(ra, acts.reshape(-1)) and np.array_equal(rd, out["durations"].cpu().numpy().reshape(-1))
        assert out["scanpath_length"].shape == (B, 1)
        assert np.array_equal(out["scanpath_length"].cpu().numpy()[:, 0], R.scanpath_length(acts, T))
    a1, a2 = (o["selected_actions"].cpu().numpy() for o in outs)
    assert (a1 != a2).mean() > 0.5                                # the second call draws another stream
    again = Sampling(convLSTM_length=T, min_length=1, seed=seed0).random_sample(probs, mu_d, s2_d)
    for k in ("selected_actions", "selected_actions_probs", "durations", "scanpath_length"):
        assert torch.equal(again[k], outs[0][k]), k


def _reference_generate_scanpath(sample_actions, drts, map_width, map_height, width, height):
    """models/sampling.py:55-75 of the reference in numpy float64"""
    x_granularity, y_granularity = float(width / map_width), float(height / map_height)
    N, T = sample_actions.shape
    action_masks, duration_masks = np.zeros((N, T)), np.zeros((N, T))
    vectors = []
    for index in range(N):
        sample_action = sample_actions[index]
        fix_vector = []
        for order in range(sample_action.shape[0]):
            if sample_action[order] == 0:
                action_masks[index, order] = 1
                break
            else:
                image_index = sample_action[order] - 1
                map_pos_x = image_index % map_width
                map_pos_y = image_index // map_width
                pos_x = map_pos_x * x_granularity + x_granularity / 2
                pos_y = map_pos_y * y_granularity + y_granularity / 2
                action_masks[index, order] = 1
                duration_masks[index, order] = 1
                fix_vector.append((pos_x, pos_y, drts[index, order]))
        vectors.append(np.array(fix_vector, dtype=np.float64).reshape(-1, 3))
    return vectors, action_masks, duration_masks


@pytest.mark.parametrize("mw,mh,w,h", [(64, 40, 512, 320), (32, 20, 512, 320), (13, 7, 100, 50)])
def test_generate_scanpath_on_other_grids(mw, mh, w, h):
    from scanpaths_amd.models.sampling import Sampling
    T, last = 6, mw * mh
    rng = np.random.Generator(np.random.PCG64(mw))
    acts = rng.integers(1, last + 1, (40, T))
    acts[0, :2] = (1, last)                                      # first and last cell, no terminate
    acts[1, 0] = 0                                               # terminate at t = 0 (cells after it are ignored)
    acts[2, T - 1] = 0                                           # terminate at t = T - 1
    acts[3] = (last, 1, 0, 5, 0, 2)
    acts[4] = 0
    acts[5] = np.arange(mw - 1, mw + T - 1)                      # across the end of the first map row
    acts[8:, 1:][rng.random((32, T - 1)) < 0.2] = 0
    durs = rng.uniform(0.05, 1.5, (40, T)).astype(np.float32)
    s = Sampling(convLSTM_length=T, min_length=1, map_width=mw, map_height=mh, width=w, height=h)
    fix, am, dm = s.generate_scanpath(torch.zeros(40, 3, 2, 2, device=DEV), None, torch.from_numpy(durs).to(DEV),
                                      torch.from_numpy(acts).to(DEV))
    want, wam, wdm = _reference_generate_scanpath(acts, durs, mw, mh, w, h)
    assert np.array_equal(am.cpu().numpy(), wam) and np.array_equal(dm.cpu().numpy(), wdm)
    length, _, _, _, nfix = s._scan(torch.from_numpy(acts).to(DEV), torch.from_numpy(durs).to(DEV))
    assert [int(x) for x in nfix.cpu()] == [len(v) for v in want] == [len(f) for f in fix]
    assert np.array_equal(length.cpu().numpy(), R.scanpath_length(acts, T))
    dyadic = (w / mw).is_integer() and (h / mh).is_integer() and math.log2(w / mw).is_integer() and math.log2(h / mh).is_integer()
    worst = 0.0
    for f, v in zip(fix, want):
        got = np.stack([f["start_x"], f["start_y"]], 1).reshape(-1, 2)
        assert np.array_equal(f["duration"], v[:, 2])            # the float32 duration, widened
        if dyadic:
            assert np.array_equal(got, v[:, :2])
        elif len(v):
            rel = np.abs(got - v[:, :2]) / v[:, :2]
            worst = max(worst, float(rel.max()))
    print(f"map {mw}x{mh} on {w}x{h}: dyadic {dyadic}, worst relative position error {worst:.3e} (bound {2.0 ** -23:.3e})")
    assert worst <= 2.0 ** -23                                   # float32 granularity in the kernel, float64 in the reference


def _beam_case(name):
    rng = np.random.Generator(np.random.PCG64(31))
    if name == "A2":                                             # A = 2: one allowed entry while terminate is masked
        p = rng.random((4, 6, 2)).astype(np.float32) + 0.05
        p[1, :, 1] = 0                                           # only terminate is positive: no sequence survives min_length
        p[2, 3:, 0] = 0
        ml = 2
    elif name == "A5":                                           # A = 5 with three positive entries: fewer than K = 8
        p = rng.random((4, 6, 5)).astype(np.float32) + 0.05
        p[:, :, (2, 4)] = 0
        p[2, :, :3] = 0                                          # one positive entry: one sequence, the other beams stay unused
        p[3, :, 0] = 0
        ml = 1
    elif name == "T64":
        p = rng.random((2, 64, 300)).astype(np.float32) ** 6
        p[0, :, 0] = 0                                           # never terminates: every beam lives through all 64 steps
        ml = 2
    elif name in ("ml=T", "ml>T"):
        p = rng.random((3, 8, 5)).astype(np.float32) + 0.05
        p[1, 4, 1:] = 0                                          # a step without an allowed positive entry: every beam dies
        ml = 8 if name == "ml=T" else 11
    else:                                                        # exact ties: inside one 256-stride, and one stride apart
        p = rng.random((3, 5, 600)).astype(np.float32) ** 4
        p[0, 2, 300] = p[0, 2, 310] = p[0, 2].max() * 2
        p[1, 1, 20] = p[1, 1, 276] = p[1, 1].max() * 2
        p[2, 0, 1] = p[2, 0, 255] = p[2, 0, 257] = p[2, 0].max() * 2
        ml = 1
    p /= p.sum(-1, keepdims=True)
    return p.astype(np.float32), ml


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("name", ["A2", "A5", "T64", "ml=T", "ml>T", "ties"])
def test_beam_search_at_its_limits(name, K):
    from oracle import sampling_oracle as SO
    from scanpaths_amd.models.sampling import Sampling
    p, ml = _beam_case(name)
    B, T, A = p.shape
    probs = torch.from_numpy(p).to(DEV)
    out = Sampling(convLSTM_length=T, min_length=ml).beam_search(probs, torch.zeros(B, T, device=DEV), torch.ones(B, T, device=DEV), beam=K)
    acts, scores = out["selected_actions"].cpu().numpy(), out["scores"].cpu().numpy()
    assert acts.shape == (B, K, T) and scores.shape == (B, K)
    unused = 0
    for b in range(B):
        wa, ws = SO.beam_search(p[b], ml, K)
        assert np.array_equal(acts[b], wa), (name, K, b)
        dead = np.isneginf(ws)
        assert np.array_equal(np.isneginf(scores[b]), dead) and (acts[b][dead] == 0).all()
        assert np.allclose(scores[b][~dead], ws[~dead], rtol=0, atol=1e-9)
        unused += int(dead.sum())
    if name in ("A2", "A5") and K == 8:
        assert unused > 0                                        # the case really runs out of candidates
    if name in ("ml=T", "ml>T"):
        assert (acts[0] != 0).all() and np.isneginf(scores[1]).all()     # nothing may terminate; sample 1 dies at step 4
