"""csrc/scanlik.hip through evaltools.scanpath_likelihood, the C entry point, the keyed evaluation, its table and the loop, against
the plain-loop restatement tests/scanpath_likelihood_ref.py.

The bar.  AUC, n, dropped and the NaN / -inf pattern of every output are integers or exact and must be EQUAL.  LL, IG, NSS, DLL, CONT,
TERM and STOP must stay within 1e-12 * max(1, |ref|): the restatement sums serially, the device lane-strided with a butterfly, and the
two log2 implementations may differ in the last bit -- the bar tests/test_saliency_ext_gpu.py uses for IG, for the same reason.  Serial
against lane-strided-plus-butterfly summation of such maps differ by at most 2e-15 relative in LL, NSS and Z (400 maps, on the CPU), so
the bar leaves a factor of about 500.  Every test prints the worst error per metric; measured on an MI355X: LL 5.2e-16,
IG 1.8e-15, NSS 5.8e-15, DLL 9.6e-16, STOP 3.2e-16, CONT 1.6e-16, TERM 1.9e-16.

Shapes: maps 3x5 (P = 15, below one wave), 8x8 (64), 5x13 (65), 30x40 (1200: a tail slot) and 32x64 (2048: the limit); T = 1, 4, 16;
R = 6; 32 scanpaths.  The issue's list asks both for S <= 40 and for a row with more than 64 scanpaths: the latter has a test of its
own with 70 one-fixation scanpaths."""
import numpy as np
import pytest
import torch

import scanpath_likelihood_ref as R

pytestmark = pytest.mark.gpu
MAPS = {(3, 5): (30.0, 50.0), (8, 8): (37.0, 53.0), (5, 13): (240.0, 320.0), (30, 40): (240.0, 320.0), (32, 64): (240.5, 320.25)}
MIX = {1: 0.01, 4: 0.0, 16: 0.05}
FLOAT_METRICS = ("LL", "IG", "NSS", "DLL", "STOP", "CONT", "TERM")
_CASES = {}


def M():
    from scanpaths_amd.utils.evaltools import scanpath_likelihood
    return scanpath_likelihood


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def softmax(g, scale, T, A):
    z = g.normal(0, scale, (T, A))
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def make_probs(g, T, A):
    """six rows: scale 0.5 and unnormalised; scale 3; scale 8 with exact zeros (and p_0 = 0 at step 0); scale 3 quantised to multiples of
    2^-10 (ties); exactly constant; scale 3 (the row that gets no scanpaths)"""
    p = np.stack([softmax(g, 0.5, T, A) * np.float32(3.7), softmax(g, 3, T, A), softmax(g, 8, T, A),
                  np.round(softmax(g, 3, T, A) * 1024) / 1024, np.full((T, A), 1.0 / A), softmax(g, 3, T, A)]).astype(np.float32)
    p[2][g.random((T, A)) < 0.25] = 0.0
    p[2, 0, 0] = 0.0
    p[2, :, 1] = np.maximum(p[2, :, 1], np.float32(1e-3))               # never an all-zero map
    return p


def case(shape, T):
    """(probs, scanpaths, rows, frame, baseline, baseline_rows, mu, sigma2) and the restatement's result, built once per shape"""
    if (shape, T) in _CASES:
        return _CASES[shape, T]
    Hm, Wm = shape
    h, w = MAPS[shape]
    P = Hm * Wm
    g = np.random.default_rng(1000 * P + T)
    probs = make_probs(g, T, 1 + P)

    def path(n):
        return np.stack([g.uniform(0, w, n), g.uniform(0, h, n), g.uniform(0.05, 0.8, n)], 1)

    paths, rows = [], []
    for r in range(5):                                                   # row 5 gets none
        for n in (0, 1, max(T - 1, 0), T, T + 3):
            paths.append(path(n))
            rows.append(r)
    # first fixations on a cell border, a corner of four cells, the frame's last pixel, just inside the frame, x = w exactly, negative, NaN
    special = [(3 * w / Wm, h / 3), (2 * w / Wm, 2 * h / Hm), (w - 1.0, h - 1.0), (np.nextafter(w, 0), np.nextafter(h, 0)), (w, h / 2),
               (w / 2, -0.25), (np.nan, h / 2)]
    for k, (x, y) in enumerate(special):
        sp = path(T + 1)
        sp[0, :2] = x, y
        paths.append(sp)
        rows.append(k % 5)
    paths[3][0, 2], paths[8][0, 2], paths[13][0, 2], paths[18][0, 2] = 0.0, -0.1, np.nan, np.inf     # durations without a density
    perm = g.permutation(len(paths))                                     # rows come shuffled
    paths, rows = [paths[i] for i in perm], [rows[i] for i in perm]
    baseline = g.uniform(0, 1, (3, P))
    baseline[1][g.random(P) < 0.3] = 0.0
    baseline[2] = 0.0                                                    # a row without mass: NaN
    brows = g.integers(0, 3, len(paths))
    mu = g.normal(-1.2, 0.5, (6, T)).astype(np.float32)
    s2 = g.uniform(0.05, 1.5, (6, T)).astype(np.float32)
    s2[1, 0] = 0.0
    c = dict(probs=probs, paths=paths, rows=rows, frame=(h, w), shape=shape, baseline=baseline, brows=brows, mu=mu, s2=s2, T=T,
             u=MIX[T], min_length=2)
    c["ref"] = R.scanpath_likelihood(probs, paths, rows, (h, w), shape, c["u"], baseline, brows, mu, s2, c["min_length"])
    _CASES[shape, T] = c
    return c


def call(c, keep=None, metrics=R.METRICS, **kw):
    keep = range(len(c["paths"])) if keep is None else keep
    return M().scanpath_likelihood(torch.from_numpy(c["probs"]).to(dev()), [c["paths"][i] for i in keep], [c["rows"][i] for i in keep],
                                   c["frame"], uniform_mix=c["u"], metrics=metrics, map_shape=c["shape"],
                                   baseline=torch.from_numpy(c["baseline"]).to(dev()), baseline_rows=c["brows"][list(keep)],
                                   log_normal_mu=torch.from_numpy(c["mu"]).to(dev()),
                                   log_normal_sigma2=torch.from_numpy(c["s2"]).to(dev()), min_length=c["min_length"], **kw)


def close(got, want, what, names):
    """equal pattern of NaN / inf, finite values within the bar; prints the worst error per name"""
    for m in names:
        a, b = np.asarray(got[m], dtype=np.float64), np.asarray(want[m], dtype=np.float64)
        assert a.shape == b.shape, (what, m, a.shape, b.shape)
        fin = np.isfinite(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, m, "NaN pattern", np.argwhere(np.isnan(a) != np.isnan(b))[:8])
        assert np.array_equal(a[~fin], b[~fin], equal_nan=True), (what, m, "inf pattern")
        err = np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))
        worst = float(err.max()) if err.size else 0.0
        print(f"{what} {m}: worst error {worst:.3g} over {int(fin.sum())} finite values, {int(np.isnan(b).sum())} NaN, "
              f"{int(np.isinf(b).sum())} inf")
        assert worst <= 1e-12, (what, m, worst)


def exact(got, want, what, names=("AUC", "n", "dropped")):
    for m in names:
        assert got[m].dtype == want[m].dtype and np.array_equal(got[m], want[m], equal_nan=True), (what, m, got[m], want[m])


@pytest.mark.parametrize("T", [1, 4, 16])
@pytest.mark.parametrize("shape", list(MAPS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_with_the_restatement(shape, T):
    c = case(shape, T)
    got = call(c)
    assert list(got) == list(R.METRICS) + ["n", "dropped"]
    what = f"{shape[0]}x{shape[1]} T={T} u={c['u']}"
    exact(got, c["ref"], what)
    close(got, c["ref"], what, ("LL", "IG", "NSS", "DLL", "STOP"))
    ref = c["ref"]
    assert ref["dropped"].sum() >= 3 and np.isnan(ref["NSS"]).sum() > np.isnan(ref["LL"]).sum()       # drops; the constant row
    assert np.isnan(ref["IG"]).sum() > np.isnan(ref["LL"]).sum()                                       # the baseline row without mass
    if c["u"] == 0.0 and T > 1:
        assert np.isinf(ref["LL"]).any() and np.isinf(ref["STOP"]).any()                               # zeros are reported as -inf


def raw(c, counts=None, want=("LL", "IG", "NSS", "AUC", "DLL", "CONT", "TERM", "dropped"), sentinel=7.0):
    """sp_scan_likelihood itself on buffers pre-filled with a sentinel; counts may lie about a scanpath (the kernel's own guard)"""
    from scanpaths_amd import hip
    L = hip.lib()
    d = dev()
    paths, T = c["paths"], c["T"]
    S, Rr = len(paths), c["probs"].shape[0]
    true = [len(p) for p in paths]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(d)
    fix = t(np.concatenate(paths, 0), np.float64)
    start, count = t(np.cumsum([0] + true[:-1]), np.int64), t(true if counts is None else counts, np.int32)
    row = np.asarray(c["rows"])
    row_n = np.bincount(row, minlength=Rr)
    rf, rn, order = t(np.cumsum(row_n) - row_n, np.int32), t(row_n, np.int32), t(np.argsort(row, kind="stable"), np.int32)
    probs, mu, s2, base, brows = t(c["probs"], np.float32), t(c["mu"], np.float32), t(c["s2"], np.float32), t(c["baseline"], np.float64), \
        t(c["brows"], np.int32)
    out = {m: torch.full((Rr * T if m in ("CONT", "TERM") else S * T,), sentinel, dtype=torch.float64, device=d) for m in want
           if m != "dropped"}
    if "dropped" in want:
        out["dropped"] = torch.full((S,), 77, dtype=torch.int32, device=d)
    o = lambda m: hip.ptr(out.get(m))
    Hm, Wm = c["shape"]
    h, w = c["frame"]
    rc = L.sp_scan_likelihood(hip.ptr(probs), hip.ptr(mu), hip.ptr(s2), hip.ptr(base), hip.ptr(brows), hip.ptr(fix), hip.ptr(start),
                              hip.ptr(count), hip.ptr(rf), hip.ptr(rn), hip.ptr(order), Rr, T, Hm, Wm, S, 3, w, h, c["u"], o("LL"),
                              o("IG"), o("NSS"), o("AUC"), o("DLL"), o("CONT"), o("TERM"), o("dropped"), hip.stream())
    hip.check(rc, "sp_scan_likelihood")
    torch.cuda.synchronize()
    return {m: v.cpu().numpy().reshape((-1, T) if m != "dropped" else (-1,)) for m, v in out.items()}


@pytest.mark.parametrize("shape", [(5, 13), (30, 40)], ids=["5x13", "30x40"])
def test_uninitialised_buffers_are_fully_overwritten_and_step_outputs(shape):
    c = case(shape, 4)
    res = raw(c)
    api = call(c)
    for m in ("LL", "IG", "NSS", "AUC", "DLL"):
        assert not (res[m] == 7.0).any(), m
        assert np.array_equal(res[m], api[m], equal_nan=True), m                 # the public call is this launch
    assert np.array_equal(res["dropped"], api["dropped"]) and not (res["dropped"] == 77).any()
    close(res, c["ref"], f"raw {shape}", ("CONT", "TERM"))
    assert res["TERM"][2, 0] == -np.inf and res["CONT"][2, 0] == 0.0             # p_0 = 0: the step cannot terminate
    # any subset of the outputs: the others are not touched, the values do not change
    some = raw(c, want=("NSS", "TERM"))
    assert set(some) == {"NSS", "TERM"} and np.array_equal(some["NSS"], res["NSS"], equal_nan=True) and \
        np.array_equal(some["TERM"], res["TERM"], equal_nan=True)


def test_the_kernel_guards_itself():
    """a count of 65 (and a negative one): NaN everywhere for that scanpath, dropped 0, the others unchanged"""
    c = case((8, 8), 4)
    good = raw(c)
    counts = [len(p) for p in c["paths"]]
    lie = [k for k, n in enumerate(counts) if n >= 4][:2]
    counts[lie[0]], counts[lie[1]] = 65, -1
    res = raw(c, counts)
    rest = [k for k in range(len(counts)) if k not in lie]
    for m in ("LL", "IG", "NSS", "AUC", "DLL"):
        assert np.isnan(res[m][lie]).all(), m
        assert np.array_equal(res[m][rest], good[m][rest], equal_nan=True), m
    assert (res["dropped"][lie] == 0).all() and np.array_equal(res["dropped"][rest], good["dropped"][rest])
    assert np.array_equal(res["CONT"], good["CONT"]) and np.array_equal(res["TERM"], good["TERM"])


def test_batch_independence():
    """any subset of the scanpaths, in another order, scores bit-identically: the sums of a step do not depend on the rest of the call"""
    c = case((30, 40), 4)
    full = call(c)
    S = len(c["paths"])
    for keep in (list(range(0, S, 2))[::-1], [5], list(np.random.default_rng(3).permutation(S))):
        part = call(c, keep)
        for m in list(R.METRICS) + ["n", "dropped"]:
            assert np.array_equal(part[m], full[m][keep], equal_nan=True), (m, keep[:4])
    for m in R.METRICS:                                                          # each output alone, and in another order
        assert np.array_equal(call(c, metrics=(m,))[m], full[m], equal_nan=True), m
    rev = call(c, metrics=R.METRICS[::-1])
    assert list(rev)[:6] == list(R.METRICS[::-1]) and all(np.array_equal(rev[m], full[m], equal_nan=True) for m in R.METRICS)


def test_more_than_64_scanpaths_on_one_row():
    c = dict(case((5, 13), 4))
    g = np.random.default_rng(9)
    h, w = c["frame"]
    c["paths"] = [np.stack([g.uniform(0, w, 1), g.uniform(0, h, 1), g.uniform(0.1, 0.5, 1)], 1) for _ in range(70)]
    c["rows"] = [1] * 66 + [0, 3, 3, 0]
    c["brows"] = g.integers(0, 2, 70)
    ref = R.scanpath_likelihood(c["probs"], c["paths"], c["rows"], c["frame"], c["shape"], c["u"], c["baseline"], c["brows"], c["mu"],
                                c["s2"], c["min_length"])
    got = call(c)
    exact(got, ref, "70 scanpaths")
    close(got, ref, "70 scanpaths", ("LL", "IG", "NSS", "DLL", "STOP"))


def test_one_upload_one_launch_one_copy_back(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    L = hip.lib()
    calls = {"launch": 0, "upload": 0, "host": 0}
    launch, upload, host = L.sp_scan_likelihood, _batch.upload, _batch.Out.host

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(L, "sp_scan_likelihood", counted("launch", launch))
    monkeypatch.setattr(_batch, "upload", counted("upload", upload))
    monkeypatch.setattr(_batch.Out, "host", counted("host", host))
    for shape, T in (((3, 5), 1), ((30, 40), 16)):
        call(case(shape, T))
    assert calls == {"launch": 2, "upload": 2, "host": 2}                         # one each per call, whatever R, S, T and the metrics
    c = case((3, 5), 4)                                                           # a host baseline travels with the one upload
    a = M().scanpath_likelihood(torch.from_numpy(c["probs"]).to(dev()), c["paths"], c["rows"], c["frame"], uniform_mix=0.0,
                                metrics=("IG",), map_shape=c["shape"], baseline=c["baseline"], baseline_rows=c["brows"])
    assert calls == {"launch": 3, "upload": 3, "host": 3} and np.array_equal(a["IG"], call(c)["IG"], equal_nan=True)


# ---- the keyed evaluation, its table and the loop ---------------------------------------------------------------------------------------------
_FV = {"names": ("start_x", "start_y", "duration"), "formats": ("f8", "f8", "f8")}
SHAPE, FRAME, T_EV = (3, 5), (24.0, 40.0), 4


def _batch_case(two_heads):
    """4 samples: keys q1, q2, q1, q3; every subject of q2 has an empty scanpath; fixation vectors in the reference's structured form"""
    g = np.random.default_rng(77 + two_heads)
    A = 1 + SHAPE[0] * SHAPE[1]
    N = 4
    predict = {}
    for head in (("good_", "poor_") if two_heads else ("",)):
        predict[head + "all_actions_prob"] = torch.from_numpy(np.stack([softmax(g, 2.0, T_EV, A) for _ in range(N)]))
        predict[head + "log_normal_mu"] = torch.from_numpy(g.normal(-1.2, 0.4, (N, T_EV)).astype(np.float32))
        predict[head + "log_normal_sigma2"] = torch.from_numpy(g.uniform(0.1, 1.0, (N, T_EV)).astype(np.float32))
    predict["good_all_actions_prob" if two_heads else "all_actions_prob"][3, 1, 1:] = 1.0 / 16       # a constant map: no NSS there

    def fv(n, outside=False):
        a = np.zeros(n, dtype=_FV)
        a["start_x"], a["start_y"], a["duration"] = g.uniform(0, FRAME[1], n), g.uniform(0, FRAME[0], n), g.uniform(0.1, 0.6, n)
        if outside:
            a["start_x"][0] = FRAME[1] + 1.0
        return a

    fix_vectors = [[fv(3), fv(5, outside=True), fv(1)], [fv(0), fv(0)], [fv(4), fv(2)], [fv(6), fv(2, outside=True), fv(0)]]
    performances = [[True, False, True], [False, True], [False, False], [True, True, False]]
    keys = ["q1", "q2", "q1", "q3"]
    baseline = g.uniform(0.1, 1.0, (2, A - 1))
    return predict, fix_vectors, performances, keys, baseline, [0, 1, 1, 0]


def _plain(fv):
    return np.stack([fv["start_x"], fv["start_y"], fv["duration"]], 1)


def _expected(predict, fix_vectors, performances, keys, baseline, image_keys, samples, u, min_length):
    """(means, per_key) of the samples from the restatement's per-fixation values, by plain loops"""
    N = len(keys)
    heads = ("good_", "poor_") if performances is not None else ("",)
    cat = lambda name: np.concatenate([predict[h + name].numpy() for h in heads], 0)
    paths, rows, brows, key = [], [], [], []
    for i in samples:
        for k, f in enumerate(fix_vectors[i]):
            paths.append(_plain(f))
            rows.append(i if performances is None or performances[i][k] else N + i)
            brows.append(image_keys[i])
            key.append(keys[i])
    ref = R.scanpath_likelihood(cat("all_actions_prob"), paths, rows, FRAME, SHAPE, u, baseline, brows, cat("log_normal_mu"),
                                cat("log_normal_sigma2"), min_length)
    order = list(dict.fromkeys(keys[i] for i in samples))
    means, per_key = {"dropped": int(ref["dropped"].sum())}, {"keys": order}
    for m in R.METRICS:
        vals = {q: [] for q in order}
        nan = 0
        for s in range(len(paths)):
            for v in ([ref[m][s]] if m == "STOP" else ref[m][s, :ref["n"][s]]):
                if np.isnan(v):
                    nan += 1
                else:
                    vals[key[s]].append(v)
        every = [v for q in order for v in vals[q]]
        per_key[m] = np.array([np.sum(vals[q]) / len(vals[q]) if vals[q] else np.nan for q in order])
        means.update({m: np.sum(every) / len(every) if every else np.nan, m + "_count": len(every), m + "_nan": nan,
                      m + "_nan_keys": int(np.isnan(per_key[m]).sum())})
    return means, per_key


def _on_device(predict):
    return {k: v.to(dev()) for k, v in predict.items()}


def _same_tables(got, want, what):
    (means, per_key), (wmeans, wper_key) = got, want
    assert per_key["keys"] == wper_key["keys"], what
    for m in R.METRICS:
        close(per_key, wper_key, what + " per key", (m,))
        close({m: np.array(means[m])}, {m: np.array(wmeans[m])}, what + " pooled", (m,))
        for k in ("_count", "_nan", "_nan_keys"):
            assert means[m + k] == wmeans[m + k], (what, m + k, means[m + k], wmeans[m + k])
    assert means["dropped"] == wmeans["dropped"], what


@pytest.mark.parametrize("two_heads", [True, False], ids=["air_two_heads", "single_head"])
def test_likelihood_evaluation_table_and_loop(two_heads, monkeypatch):
    from scanpaths_amd import hip, inference
    from scanpaths_amd.utils import evaluation as E
    predict, fix_vectors, performances, keys, baseline, image_keys = _batch_case(two_heads)
    perf = performances if two_heads else None
    u, min_length = 0.02, 0                                                       # (an empty scanpath scores -inf under a min_length)
    kw = dict(uniform_mix=u, metrics=R.METRICS, min_length=min_length, frame_size=FRAME, map_shape=SHAPE)
    base = torch.from_numpy(baseline).to(dev())
    got = E.likelihood_evaluation(_on_device(predict), fix_vectors, keys, perf, image_keys, base, **kw)
    want = _expected(predict, fix_vectors, perf, keys, baseline, image_keys, range(4), u, min_length)
    _same_tables(got, want, f"two_heads={two_heads}")
    means, per_key = got
    assert per_key["keys"] == ["q1", "q2", "q3"] and means["dropped"] == 2 and per_key["dropped"].tolist() == [1, 0, 1]
    q2 = 1                                                                        # every subject's scanpath is empty: NaN, and counted
    assert all(np.isnan(per_key[m][q2]) for m in R.METRICS[:5]) and means["LL_nan_keys"] == 1 and np.isfinite(per_key["STOP"][q2])
    assert means["LL_nan"] == means["AUC_nan"] == 2 and means["DLL_nan"] == 0 and means["STOP_nan"] == 0
    assert means["NSS_nan"] == 4 and means["LL_count"] == 18 and means["DLL_count"] == 20 and means["STOP_count"] == 10   # 2 on the constant map
    # the table: two half-batches merge to the whole batch
    halves = []
    for samples in ((0, 1), (2, 3)):
        sl = {k: v[list(samples)].to(dev()) for k, v in predict.items()}
        halves.append(E.likelihood_evaluation(sl, [fix_vectors[i] for i in samples], [keys[i] for i in samples],
                                              None if perf is None else [perf[i] for i in samples], [image_keys[i] for i in samples],
                                              base, **kw)[0])
    table = E.LikelihoodTable()
    for part in halves:
        table.add(part)
    merged = table.result()
    for m in R.METRICS:
        close({m: np.array(merged[m])}, {m: np.array(means[m])}, "merged halves", (m,))
        assert merged[m + "_count"] == means[m + "_count"] and merged[m + "_nan"] == means[m + "_nan"], m
    assert merged["dropped"] == means["dropped"]

    # the loop: a stub model that returns fixed tensors, a two-batch loader; no sampling entry point is called
    class Stub:
        calls = 0

        def eval(self):
            return self

        def __call__(self, images, attention_maps):
            assert images.is_cuda and attention_maps.is_cuda
            lo = 2 * Stub.calls
            Stub.calls += 1
            return {k: v[lo:lo + 2].to(dev()) for k, v in predict.items()}

    def no_sampling(*a):
        raise AssertionError("the likelihood loop does not sample")

    L = hip.lib()
    for name in ("sp_sample_actions", "sp_generate_scanpath", "sp_beam_search"):
        monkeypatch.setattr(L, name, no_sampling)
    launches = []
    launch = L.sp_scan_likelihood
    monkeypatch.setattr(L, "sp_scan_likelihood", lambda *a: launches.append(1) or launch(*a))
    loader = [{"images": torch.zeros(2, 3, 8, 8), "attention_maps": torch.zeros(2, 1, 8, 8), "fix_vectors": fix_vectors[lo:lo + 2],
               "performances": performances[lo:lo + 2], "question_ids": keys[lo:lo + 2], "baseline_rows": image_keys[lo:lo + 2],
               "img_names": ["a", "b"]} for lo in (0, 2)]
    loop_means, per_batch = inference.run_likelihood_loop(Stub(), loader, uniform_mix=u, metrics=R.METRICS, min_length=min_length,
                                                          baseline=base, frame_size=FRAME, map_shape=SHAPE)
    assert Stub.calls == 2 and len(launches) == 2 and len(per_batch) == 2 and per_batch[0]["keys"] == ["q1", "q2"]
    assert set(loop_means) == set(merged)
    for k, v in merged.items():
        assert np.array_equal(loop_means[k], v, equal_nan=True), (k, loop_means[k], v)


def test_cell_baselines_and_zero_gain_against_the_own_baseline():
    g = np.random.default_rng(5)
    Hm, Wm = 5, 13
    h, w = 60.0, 130.0
    G = 4
    image = g.integers(0, G, 30)
    paths = [np.stack([g.uniform(-5, w + 5, n), g.uniform(-5, h + 5, n)], 1) for n in g.integers(0, 90, 30)]      # some outside; any length
    base = M().cell_baselines(paths, image, (h, w), (Hm, Wm))
    assert base.is_cuda and base.dtype == torch.float64 and tuple(base.shape) == (G, Hm * Wm)
    want = np.zeros((G, Hm * Wm))
    for sp, im in zip(paths, image):
        for x, y in sp:
            c = R.cell_of(x, y, (h, w), (Hm, Wm))
            if c is not None:
                want[[q for q in range(G) if q != im], c] += 1.0
    assert np.array_equal(base.cpu().numpy(), want)
    # a model whose map IS its baseline row (unnormalised counts, exact in float32) gains exactly 0 bits, at any mix
    T = 3
    probs = torch.cat([torch.full((G, 1), 0.25, dtype=torch.float64, device=base.device), base], 1).to(torch.float32)
    probs = probs[:, None, :].repeat(1, T, 1)
    short = [sp[:T + 1] for sp in paths]
    for u in (0.0, 0.01):
        res = M().scanpath_likelihood(probs, short, image, (h, w), uniform_mix=u, metrics=("IG", "LL"), map_shape=(Hm, Wm),
                                      baseline=base, baseline_rows=image)
        scored = ~np.isnan(res["LL"])
        assert scored.sum() > 40 and (res["IG"][scored & np.isfinite(res["LL"])] == 0.0).all()
        assert np.isnan(res["IG"][scored & np.isinf(res["LL"])]).all()             # -inf - -inf: a cell nobody else looked at, at u = 0
