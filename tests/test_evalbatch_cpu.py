"""CPU-only checks of the one packer of the evaluation scorers (scanpaths_amd/utils/evaltools/_batch.py): pack,
check_pairs, the layout of upload and Out on torch's CPU device, and the refusals of sed_stde_pairs / tde_pairs, which come before a
device or the library is touched.  No device, no library."""
import numpy as np
import pytest
import torch

from scanpaths_amd.utils.evaltools import _batch as B

CPU = torch.device("cpu")


def _walk(n, ncol=2, seed=0):
    return np.random.default_rng(seed + n).uniform(0, 100, (n, ncol))


def _check(b, ncol, counts):
    assert b.ncol == ncol and b.rows.shape == (sum(counts), ncol) and b.rows.dtype == np.float64 and b.rows.flags["C_CONTIGUOUS"]
    assert b.counts.dtype == np.int32 and b.counts.tolist() == list(counts)
    assert b.starts.dtype == np.int64 and b.starts.tolist() == [sum(counts[:k]) for k in range(len(counts))]


def test_pack_shapes_with_empty_scanpaths_anywhere():
    _check(B.pack([], min_cols=2), 2, [])
    _check(B.pack([], min_cols=3), 3, [])
    _check(B.pack([[], np.zeros((0, 5)), np.zeros(0)], min_cols=2), 2, [0, 0, 0])        # an empty scanpath has no width
    a, c = _walk(3, 3), _walk(5, 3)
    for paths, counts in (([[], a, c], [0, 3, 5]), ([a, np.zeros((0, 2)), c], [3, 0, 5]), ([a, c, []], [3, 5, 0])):
        b = B.pack(paths, min_cols=2)
        _check(b, 3, counts)
        assert np.array_equal(b.rows, np.concatenate([a, c], 0))
    b = B.pack([a[::2], np.asfortranarray(c)], min_cols=2)                                  # strided inputs come out contiguous
    _check(b, 3, [2, 5])
    assert np.array_equal(b.rows, np.concatenate([a[::2], c], 0))
    assert B.starts(np.array([2, 0, 3], dtype=np.int32)).tolist() == [0, 2, 2]


def test_pack_refusals():
    with pytest.raises(ValueError, match="scanpaths need the same number .>= 2. of columns"):
        B.pack([_walk(3, 2), _walk(3, 3)], min_cols=2)
    with pytest.raises(ValueError, match="groups need the same number .>= 3. of columns"):
        B.pack([_walk(3, 2)], min_cols=3, what="group")
    with pytest.raises(ValueError, match="columns"):
        B.pack([[1.0, 2.0, 3.0]], min_cols=2)                                               # a flat list is one column
    _check(B.pack([_walk(B.MAX_FIXATIONS)], min_cols=2), 2, [64])
    with pytest.raises(ValueError, match="scanpath of 65 fixations exceeds the kernel limit 64"):
        B.pack([_walk(3), _walk(B.MAX_FIXATIONS + 1)], min_cols=2)
    _check(B.pack([_walk(7)], min_cols=2, limit=7), 2, [7])
    with pytest.raises(ValueError, match="group of 8 fixations exceeds the kernel limit 7"):
        B.pack([_walk(8)], min_cols=2, limit=7, what="group")
    _check(B.pack([_walk(500)], min_cols=2, limit=None), 2, [500])
    with pytest.raises(ValueError, match="scanpath 1 is empty"):
        B.pack([_walk(3), [], _walk(2)], min_cols=2, allow_empty=False)
    _check(B.pack([_walk(3)], min_cols=2, allow_empty=False), 2, [3])


def test_check_pairs():
    for bad in ([(0, -1)], [(0, 3)], [(0, 1), (3, 0)], [(-1, 0)]):
        with pytest.raises(ValueError, match="pair index out of range"):
            B.check_pairs(bad, 3)
    with pytest.raises(ValueError, match="out of range"):
        B.check_pairs([(0, 0)], 0)
    for empty in ([], np.zeros((0, 2), dtype=np.int64)):
        pr = B.check_pairs(empty, 0)
        assert pr.shape == (0, 2) and pr.dtype == np.int32
    pr = B.check_pairs(np.array([[0, 1, 2], [2, 2, 0]]).T, 3)                               # a transposed view
    assert pr.dtype == np.int32 and pr.flags["C_CONTIGUOUS"] and pr.tolist() == [[0, 2], [1, 2], [2, 0]]
    with pytest.raises(ValueError, match="group index out of range"):
        B.check_index([0, 2], 2, "group")
    assert B.check_index([1, 0], 2, "group").dtype == np.int64


def _spans(buf, at, nbytes):
    """{name: (offset, bytes)} of addresses inside buf; every offset a multiple of 8, no two sections overlapping"""
    off = {k: a - buf.data_ptr() for k, a in at.items()}
    assert all(o % 8 == 0 and 0 <= o and o + max(nbytes[k], 1) <= buf.numel() for k, o in off.items()), off
    spans = sorted((off[k], off[k] + max(nbytes[k], 1)) for k in off)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    return off


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("P", [1, 3])
def test_upload_layout_is_aligned_whatever_the_lengths_and_the_order(K, P):
    b = B.pack([_walk(n + 1, 3) for n in range(K)], min_cols=2)
    pairs = B.check_pairs([(k % K, (k + 1) % K) for k in range(P)], K)
    group = np.arange(K, dtype=np.int32)
    for sections in (b.sections(pairs=pairs, group=group),
                     dict(counts=b.counts, pairs=pairs, group=group, starts=b.starts, rows=b.rows)):      # int32 sections first
        buf, at = B.upload(sections, CPU)
        assert buf.dtype == torch.uint8 and list(at) == list(sections)
        off = _spans(buf, at, {k: v.nbytes for k, v in sections.items()})
        raw = buf.numpy()
        for k, v in sections.items():
            assert np.array_equal(raw[off[k]:off[k] + v.nbytes].view(v.dtype).reshape(v.shape), v), k


def test_upload_gives_an_empty_section_an_address_of_its_own():
    b = B.pack([[], []], min_cols=3)
    sections = b.sections(pairs=B.check_pairs([], 2), tail=np.zeros(0))
    buf, at = B.upload(sections, CPU)
    _spans(buf, at, {k: v.nbytes for k, v in sections.items()})
    assert len(set(at.values())) == len(at)


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("P", [1, 3])
def test_out_layout_and_copy_back(K, P):
    sections = {"kept": (np.int32, K), "rows": (np.float64, 3 * K), "flags": (np.int32, P), "scores": (np.float64, 5 * P),
                "none": (np.float64, 0)}
    out = B.Out(sections, CPU)
    at = {k: out.ptr(k) for k in sections}
    nbytes = {k: np.dtype(dt).itemsize * n for k, (dt, n) in sections.items()}
    off = _spans(out.buf, at, nbytes)
    assert out.ptr("absent") is None
    out.buf.zero_()
    want = {}
    for j, (k, (dt, n)) in enumerate(sections.items()):                                     # write through the addresses, as a kernel does
        want[k] = (np.arange(n) + 10 * j).astype(dt)
        out.buf.numpy()[off[k]:off[k] + nbytes[k]] = want[k].view(np.uint8)
    host = out.host()
    assert list(host) == list(sections)
    for k, (dt, n) in sections.items():
        assert host[k].dtype == np.dtype(dt) and host[k].shape == (n,) and np.array_equal(host[k], want[k]), k
    part = out.host("scores", "flags")
    assert list(part) == ["scores", "flags"] and all(np.array_equal(part[k], want[k]) for k in part)


def test_old_scorers_refuse_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M

    def no_device():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(M, "_device", no_device)
    monkeypatch.setattr(hip, "lib", no_device)
    a, b = _walk(4), _walk(6)
    calls = (lambda paths, pairs: M.sed_stde_pairs(paths, pairs, (240, 320, 3)), lambda paths, pairs: M.tde_pairs(paths, pairs, k=2))
    for call in calls:
        for bad in ([(0, 2)], [(-1, 0)], [(0, 1), (5, 0)]):
            with pytest.raises(ValueError, match="out of range"):
                call([a, b], bad)
        with pytest.raises(ValueError, match="kernel limit"):
            call([a, _walk(M.MAX_FIXATIONS + 1)], [(0, 1)])
        with pytest.raises(ValueError, match="columns"):
            call([a, _walk(4, 3)], [(0, 1)])
        with pytest.raises(ValueError, match="columns"):
            call([a[:, :1], b[:, :1]], [(0, 1)])
    with pytest.raises(ValueError, match="distance_mode"):
        M.tde_pairs([a, b], [(0, 1)], k=2, distance_mode="Median")
    assert M.MAX_FIXATIONS is B.MAX_FIXATIONS
