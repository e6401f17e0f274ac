"""What the fp64 parity modules share (tests/test_gemm_fp32_gpu.py, test_conv_f16x2_gpu.py, test_conv_bf16x3_gpu.py, test_head_direct_gpu.py,
test_rank1_grads_gpu.py, test_lstm_cell_gpu.py, test_decoder_ops_gpu.py, test_pool_sum_gpu.py, their *_ref.py restatements and tests/test_ops_gpu.py): the element-wise bar and its constants,
seeded data, guarded buffers on the host and on a device, the ctypes ABI, the max-norm metric, and the per-module record of PARITY figures.  A plain
module: pytest collects and registers nothing here, and no module keeps state in another.  tests/test_parity_harness_cpu.py holds the checks
below to their own failure cases on CPU buffers.  THE BAR (element-wise):  |got - ref| <= c 2^-24 S + 2^-149  with S the contraction over
absolute values and c the launch's longest chain of dependent fp32 roundings plus one (derived per kernel in the *_ref.py modules: chain_*)."""
import time
import zlib

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
SENTINEL = 0x7FC5A5A5          # int32 bit pattern of every output pad / gap / guard / workspace-tail word: a NaN, so a read of it shows too
GUARD = 64                     # words before and after every allocation (256 bytes: the 16-byte alignment of the live part is kept)
NAN = float("nan")


def cdiv(a, b):
    return -(-a // b)


def bar(S, c):
    return c * U * S + TINY


def worst(got, ref, S, c):
    """(max err / bar, flat index of it, err there, bar there); got must be finite"""
    g = got.double()
    assert torch.isfinite(g).all(), "a live output word is not finite"
    q = (g - ref).abs() / bar(S, c)
    i = int(q.argmax())
    return float(q.reshape(-1)[i]), i, float((g - ref).abs().reshape(-1)[i]), float(bar(S, c).reshape(-1)[i])


def randn(*shape, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal(shape).astype(np.float32))


def seed_of(name):
    return zlib.crc32(name.encode())


def rand(*shape, seed=0, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed + sum(shape)))
    return torch.from_numpy(g.standard_normal(shape).astype(np.float32) * scale)


# ---- guarded buffers: on the host ... --------------------------------------------------------------------------------------------------------------
class Guarded:
    """[nb] items of [rows][cols] with row stride ld and item stride `stride` inside one flat fp32 allocation: GUARD words, `offset` words, the
    items, GUARD words.  fill "nan": every word that is not data is NaN (operands); "sentinel": SENTINEL (outputs, workspaces).  data None
    leaves the live words at the fill (an output under beta = 0, a workspace)."""
    def __init__(self, nb, rows, cols, ld, stride=None, *, fill, data=None, offset=0):
        stride = rows * ld if stride is None else stride
        assert cols <= ld and (nb == 1 or stride >= (rows - 1) * ld + cols)
        self.nb, self.rows, self.cols, self.ld, self.stride, self.start = nb, rows, cols, ld, stride, GUARD + offset
        n = self.start + (nb - 1) * stride + rows * ld + GUARD
        if fill == "nan":
            self.flat = torch.full((n,), NAN, dtype=torch.float32)
        else:
            self.flat = torch.full((n,), SENTINEL, dtype=torch.int32).view(torch.float32)
        if data is not None:
            self.live(self.flat).copy_(data.reshape(nb, rows, cols))

    def live(self, flat):
        return flat.as_strided((self.nb, self.rows, self.cols), (self.stride, self.ld, 1), self.start)

    def pad_mask(self):
        m = torch.ones(self.flat.numel(), dtype=torch.bool)
        self.live(m).fill_(False)
        return m

    def pads_untouched(self, flat_after):
        """every word outside the live region still holds what it held"""
        m = self.pad_mask()
        return bool((flat_after.view(torch.int32)[m] == self.flat.view(torch.int32)[m]).all())

    def all_untouched(self, flat_after):
        return bool((flat_after.view(torch.int32) == self.flat.view(torch.int32)).all())


# ---- ... and on a device ---------------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda:0")


def abi():
    from scanpaths_amd import hip
    return hip, hip.lib()


def u16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev())


def f32(a):
    return torch.from_numpy(np.array(a, dtype=np.float32).reshape(-1)).to(dev())


def ints(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.int32).contiguous().to(dev())


def same_bits(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


class Buffer:
    """a fresh copy of a Guarded allocation on a device: what ONE launch reads or writes.  ptr is the address of the first live word."""
    def __init__(self, g, device=None):
        self.g = g
        self.dev = g.flat.to(dev() if device is None else device, copy=True)
        self.ptr = self.dev.data_ptr() + 4 * g.start

    def flat(self):
        """the whole allocation as it is now, on the host"""
        return self.dev.cpu()

    def pads_untouched(self):
        return self.g.pads_untouched(self.flat())

    def untouched(self):
        """no word changed at all: what a refused call must leave"""
        return self.g.all_untouched(self.flat())

    def live(self):
        """the live words [nb, rows, cols] after the launch; every other word must hold what it held"""
        flat = self.flat()
        assert self.g.pads_untouched(flat), "a word outside the live region (guard, pad or gap) changed"
        return self.g.live(flat)

    def read(self):
        """the live words of a flat buffer as raw int32 (numpy), guards checked"""
        return self.live().reshape(-1).view(torch.int32).numpy()


def up(g, device=None):
    """a host allocation with a layout of its own (strided rows, batch gaps, an offset) on the device; None stays None"""
    return None if g is None else Buffer(g, device)


def at(buf, extra_bytes=0):
    """the pointer a launch gets: NULL for an absent buffer"""
    return None if buf is None else buf.ptr + extra_bytes


def operand(t, device=None):
    """a float tensor, flat, between NaN guards; None (an absent optional operand) stays None"""
    return None if t is None else Buffer(Guarded(1, 1, t.numel(), t.numel(), fill="nan", data=t.float().reshape(-1)), device)


def output(n, data=None, device=None):
    """n words (an output, or a workspace of exactly the queried size) between sentinel guards; data: what they hold before the launch"""
    return Buffer(Guarded(1, 1, n, n, fill="sentinel", data=None if data is None else data.float().reshape(-1)), device)


def raw(nbytes, init=None, device=None):
    """nbytes of any type between sentinel guards: the output of a splitter, a scale vector, a scratch buffer; init: its bytes (numpy)"""
    assert nbytes % 4 == 0
    bits = None if init is None else torch.from_numpy(np.ascontiguousarray(init).view(np.int32).reshape(-1).copy()).view(torch.float32)
    return Buffer(Guarded(1, 1, nbytes // 4, nbytes // 4, fill="sentinel", data=bits), device)


# ---- the max-norm metric of tests/test_ops_gpu.py --------------------------------------------------------------------------------------------------
def close(a, b, tol, what=""):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3g}, tol {tol:g})"


def stress_bar(base, r32, r64):
    """max(existing bar, 10 max|ref32 - ref64|) in the metric of close (error over max(1, max|ref64|))"""
    r32, r64 = r32.detach().double(), r64.detach().double()
    return max(base, 10.0 * (r32 - r64).abs().max().item() / max(1.0, r64.abs().max().item()))


def decode_split(op, shape):
    """fp32 value of a 2xfp16 split operand [rows][K/16][2][16]"""
    n = 1
    for d in shape:
        n *= d
    planes = op.buf[:2 * n].view(-1, 2, 16).float()
    return ((planes[:, 0] + planes[:, 1]) / float(op.scale[0])).reshape(shape)


class Worst:
    """close with the figure kept: err / bar of every comparison of one test, the worst printed at its end (or at the failing one)"""
    def __init__(self, name):
        self.name, self.rows = name, []

    def close(self, got, ref, bar, what):
        a, b = got.detach().cpu().double(), ref.detach().cpu().double()
        assert a.shape == b.shape, (self.name, what, a.shape, b.shape)
        err = (a - b).abs().max().item() / max(1.0, b.abs().max().item()) if a.numel() else 0.0
        self.rows.append((err / bar, what, err, bar))
        if not err <= bar:
            self.report()
        close(got, ref, bar, f"{self.name} {what}")

    def report(self):
        r = max(self.rows, key=lambda t: (t[0] != t[0], t[0]))
        print(f"PARITY {self.name}: worst err/bar {r[0]:.3f} ({r[1]}: err {r[2]:.2e}, bar {r[3]:.1e}; {len(self.rows)} comparisons)")


# ---- the element-wise checks, with the figures of one module ---------------------------------------------------------------------------------------
class Summary:
    """One per test module: SUM = parity.Summary("f16x2"); _summary = SUM.fixture().  label: what the module's "total" line is called (none: plain
    "total"); groups: the order of the PARITY-SUMMARY lines (default: the order in which the groups were first judged)."""
    def __init__(self, label=None, groups=()):
        self.label, self.groups, self.rows = label, tuple(groups), {}          # rows: group -> [(err / bar, case, err, bar, chain)]

    def judge_values(self, group, name, got, ref, S, chain):
        """finiteness and the element-wise bar; the figure is kept and printed"""
        q, i, err, b = worst(got, ref, S, chain)
        self.rows.setdefault(group, []).append((q, name, err, b, chain))
        print(f"PARITY {group} {name}: err/bar {q:.3f} (err {err:.2e}, bar {b:.2e}, c {chain}, element {i})")
        assert q <= 1.0, f"{group} {name}: err {err:.3e} > bar {b:.3e} at element {i} (c = {chain})"

    def judge(self, group, name, out, flat_after, ref, S, chain, legacy=None):
        """out: the Guarded layout of the output, flat_after: its allocation after the launch (on the host).  Guards, finiteness, the element-wise
        bar, and -- legacy given -- the max-norm bar"""
        assert out.pads_untouched(flat_after), f"{group} {name}: a word outside the live output changed"
        got = out.live(flat_after)
        self.judge_values(group, name, got, ref, S, chain)
        if legacy is not None:
            close(got, ref, legacy, f"{group} {name}")

    def exact(self, group, name, got, ref):
        """lattice data: every summation order is exact, so got equals the fp64 result (up to the sign of a zero)"""
        got = got.double()
        ref = ref.reshape(got.shape)
        bad = (got != ref).nonzero()
        assert bad.numel() == 0, (f"{group} {name}: {bad.shape[0]} words differ from the exact result, first at {bad[0].tolist()}: "
                                  f"{got[tuple(bad[0])]} != {ref[tuple(bad[0])]}")

    def report(self, seconds):
        order = self.groups + tuple(g for g in self.rows if g not in self.groups)
        for group in order:
            rows = self.rows.get(group)
            if rows:
                q, name, err, b, chain = max(rows)
                print(f"\nPARITY-SUMMARY {group}: {len(rows)} comparisons, worst err/bar {q:.3f} at {name} (err {err:.2e}, bar {b:.2e}, c {chain})", end="")
        print(f"\nPARITY-SUMMARY {'total' if self.label is None else self.label + ' total'} {seconds:.1f} s")

    def fixture(self):
        """the module-scoped autouse fixture that prints this object's summary lines and the module's time at the module's end"""
        import pytest

        @pytest.fixture(scope="module", autouse=True)
        def at_module_end():
            t0 = time.time()
            yield
            self.report(time.time() - t0)
        return at_module_end
