"""Host reference of csrc/sampling.hip ``sample_rows_kernel`` -- TEST INFRASTRUCTURE ONLY, plain numpy, no kernel of the package.

The generator is a public contract (include/scanpaths_amd.h: Philox4x32-10(seed; row)), so every draw of the kernel is a deterministic
function of its inputs and can be checked one by one:

  * ``philox4x32_10`` / ``u01`` / ``row_uniforms``  -- the random words and the three uniforms of a row, bit for bit;
  * ``acceptable_mask`` / ``acceptable_actions``     -- the set of actions a correct inverse-CDF sampler may return for a uniform,
                                                       from an fp64 CDF and an a-priori float32 rounding budget (DELTA_ADDS);
  * ``durations``                                    -- exp(eps * sigma2 + mu) in fp64 (sigma2 as the scale: the reference's quirk);
  * ``emulate_kernel_total`` / ``emulate_kernel_search`` / ``find_segment_end_traps``
                                                     -- a float32, add-for-add emulation of the search AS OF THE COMMIT BEFORE THE
                                                       SEGMENT-END FIX (fallback = the row's last positive entry).  It exists only
                                                       to FIND inputs that land on a segment's end; no GPU assertion depends on
                                                       its prediction being right.
  * ``make_case`` / ``trap_row``                     -- the inputs the CPU and the GPU tests share.
"""
from __future__ import annotations

import math

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_F32 = np.float32
NTHREADS = 256                       # block size of sample_rows_kernel: the row is cut into 256 segments of ``per`` entries


# ---------------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
# ---------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two; broadcast against each other.  Returns four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in counter]
    k0, k1 = (np.asarray(x, dtype=np.uint64) & _M32 for x in key)
    c = list(np.broadcast_arrays(*c, k0, k1)[:4])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return [x.astype(np.uint32) for x in c]


def u01(x):
    """uint32 -> float32 in (0, 1): ((x >> 8) + 0.5) * 2^-24 in float32 arithmetic, as the kernel evaluates it.  For
    x >> 8 >= 2^23 the sum is a tie of float32 and rounds to even -- numpy's float32 addition does the same.  For the one value
    x >> 8 = 2^24 - 1 "even" is 2^24, i.e. u = 1: like the kernel, keep it at the largest float32 below 1."""
    hi = (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(_F32)          # < 2^24: exact
    return np.minimum((hi + _F32(0.5)) * _F32(1.0 / 16777216.0), _F32(1.0 - 2.0 ** -24))


def row_words(rows, seed):
    """the Philox block of each row: counter (row & 0xffffffff, row >> 32, 0, 0), key (seed & 0xffffffff, seed >> 32)"""
    rows = np.asarray(rows, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    zero = np.zeros_like(rows)
    return philox4x32_10((rows & _M32, rows >> np.uint64(32), zero, zero), (seed & 0xFFFFFFFF, seed >> 32))


def row_uniforms(nrows, seed):
    """(u_action, u_radius, u_angle): float32 [nrows] each -- words 0, 1, 2 of the row's block"""
    w = row_words(np.arange(nrows), seed)
    return u01(w[0]), u01(w[1]), u01(w[2])


# ---------------------------------------------------------------------------------------------------------------------------
# the set of acceptable actions
# ---------------------------------------------------------------------------------------------------------------------------
def per_of(A):
    return (A + NTHREADS - 1) // NTHREADS


def delta_adds(A):
    """The rounding budget of the comparison ``running sum >= u * total``, in units of 2^-24 * total.

    Every float32 addition of non-negative terms is off by at most half an ulp of its result, i.e. by at most 2^-24 times a partial
    sum, and every partial sum is at most ``total`` (to first order).  The kernel's running sum at an entry went through
        per   additions  for a segment's own sum (the last coarse step adds a sum that was built from zero),
        256   additions  at most in the coarse scan over the segment sums,
        per   additions  at most in the fine scan inside (or, after the segment-end fix, past) the segment,
    and the other side of the comparison, target = u * total, through
        per   additions  ... already counted above: total is built from the same per-thread segment sums,
        6     butterfly levels inside a wave and 3 additions across the four waves (each scaled by u < 1),
        1     rounding of the product.
    That is 2 * per + 256 + 10; the constant is rounded up to 16 for the second-order terms (partial sums that exceed ``total`` by
    their own rounding).  Nothing here is fitted to what the kernel returns."""
    return 2 * per_of(A) + 256 + 16


def acceptable_mask(p, lo, u):
    """p [R, A] float32 rows, lo [R] (1 where the terminate action is masked), u [R] float32 uniforms -> bool [R, A].

    c = fp64 cumulative sum of the float32 row over a >= lo, total = c[-1], target = u * total (fp64).  Action a is acceptable iff
    p[a] > 0, a >= lo and its CDF interval [c[a-1], c[a]] meets [target - delta, target + delta], delta = delta_adds(A) * 2^-24 *
    total.  A row without allowed mass (total == 0) has the single answer ``lo``."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 2
    R, A = p.shape
    lo = np.broadcast_to(np.asarray(lo, dtype=np.int64), (R,))
    pm = p.astype(np.float64)
    pm[lo == 1, 0] = 0.0
    c = np.cumsum(pm, axis=1)
    total = c[:, -1:]
    target = np.asarray(u, dtype=np.float64).reshape(R, 1) * total
    delta = delta_adds(A) * 2.0 ** -24 * total
    c_prev = np.concatenate([np.zeros((R, 1)), c[:, :-1]], axis=1)
    ok = (pm > 0) & (c_prev <= target + delta) & (c >= target - delta)
    dead = total[:, 0] == 0
    ok[dead] = False
    ok[dead, lo[dead]] = True
    return ok


def acceptable_actions(p_row, t, min_length, u):
    """one row: the sorted array of actions a correct sampler may return at step t for the uniform u"""
    lo = 1 if t < min_length else 0
    return np.flatnonzero(acceptable_mask(np.asarray(p_row, dtype=np.float32)[None], [lo], [u])[0])


def lo_of_rows(nrows, T, min_length):
    """row = b * T + t: terminate masked for t < min_length"""
    return ((np.arange(nrows) % T) < min_length).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# durations
# ---------------------------------------------------------------------------------------------------------------------------
def durations(mu, sigma2, seed):
    """mu, sigma2: float32 arrays of B*T elements in row order.  Returns (duration, eps) in fp64:
    eps = sqrt(-2 ln u01(c[1])) * cos(2 pi u01(c[2])), duration = exp(eps * sigma2 + mu)."""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    s2 = np.asarray(sigma2, dtype=np.float64).reshape(-1)
    _, u1, u2 = row_uniforms(mu.size, seed)
    eps = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * math.pi * u2.astype(np.float64))
    return np.exp(eps * s2 + mu), eps


def scanpath_length(actions, T):
    """the literal loop of the reference's models/sampling.py:29-33 on [B, T] actions"""
    actions = np.asarray(actions)
    length = np.zeros(actions.shape[0])
    for index in range(T):
        length[np.logical_and(length == 0, actions[:, index] == 0)] = index
    length[length == 0] = T
    return length


# ---------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernel's search as of the commit before the segment-end fix (input finder only)
# ---------------------------------------------------------------------------------------------------------------------------
def _tables(p_row, lo):
    """per-row tables of the kernel's float32 arithmetic: segment sums built from zero, their serial running sum (the coarse scan),
    and for every segment the fine scan's running sums (started from the coarse sum before the segment)"""
    p = np.asarray(p_row, dtype=np.float32)
    A = p.size
    per = per_of(A)
    pm = np.zeros(NTHREADS * per, dtype=np.float32)             # padding and the masked terminate add 0.f: exact, like skipping them
    pm[:A] = p
    if lo:
        pm[0] = 0
    seg = pm.reshape(NTHREADS, per)
    part = np.zeros(NTHREADS, dtype=np.float32)
    for j in range(per):
        part = part + seg[:, j]
    coarse = np.cumsum(part, dtype=np.float32)                  # numpy accumulates serially: run_i = fl(run_{i-1} + part[i])
    run = np.concatenate([np.zeros(1, np.float32), coarse[:-1]])
    fine = np.empty((NTHREADS, per), dtype=np.float32)
    for j in range(per):
        run = run + seg[:, j]
        fine[:, j] = run
    return {"A": A, "per": per, "pm": pm, "seg": seg, "part": part, "coarse": coarse, "fine": fine}


def emulate_kernel_total(p_row, lo, tables=None):
    """``total`` in the kernel's order: per-thread segment sums, xor butterfly 32, 16, ..., 1 inside each 64-lane wave, then
    sh[0] + sh[1] + sh[2] + sh[3]"""
    tb = tables or _tables(p_row, lo)
    v = tb["part"].reshape(4, 64).copy()
    lane = np.arange(64)
    o = 32
    while o:
        v = v + v[:, lane ^ o]
        o >>= 1
    sh = v[:, 0]
    return ((sh[0] + sh[1]) + sh[2]) + sh[3]


def emulate_kernel_search(p_row, lo, target_f32, tables=None):
    """-> (chosen, fell_off_segment_end): the coarse scan over 256 segment sums, the fine scan inside the chosen segment, and --
    as of the commit before the fix -- the jump to the row's last positive entry when the fine scan ends short of the target"""
    tb = tables or _tables(p_row, lo)
    target = np.float32(target_f32)
    per, pm = tb["per"], tb["pm"]
    hit = np.flatnonzero(tb["coarse"] >= target)
    seg = int(hit[0]) if hit.size else NTHREADS - 1
    ok = np.flatnonzero((tb["fine"][seg] >= target) & (tb["seg"][seg] > 0))
    if ok.size:
        return seg * per + int(ok[0]), False
    pos = np.flatnonzero(pm > 0)
    return (int(pos[-1]) if pos.size else int(lo)), True


def segment_end_hazards(p_row, lo, tables=None):
    """The float32 targets at which the search falls off a segment's end although positive entries follow it, as closed intervals
    [(lo_bits, hi_bits, segment)] of float32 bit patterns.  Segment i is chosen for coarse[i-1] < target <= coarse[i]; its fine scan
    ends at fine_end = fine[i][last positive entry]; the draw falls off iff fine_end < target, i.e. fine_end < fl(run + part)."""
    tb = tables or _tables(p_row, lo)
    pm, per = tb["pm"], tb["per"]
    pos = np.flatnonzero(pm > 0)
    out = []
    if not pos.size:
        return out
    last_pos = int(pos[-1])
    prev = np.float32(0)
    for i in range(NTHREADS):
        top = tb["coarse"][i]
        posi = np.flatnonzero(tb["seg"][i] > 0)
        if posi.size and last_pos >= (i + 1) * per:
            fine_end = tb["fine"][i][posi[-1]]
            below = max(prev, fine_end)
            if below < top:                                       # positive float32: the bit patterns are ordered like the values
                out.append((int(np.float32(below).view(np.uint32)) + 1, int(np.float32(top).view(np.uint32)), i))
        prev = top
    return out


def find_segment_end_traps(p_row, rows, seeds, lo):
    """One p_row replicated over ``rows`` rows: the (seed, row) pairs whose action uniform lands on a segment-end hazard.  The
    hazardous targets depend on p_row alone and are computed once; every seed's u stream is then matched against them."""
    tb = _tables(p_row, lo)
    haz = segment_end_hazards(p_row, lo, tb)
    if not haz:
        return []
    starts = np.array([h[0] for h in haz], dtype=np.int64)
    ends = np.array([h[1] for h in haz], dtype=np.int64)
    total = emulate_kernel_total(p_row, lo, tb)
    seeds = np.asarray(list(seeds), dtype=np.uint64)
    r = np.arange(rows, dtype=np.uint64)[None, :]
    zero = np.zeros_like(r)
    w0 = philox4x32_10((r & _M32, r >> np.uint64(32), zero, zero), ((seeds & _M32)[:, None], (seeds >> np.uint64(32))[:, None]))[0]
    target = u01(w0) * total                                     # float32 product, rounded once like the kernel's
    bits = target.view(np.uint32).astype(np.int64)
    k = np.searchsorted(starts, bits, side="right") - 1
    hit = (k >= 0) & (bits <= ends[np.maximum(k, 0)])
    si, ri = np.nonzero(hit)
    return [(int(seeds[s]), int(rw)) for s, rw in zip(si, ri)]


# ---------------------------------------------------------------------------------------------------------------------------
# shared test inputs
# ---------------------------------------------------------------------------------------------------------------------------
def softmax_rows(rng, n, A, scale=2.0):
    z = scale * rng.standard_normal((n, A))
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


TRAP_A, TRAP_ROWS, TRAP_T, TRAP_SEEDS = 1201, 4096, 4, 1024


def trap_row():
    """the committed trap input: one PCG64-seeded row softmax(2 * randn) at A = 1201"""
    return softmax_rows(np.random.Generator(np.random.PCG64(25)), 1, TRAP_A)[0]


_trap_cache = []


def committed_traps():
    """the (seed, row) pairs of the trap input: seeds 0 .. TRAP_SEEDS-1 over B * T = 4096 replicas of trap_row(), terminate allowed
    everywhere (min_length 0).  About a second of numpy; computed once per process."""
    if not _trap_cache:
        row, found = trap_row(), []
        for s0 in range(0, TRAP_SEEDS, 256):                      # chunks keep the [seeds, rows] word arrays small
            found += find_segment_end_traps(row, TRAP_ROWS, range(s0, s0 + 256), 0)
        _trap_cache.append(found)
    return _trap_cache[0]


CASE_T, CASE_ROWS = 4, 2048
CASE_SIZES = (2, 7, 255, 256, 257, 513, 1201, 2561)
CASE_SEEDS = (3, 2 ** 32 + 5, 2 ** 64 - 1)
PLANTED = ("scattered_zeros", "segment0_zeros", "last_entry", "entry_1", "terminate_0.99", "no_allowed_mass", "sum_37.5", "tiny_beside_1")


def parity_cases():
    """(A, min_length, seed): every A at min_length 2 with the three seeds in turn, every min_length of {0, 1, 2, T, T + 3} on
    A in {7, 257, 1201}"""
    out = [(A, 2, CASE_SEEDS[i % 3]) for i, A in enumerate(CASE_SIZES)]
    for i, A in enumerate((7, 257, 1201)):
        for j, ml in enumerate((0, 1, CASE_T, CASE_T + 3)):
            out.append((A, ml, CASE_SEEDS[(i + j + 1) % 3]))
    return out


def make_case(A):
    """probs [B, T, A] float32 with B * T = 2048: softmax(2 * randn) rows; samples 0..7 (all T steps each, so that every planted
    row meets both the masked and the unmasked terminate) carry the rows of PLANTED, in that order"""
    T, B = CASE_T, CASE_ROWS // CASE_T
    rng = np.random.Generator(np.random.PCG64(1000 + A))
    p = softmax_rows(rng, B * T, A).reshape(B, T, A)
    per = per_of(A)
    z = rng.random((T, A)) < 0.3                                 # exact zeros scattered through the row
    z[:, A - 1] = False
    p[0][z] = 0.0
    p[1, :, 1:per] = 0.0                                         # segment 0 = entries [0, per): all of it beyond the terminate
    p[2] = 0.0
    p[2, :, A - 1] = 1.0                                         # all mass on the last entry
    p[3] = 0.0
    p[3, :, 1] = 1.0                                             # all mass on entry 1
    p[4] *= np.float32(0.01) / p[4, :, 1:].sum(-1, keepdims=True, dtype=np.float32)
    p[4, :, 0] = 0.99                                            # 0.99 on terminate (masked for t < min_length)
    p[5] = 0.0
    p[5, :2, 0] = 0.7                                            # only terminate: no allowed mass while it is masked
    #                                                              (steps 2, 3 of this sample are zero throughout)
    p[6] *= np.float32(37.5)                                     # an unnormalised row
    p[7] = 1e-30
    p[7, :, A // 2] = 1.0                                        # entries of 1e-30 beside one of 1
    return np.ascontiguousarray(p)
