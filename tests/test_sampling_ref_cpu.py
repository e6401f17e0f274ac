"""CPU: the host reference of the sampler (tests/sampling_ref.py) against published vectors and against itself, and the input
conditions of tests/test_sampling_gpu.py (those inputs must be sharp enough for an exact per-draw comparison to mean something)."""
import numpy as np
import pytest

import sampling_ref as R


def test_philox4x32_10_known_answer_vectors():
    """the three Philox4x32-10 vectors of the Random123 distribution's kat_vectors"""
    kat = (((0,) * 4, (0,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        assert tuple(int(x) for x in R.philox4x32_10(ctr, key)) == want
    # vectorised over rows, with the documented counter / key layout
    w = R.row_words(np.array([0, 0x85a308d3243f6a88], dtype=np.uint64), 0)
    assert int(w[0][0]) == 0x6627e8d5 and int(w[3][0]) == 0x9b00dbd8
    one = R.philox4x32_10((0x243f6a88, 0x85a308d3, 0, 0), (0, 0))
    assert [int(x[1]) for x in w] == [int(x) for x in one]
    w = R.row_words(np.array([5]), 0x299f31d0a4093822)
    assert [int(x[0]) for x in w] == [int(x) for x in R.philox4x32_10((5, 0, 0, 0), (0xa4093822, 0x299f31d0))]


def test_u01_is_inside_the_open_unit_interval():
    x = np.array([0, 0xffffffff, 0x800000ff], dtype=np.uint32)
    u = R.u01(x)
    assert u.dtype == np.float32
    assert (u > 0).all() and (u < 1).all()
    assert float(u[0]) == 2.0 ** -25
    assert float(u[2]) == 0.5                                   # 2^23 + 0.5 is a tie of float32: to even, i.e. down
    assert float(R.u01(np.uint32(0x800001ff))) == (2 ** 23 + 2) * 2.0 ** -24      # 2^23 + 1.5: to even, i.e. up
    assert float(u[1]) == 1.0 - 2.0 ** -24                      # 2^24 - 0.5 would round to 2^24: held below 1


@pytest.mark.parametrize("A", [1201, 2561])
def test_emulated_search_returns_an_acceptable_action_when_it_stays_inside_its_segment(A):
    """2000 draws: the float32 emulation of the kernel's two-level search and the fp64 inverse CDF with its a-priori rounding budget
    agree wherever the emulated fine scan does not fall off its segment's end"""
    rng = np.random.Generator(np.random.PCG64(A))
    rows = R.softmax_rows(rng, 20, A)
    u = R.row_uniforms(2000, 11)[0]
    P = np.repeat(rows, 100, axis=0)
    lo = (np.arange(2000) % 2).astype(np.int64)
    ok = R.acceptable_mask(P, lo, u)
    fell = 0
    for r in range(20):
        tb = [R._tables(rows[r], 0), R._tables(rows[r], 1)]
        for i in range(r * 100, r * 100 + 100):
            t = tb[lo[i]]
            target = u[i] * R.emulate_kernel_total(rows[r], lo[i], t)
            chosen, off = R.emulate_kernel_search(rows[r], lo[i], target, t)
            fell += off
            if not off:
                assert ok[i, chosen], (r, i, chosen, np.flatnonzero(ok[i]))
    assert fell <= 2                                             # ~1e-6 per draw: a count here means the emulation is broken


def test_emulated_total_follows_the_block_sum_order():
    """segment sums, a butterfly per 64-lane wave, then the four wave sums left to right: close to but not the serial sum"""
    row = R.softmax_rows(np.random.Generator(np.random.PCG64(1)), 1, 2561)[0]
    tot = R.emulate_kernel_total(row, 0)
    assert tot.dtype == np.float32 and abs(float(tot) - float(row.astype(np.float64).sum())) <= 16 * 2.0 ** -24
    assert float(R.emulate_kernel_total(row, 1)) < float(tot)


def test_committed_trap_inputs_hit_the_segment_end():
    """A = 1201, one softmax(2 randn) row over 4096 rows, seeds 0 .. 1023: at least 8 draws land where the serial fine scan ends an
    ulp short of the coarse scan's fl(run + part); the search as of the commit before the fix jumps to the row's last positive
    entry there, which the fp64 inverse CDF does not accept"""
    row = R.trap_row()
    traps = R.committed_traps()
    assert len(traps) >= 8, traps
    tb = R._tables(row, 0)
    total = R.emulate_kernel_total(row, 0, tb)
    last = int(np.flatnonzero(row > 0)[-1])
    for seed, r in traps:
        u = R.u01(R.row_words(np.array([r]), seed)[0])[0]
        chosen, off = R.emulate_kernel_search(row, 0, u * total, tb)
        assert off and chosen == last, (seed, r, chosen)
        ok = R.acceptable_actions(row, r % R.TRAP_T, 0, u)
        assert chosen not in ok and ok.size >= 1 and ok.max() < last, (seed, r, ok)


def _single_share(p, min_length, seed):
    rows = p.reshape(-1, p.shape[-1])
    ok = R.acceptable_mask(rows, R.lo_of_rows(rows.shape[0], p.shape[1], min_length), R.row_uniforms(rows.shape[0], seed)[0])
    assert ok.any(1).all()                                       # the reference always accepts something
    return float((ok.sum(1) == 1).mean())


@pytest.mark.parametrize("A,min_length,seed", R.parity_cases())
def test_gpu_parity_inputs_have_a_single_answer_for_most_draws(A, min_length, seed):
    """an exact comparison is only as sharp as its inputs: at least 80 % of the draws of every GPU case have exactly one acceptable
    action (a flat row at A = 2561 has ~9 % ambiguous draws under the rounding budget; the budget is not what gets adjusted)"""
    share = _single_share(R.make_case(A), min_length, seed)
    print(f"A={A} min_length={min_length} seed={seed}: single-answer share {share:.4f}")
    assert share >= 0.8


def test_gpu_trap_and_seed_inputs_have_a_single_answer_for_most_draws():
    p = np.broadcast_to(R.trap_row(), (R.TRAP_ROWS // R.TRAP_T, R.TRAP_T, R.TRAP_A))
    assert _single_share(np.ascontiguousarray(p), 0, R.committed_traps()[0][0]) >= 0.8


def test_planted_rows_are_what_they_claim():
    for A in R.CASE_SIZES:
        p = R.make_case(A)
        per = R.per_of(A)
        assert p.dtype == np.float32 and p.shape == (R.CASE_ROWS // R.CASE_T, R.CASE_T, A) and (p >= 0).all()
        assert (p[0] == 0).any() and (p[0, :, A - 1] > 0).all()
        assert (p[1, :, 1:per] == 0).all() and (p[1, :, 0] > 0).all()
        assert (p[2].sum(-1) == 1).all() and (p[2, :, A - 1] == 1).all()
        assert (p[3].sum(-1) == 1).all() and (p[3, :, 1] == 1).all()
        assert (p[4, :, 0] == np.float32(0.99)).all() and np.allclose(p[4, :, 1:].sum(-1, dtype=np.float64), 0.01, rtol=1e-5)
        assert (p[5, :, 1:] == 0).all() and (p[5, :2, 0] > 0).all() and (p[5, 2:] == 0).all()
        assert np.allclose(p[6].sum(-1, dtype=np.float64), 37.5, rtol=1e-5)
        assert (np.sort(p[7], -1)[:, :-1] == np.float32(1e-30)).all() and (p[7, :, A // 2] == 1).all()


def test_acceptable_actions_contract_on_degenerate_rows():
    z = np.zeros(7, dtype=np.float32)
    assert list(R.acceptable_actions(z, 0, 1, 0.3)) == [1] and list(R.acceptable_actions(z, 1, 1, 0.3)) == [0]
    z[0] = 0.7
    assert list(R.acceptable_actions(z, 0, 1, 0.3)) == [1] and list(R.acceptable_actions(z, 1, 1, 0.3)) == [0]
    p = np.array([0.5, 0.0, 0.25, 0.25], dtype=np.float32)
    assert list(R.acceptable_actions(p, 3, 0, 0.2)) == [0] and list(R.acceptable_actions(p, 3, 0, 0.6)) == [2]
    assert list(R.acceptable_actions(p, 0, 1, 0.2)) == [2] and list(R.acceptable_actions(p, 0, 1, 0.6)) == [3]
    assert list(R.acceptable_actions(p, 3, 0, 0.5)) == [0, 2]    # on a boundary both neighbours are acceptable, the zero entry never
    assert list(R.scanpath_length(np.array([[0, 3, 0, 1], [2, 2, 2, 2], [1, 0, 0, 0], [0, 1, 1, 1]]), 4)) == [2, 4, 1, 4]
