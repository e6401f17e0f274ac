"""Characterisation of the host layer above the evaluation kernels: the keyed calls of utils/evaluation.py from likelihood_evaluation
down, the sum tables and the batch loops of inference.py, with the eight device entry points replaced by the deterministic stand-ins
of tests/keyed_tables_cases.py (dyadic values: every sum the host forms is exact and independent of its order).  The fixture
tests/golden/keyed_tables.npz was recorded by tests/golden/make_golden_keyed_tables.py before the host layer was consolidated; the
consolidated code is held to it:
  sums of dyadics and single divisions of them, counts, keys, refusal messages, forward-call logs: equal to the bit, dtype and shape;
  "TFP_AUC" and "PM" (sums of up to 6 <= 8 non-negative quotients, worst-case reordering (n - 1) 2^-53 ~ 7.8e-16 relative): rtol 2e-15;
  the log-based saccade and turn entries ("summary", "human_summary", "JSD_*", "W1_amplitude"): equal to the bit to a direct call of
  saccade_summary / saccade_comparison (turn_summary / turn_comparison) on the result's own summed lattices (tables) -- np.log2 may
  differ in the last place between numpy builds, so no stored number is compared."""
import os

import numpy as np
import pytest

import keyed_tables_cases as C
from helpers import load_npz

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyed_tables.npz")
TOLERANT = ("TFP_AUC", "PM")


@pytest.fixture(scope="module")
def results():
    with pytest.MonkeyPatch.context() as mp:
        C.install(mp.setattr)
        return C.collect(mp.setattr)


def test_fixture_holds(results):
    got = {k: v for k, v in C.flatten(results).items() if not C.is_derived(k)}
    want = C.unpack(load_npz(GOLDEN))
    assert sorted(got) == sorted(want)
    assert any(np.isneginf(v).any() for k, v in got.items() if v.dtype == np.float64), "a -inf score is among the cases"
    assert got["lik/plain/0/NSS_nan_keys"] == 1 and got["search/model/heads/steps3/human1/0/TFP_nan"] == 1
    for k, v in got.items():
        w = want[k]
        assert v.dtype == w.dtype and v.shape == w.shape, (k, v.dtype, w.dtype, v.shape, w.shape)
        if k.rsplit("/", 1)[-1] in TOLERANT:
            assert np.allclose(v, w, rtol=2e-15, atol=0.0, equal_nan=True), (k, v, w)
        else:
            assert np.array_equal(v, w, equal_nan=v.dtype.kind == "f"), (k, v, w)


def test_forward_calls_per_loop(results):
    """whether a loop hands batch["tasks"] to the model, and that the ablation zeroes the maps of every batch: read from the results, so
    that the pinned behaviour is legible here and not only in the fixture"""
    for name, with_tasks in (("likelihood", False), ("likelihood_gold", False), ("test", False), ("search_efficiency", True),
                             ("saccade_statistics", True), ("turn_statistics", True)):
        for tasks in (0, 1):
            for ablate in (0, 1):
                log = results[f"loop/{name}/tasks{tasks}/ablate{ablate}/forward_log"]
                assert log.tolist() == [[3 if with_tasks and tasks else 2, ablate]] * 2, (name, tasks, ablate, log)


def _against(case, label, lattice, by_label, name="lattice"):
    kind = case.rsplit("/", 1)[-1]
    if kind == "dict":
        return by_label.get(label)
    if case == "turn/eval/table":                                    # result() without a table: compared to its own human side
        return None
    return lattice if label is None and (kind == name or case.startswith("loop/")) else None


def test_saccade_derived_entries(results):
    from scanpaths_amd.utils.evaltools.saccade_statistics import saccade_comparison, saccade_summary
    kw = dict(amplitude_edges=C.EDGES, n_directions=C.DIRECTIONS)
    human = results["saccade/human/groups"][0]
    lattice, by_label = human["human_lattice_sum"], {None: human["human_lattice_sum"], "find": human["by_group"]["find"]["human_lattice_sum"]}
    seen = 0
    for case, res in results.items():
        if not (case.startswith("saccade/") or case.startswith("loop/saccade_statistics/")) or case.endswith("forward_log"):
            continue
        means = res[0] if isinstance(res, tuple) else res
        for label, node in [(None, means)] + list(means.get("by_group", {}).items()):
            want = {}
            if not case.endswith("/bare"):
                if "human_lattice_sum" in node:
                    want["human_summary"] = saccade_summary(node["human_lattice_sum"], C.FRAME, **kw)
                if "lattice_sum" in node:
                    want["summary"] = saccade_summary(node["lattice_sum"], C.FRAME, **kw)
                    other = _against(case, label, lattice, by_label)
                    other = node.get("human_lattice_sum") if other is None else other
                    if other is not None:
                        want.update(saccade_comparison(node["lattice_sum"], other, C.FRAME, **kw))
            got = {k: v for k, v in node.items() if k in C.DERIVED}
            assert sorted(got) == sorted(want), (case, label)
            got, want = C.flatten(got), C.flatten(want)
            for k in want:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (case, label, k)
            seen += len(want)
    assert seen > 100


def test_turn_derived_entries(results):
    from scanpaths_amd.utils.evaltools.turn_statistics import turn_comparison, turn_summary
    human = results["turn/human/groups"][0]
    table, by_label = human["human_table_sum"], {None: human["human_table_sum"], "find": human["by_group"]["find"]["human_table_sum"]}
    seen = 0
    for case, res in results.items():
        if not (case.startswith("turn/") or case.startswith("loop/turn_statistics/")) or case.endswith("forward_log"):
            continue
        means = res[0] if isinstance(res, tuple) else res
        for label, node in [(None, means)] + list(means.get("by_group", {}).items()):
            want = {}
            if "human_table_sum" in node:
                want["human_summary"] = turn_summary(node["human_table_sum"])
            if "table_sum" in node:
                want["summary"] = turn_summary(node["table_sum"])
                other = _against(case, label, table, by_label, "table")
                other = node.get("human_table_sum") if other is None else other
                if other is not None:
                    want.update(turn_comparison(node["table_sum"], other))
            got = {k: v for k, v in node.items() if k in C.DERIVED}
            assert sorted(got) == sorted(want), (case, label)
            got, want = C.flatten(got), C.flatten(want)
            for k in want:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (case, label, k)
            seen += len(want)
    assert seen > 100
