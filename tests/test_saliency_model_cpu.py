"""CPU-only checks of the closed-form saliency layer: the third library's header, binding and exports name the same
functions and leave the two pinned libraries alone; its launcher refuses bad arguments before any launch; every argument refusal of
the Python layer is raised before a device or a library is touched; expected_durations and SaliencyModelTable hold answers worked out
by hand; and the Python restatement of the closed form (tests/expected_maps_ref.py) equals the exhaustive enumeration of all action
sequences under the sampler's rule in exact rational arithmetic -- which makes it independent of the closed form's own reasoning."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import abi
import expected_maps_ref as X
import model_abi
import stats_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sp_model_abi_version": ("int", 0), "sp_model_max_fixations": ("int", 0), "sp_model_max_cells": ("int", 0),
         "sp_model_fixation_expectation_workspace": ("int64_t", 6), "sp_model_fixation_expectation": ("int", 18)}


def S():
    from scanpaths_amd.utils.evaltools import saliency_maps
    return saliency_maps


# ---- the third library --------------------------------------------------------------------------------------------------------------------
def test_model_header_binding_and_exports_agree():
    """three-way agreement, and the names of this pull request are there; neither the number of exports nor the exact set is pinned:
    the next closed-form statistic joins this library"""
    from scanpaths_amd import hip
    decls = model_abi.header_decls()
    assert set(decls) == set(hip.MODEL_SIGNATURES) == set(model_abi.exported_functions(model_abi.lib_path())) >= set(NAMES)
    assert all(n.startswith("sp_model_") for n in decls)
    for name, (ret, args) in decls.items():
        cret, cargs = hip.MODEL_SIGNATURES[name]
        assert cret is model_abi.KINDS[ret] and len(cargs) == len(args), (name, cret, cargs)
        for a, c in zip(args, cargs):
            assert c is model_abi.want_ctype(a), (name, a, c)
    for name, (ret, nargs) in NAMES.items():
        assert decls[name][0] == ret and len(decls[name][1]) == nargs, (name, decls[name])
    lib = model_abi.raw_lib()
    assert model_abi.header_version() == hip.MODEL_ABI_VERSION == lib.sp_model_abi_version() >= 1
    from scanpaths_amd.utils.evaltools import _args, _batch
    assert lib.sp_model_max_fixations() == _batch.MAX_FIXATIONS == X.MAX_FIXATIONS == 64
    assert lib.sp_model_max_cells() == _args.MAX_CELLS == X.MAX_CELLS == 2048
    note = model_abi.header_comment()
    assert "next closed-form statistic" in note and "SP_MODEL_ABI_VERSION bumped" in note and "not into a fourth library" in note
    lines = open(os.path.join(ROOT, "scanpaths_amd", "csrc", "Makefile")).read().splitlines()
    assert "all: $(OUT) $(STATS_OUT)" in lines and "all: $(MODEL_OUT)" in lines
    assert "MODEL_SRCS = scanexpect.hip" in lines
    assert not any("scanexpect" in line for line in lines if line.startswith(("SRCS", "STATS_SRCS")))
    assert [line for line in lines if line.startswith("\trm -f")][0].split().count("$(MODEL_OUT)") == 1
    assert "scanexpect.hip" in open(os.path.join(ROOT, "scanpaths_amd", "csrc", "scan_common.h")).read().split("#pragma once")[0]


def test_the_pinned_libraries_are_untouched_and_share_no_symbol():
    from scanpaths_amd import hip
    assert len(hip.SIGNATURES) == 154 and hip.ABI_VERSION == abi.header_abi_version() == 4
    main, stats = set(abi.exported_functions()), set(stats_abi.exported_functions(stats_abi.lib_path()))
    model = set(model_abi.exported_functions(model_abi.lib_path()))
    assert len(main) == 154 and len(stats) == 5 and hip.STATS_ABI_VERSION == stats_abi.header_version() == 1
    assert not main & model and not stats & model and not main & stats
    assert not set(hip.MODEL_SIGNATURES) & (set(hip.SIGNATURES) | set(hip.STATS_SIGNATURES))
    assert not set(model_abi.header_decls()) & (set(abi.header_symbols()) | set(stats_abi.header_decls()))


def test_model_lib_loads_once_and_refuses_a_missing_or_mismatched_library(monkeypatch, tmp_path):
    from scanpaths_amd import hip
    model_abi.lib_path()
    first = hip.model_lib()
    assert hip.model_lib() is first
    assert first.sp_model_fixation_expectation.argtypes == hip.MODEL_SIGNATURES["sp_model_fixation_expectation"][1]
    assert hip.MODEL_HEADER_PATH == model_abi.HEADER
    monkeypatch.setattr(hip, "_model_lib", None)
    monkeypatch.setattr(hip, "MODEL_LIB_PATH", str(tmp_path / "libscanpaths_amd_model.so"))
    with pytest.raises(RuntimeError, match=r"is missing: build it with .*g\.build\(\)"):
        hip.model_lib()
    monkeypatch.undo()
    monkeypatch.setattr(hip, "_model_lib", None)
    monkeypatch.setattr(hip, "MODEL_ABI_VERSION", hip.MODEL_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match=f"ABI version {first.sp_model_abi_version()}, this binding expects"):
        hip.model_lib()
    monkeypatch.undo()
    assert hip.model_lib() is first


def test_launcher_refuses_bad_arguments_without_a_device():
    """SP_ENULL (-2) / SP_EINVAL (-1) come before the launch, so on a machine without a GPU too.  Every call below is a refused one."""
    lib = model_abi.raw_lib()
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks

    def with_(base, **kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.sp_model_fixation_expectation(*a)

    # (probs, step_weight, row_group, R, T, Hm, Wm, ngroups, min_length, max_steps, cell_pixel, H, W, work, maps, fixations, bad, stream)
    ok = [p, p, p, 3, 4, 30, 40, 2, 1, 6, p, 240, 320, p, p, p, p, None]
    for k in (0, 2, 10, 13, 14, 15, 16):                            # every pointer but step_weight
        assert with_(ok, **{f"a{k}": None}) == -2, k
        assert with_(ok, **{f"a{k}": None, "a1": None}) == -2, k
    for k, bad in ((3, -1), (3, -7), (4, 0), (4, -2), (5, 0), (5, -30), (5, 52), (6, 0), (6, -1), (6, 69), (6, 1 << 20), (7, -1), (8, -1),
                   (8, -9), (9, 0), (9, -5), (9, 65), (11, 0), (11, -240), (12, 0), (12, -1), (11, 1 << 23)):
        assert with_(ok, **{f"a{k}": bad}) == -1, (k, bad)          # 52 x 40 and 30 x 69 cells: above 2048; 2^23 x 320 pixels: outside int
        assert with_(ok, **{f"a{k}": bad, "a1": None}) == -1, (k, bad)
    assert with_(ok, a5=32, a6=65) == -1                            # 2080 cells
    assert with_(ok, a11=46341, a12=46341) == -1                    # 2^31 < 46341^2: H W outside int
    assert with_(ok, a0=None, a3=-1) == -2                          # NULL is answered before a bad scalar
    assert with_(ok, a16=None, a9=0) == -2
    ws = lib.sp_model_fixation_expectation_workspace
    assert ws(3, 4, 30, 40, 2, 6) >= 2 * 3 * 4 + 2 * 1200 and ws(3, 40, 30, 40, 2, 6) == ws(3, 6, 30, 40, 2, 6)      # Tm = min(T, max_steps)
    assert ws(0, 1, 1, 1, 0, 1) >= 0
    for bad in ((-1, 4, 30, 40, 2, 6), (3, 0, 30, 40, 2, 6), (3, 4, 0, 40, 2, 6), (3, 4, 32, 65, 2, 6), (3, 4, 30, 40, -1, 6),
                (3, 4, 30, 40, 2, 0), (3, 4, 30, 40, 2, 65)):
        assert ws(*bad) == -1, bad


def test_public_surface():
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    empty, KW = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(S().expected_cell_pixels).parameters
    assert list(p) == ["map_shape", "frame_size", "output_shape"] and p["output_shape"].default is None
    p = inspect.signature(S().expected_fixation_maps).parameters
    assert list(p) == ["probs", "row_groups", "n_groups", "min_length", "max_steps", "frame_size", "output_shape", "map_shape", "step_weight"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps", "frame_size"))
    assert all(p[k].kind is KW and p[k].default is None for k in ("output_shape", "map_shape", "step_weight"))
    assert list(inspect.signature(S().expected_durations).parameters) == ["log_normal_mu", "log_normal_sigma2"]
    p = inspect.signature(S().scanpath_saliency).parameters
    assert p["prediction"].default == "scanpaths" and p["pred_maps"].default is None and p["pred_maps"].kind is KW
    assert p["pred_weight"].default == "count" and p["mode"].default == "constant" and p["truncate"].default == 4.0   # defaults stay
    p = inspect.signature(E.saliency_model_evaluation).parameters
    assert list(p) == ["predict", "fix_vectors", "keys", "performances", "image_keys", "sigma", "min_length", "max_steps", "pred_weight",
                       "frame_size", "map_shape", "extra_metrics", "kw"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("sigma", "min_length", "max_steps"))
    assert p["pred_weight"].default == "count" and p["frame_size"].default == (240, 320) and p["map_shape"].default is None
    assert issubclass(E.SaliencyModelTable, E._SumTable)
    p = inspect.signature(inference.run_saliency_loop).parameters
    assert list(p) == ["model", "loader", "sigma", "min_length", "max_steps", "pred_weight", "extra_metrics", "ablate_attention_info",
                       "frame_size", "map_shape", "kw"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("sigma", "min_length", "max_steps"))
    assert p["frame_size"].default == (240, 320) and p["ablate_attention_info"].default is False


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from scanpaths_amd import hip

    def no_lib(*a, **k):
        raise AssertionError("validation must come first")

    monkeypatch.setattr(S(), "_device", no_lib)
    for name in ("lib", "stats_lib", "model_lib"):
        monkeypatch.setattr(hip, name, no_lib)


def test_map_refusals_come_before_any_device_call(monkeypatch):
    _no_device(monkeypatch)
    maps, pixels = S().expected_fixation_maps, S().expected_cell_pixels
    probs = torch.full((2, 3, 1 + 6), 0.1)
    ok = dict(min_length=1, max_steps=4, frame_size=(20, 45), map_shape=(2, 3))
    for missing in ("min_length", "max_steps", "frame_size"):
        with pytest.raises(TypeError):
            maps(probs, [0, 0], 1, **{k: v for k, v in ok.items() if k != missing})
    for bad in (0, -1, 1.5, True, None, 65):
        with pytest.raises(ValueError, match="max_steps"):
            maps(probs, [0, 0], 1, **dict(ok, max_steps=bad))
    for bad in (-1, 0.5, None, True):
        with pytest.raises(ValueError, match="min_length"):
            maps(probs, [0, 0], 1, **dict(ok, min_length=bad))
    for bad in ((0, 45), (20, float("inf")), (float("nan"), 45), (20.5, 45)):
        with pytest.raises(ValueError, match="frame_size"):
            maps(probs, [0, 0], 1, **dict(ok, frame_size=bad))
        with pytest.raises(ValueError, match="frame_size"):
            pixels((2, 3), bad)
    for bad in ((0, 5), (3,), (3, -5), (2.5, 4), (1 << 16, 1 << 16)):
        with pytest.raises(ValueError, match="output_shape"):
            maps(probs, [0, 0], 1, **dict(ok, output_shape=bad))
        with pytest.raises(ValueError, match="output_shape"):
            pixels((2, 3), (20, 45), bad)
    for bad in ((0, 5), (3,), (2.5, 4), None, (32, 65)):
        with pytest.raises(ValueError, match="map_shape|kernel limit"):
            pixels(bad, (20, 45))
    for bad in ((3, 3), (1, 7), (0, 6)):
        with pytest.raises(ValueError, match="map_shape"):
            maps(probs, [0, 0], 1, **dict(ok, map_shape=bad))
    with pytest.raises(ValueError, match="map_shape is required"):
        maps(probs, [0, 0], 1, **dict(ok, map_shape=None))             # only 1201 actions have a default
    with pytest.raises(ValueError, match="kernel limit"):
        maps(torch.zeros(1, 1, 1 + 2080), [0], 1, **dict(ok, map_shape=(32, 65)))
    for bad in (np.zeros((2, 3, 7)), torch.zeros(2, 7), torch.zeros(2, 0, 7), torch.zeros(2, 3, 1)):
        with pytest.raises(ValueError, match="probs"):
            maps(bad, [0, 0], 1, **ok)
    for bad in ([1, 0], [-1, 0], [0, 2]):
        with pytest.raises(ValueError, match="out of range"):
            maps(probs, bad, 1, **ok)
    with pytest.raises(ValueError, match="one group per row"):
        maps(probs, [0], 1, **ok)
    for bad in (0, -1, None, 1.5):
        with pytest.raises(ValueError, match="n_groups"):
            maps(probs, [0, 0], bad, **ok)
    one = np.ones((2, 3))
    for bad in (np.ones((2, 4)), np.ones(6), np.where(np.eye(2, 3) > 0, np.nan, one), np.where(np.eye(2, 3) > 0, np.inf, one),
                np.where(np.eye(2, 3) > 0, -1e-300, one)):
        with pytest.raises(ValueError, match="step_weight"):
            maps(probs, [0, 0], 1, **dict(ok, step_weight=bad))
    res = maps(torch.zeros(0, 3, 7), [], 2, **dict(ok, output_shape=(4, 9)))                # no row: zero maps, no device
    assert res["maps"].dtype == torch.float64 and tuple(res["maps"].shape) == (2, 4, 9) and not res["maps"].any()
    assert res["fixations"].dtype == np.float64 and res["bad"].dtype == np.int32 and len(res["fixations"]) == len(res["bad"]) == 0


def test_scoring_and_keyed_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    _no_device(monkeypatch)
    sal = S().scanpath_saliency
    sp = np.array([[1.0, 1.0, 0.2], [5.0, 3.0, 0.3]])
    good = np.ones((1, 4, 6))
    with pytest.raises(ValueError, match="prediction"):
        sal([sp], [0], [], [], (4, 6), 1.0, prediction="map")
    for prediction in ("scanpaths", "centre_prior"):
        with pytest.raises(ValueError, match="pred_maps is read with prediction='maps' only"):
            sal([sp], [0], [], [], (4, 6), 1.0, prediction=prediction, pred_maps=good)
    with pytest.raises(ValueError, match="needs pred_maps"):
        sal([sp], [0], [], [], (4, 6), 1.0, prediction="maps")
    with pytest.raises(ValueError, match="takes no predicted scanpaths"):
        sal([sp], [0], [sp], [0], (4, 6), 1.0, prediction="maps", pred_maps=good)
    for bad in (np.ones((2, 4, 6)), np.ones((1, 6, 4)), np.ones((4, 6)), np.ones((1, 4, 6), np.float32), torch.ones(1, 4, 6)):
        with pytest.raises(ValueError, match="float64"):
            sal([sp], [0], [], [], (4, 6), 1.0, prediction="maps", pred_maps=bad)
    with pytest.raises(ValueError, match="float64"):
        sal([sp], [0], [], [], (8, 12), 1.0, output_shape=(4, 6), prediction="maps", pred_maps=np.ones((1, 8, 12)))
    ev = E.saliency_model_evaluation
    predict = {"all_actions_prob": torch.full((2, 3, 7), 0.1)}
    fv, keys = [[sp], [sp, sp]], ["a", "b"]
    ok = dict(sigma=1.0, min_length=1, max_steps=4, frame_size=(20, 45), map_shape=(2, 3))
    for missing in ("sigma", "min_length", "max_steps"):
        with pytest.raises(TypeError):
            ev(predict, fv, keys, **{k: v for k, v in ok.items() if k != missing})
    with pytest.raises(ValueError, match="a union over samples, not an expectation"):
        ev(predict, fv, keys, **dict(ok, pred_weight="binary"))
    with pytest.raises(ValueError, match="pred_weight"):
        ev(predict, fv, keys, **dict(ok, pred_weight="sum"))
    for bad in (0, 65, None):
        with pytest.raises(ValueError, match="max_steps"):
            ev(predict, fv, keys, **dict(ok, max_steps=bad))
    with pytest.raises(ValueError, match="min_length"):
        ev(predict, fv, keys, **dict(ok, min_length=-1))
    with pytest.raises(ValueError, match="one key per sample"):
        ev(predict, fv, ["a"], **ok)
    with pytest.raises(ValueError, match="one performance per subject"):
        ev(predict, fv, keys, [[True], [True]], **ok)
    with pytest.raises(ValueError, match="one image key per sample"):
        ev(predict, fv, keys, None, ["i"], **ok)
    with pytest.raises(ValueError, match="on two images"):
        ev(predict, fv, ["a", "a"], None, ["i", "j"], **ok)
    with pytest.raises(ValueError, match="predict lacks 'log_normal_mu'"):
        ev(predict, fv, keys, **dict(ok, pred_weight="duration"))
    with pytest.raises(ValueError, match="predict lacks 'good_all_actions_prob'"):
        ev(predict, fv, keys, [[True], [True, False]], **ok)
    with pytest.raises(ValueError, match="this function's to set"):
        ev(predict, fv, keys, **dict(ok, prediction="scanpaths"))
    for bad in (("IG",), ("CC", "sAUC")):
        with pytest.raises(ValueError, match="a batch is not the dataset.*saliency_model_evaluation"):
            inference.run_saliency_loop(None, [], sigma=1.0, min_length=1, max_steps=4, extra_metrics=bad)
    with pytest.raises(TypeError):
        inference.run_saliency_loop(None, [], min_length=1, max_steps=4)


def test_a_missing_device_is_an_error_not_a_fallback(monkeypatch):
    from scanpaths_amd import hip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hip.HipError, match="no CPU path"):
        S().expected_cell_pixels((2, 3), (20, 45), (4, 10))                                   # a table no other test asks for
    with pytest.raises(hip.HipError, match="no CPU path"):
        S().expected_fixation_maps(torch.full((1, 2, 7), 0.1), [0], 1, min_length=0, max_steps=2, frame_size=(20, 45), map_shape=(2, 3))


# ---- hand values --------------------------------------------------------------------------------------------------------------------------
def test_expected_durations_by_hand():
    mu = torch.tensor([[0.0, 1.0, -2.0], [0.5, 0.0, 3.0]])
    s2 = torch.tensor([[0.0, 2.0, 1.0], [-1.0, 0.5, 0.0]])
    got = S().expected_durations(mu, s2)
    want = [[1.0, math.exp(3.0), math.exp(-1.5)], [math.e, math.exp(0.125), math.exp(3.0)]]     # exp(mu + s2^2 / 2); the sign of s2 drops out
    assert got.dtype == np.float64 and got.shape == (2, 3)
    assert np.allclose(got, want, rtol=4 * 2.0 ** -53, atol=0) and got[0, 0] == 1.0
    # float32 inputs are widened exactly, then everything is float64: 0.1f is not 0.1
    m32 = np.float64(np.float32(0.1))
    assert S().expected_durations(torch.tensor([[0.1]]), torch.tensor([[0.0]]))[0, 0] == np.exp(m32) != np.exp(0.1)
    assert np.array_equal(S().expected_durations(mu.numpy(), s2.numpy()), got)
    assert np.array_equal(S().expected_durations(mu.double(), s2.half()), got)                # any float dtype is read as float32
    with pytest.raises(ValueError, match="one shape"):
        S().expected_durations(mu, s2[:, :2])
    with pytest.raises(ValueError, match=r"\[R, T\]"):
        S().expected_durations(mu[0], s2[0])


def test_saliency_model_table_by_hand():
    from scanpaths_amd.utils.evaluation import SaliencyModelTable
    a = {"NSS": 1.5, "NSS_sum": 3.0, "NSS_count": 2, "NSS_nan": 1, "CC": float("nan"), "CC_sum": 0.0, "CC_count": 0, "CC_nan": 3,
         "rows_count": 5, "rows_bad": 1, "fixations_sum": 10.0}
    b = {"NSS": 0.25, "NSS_sum": 0.25, "NSS_count": 1, "NSS_nan": 0, "CC": 0.5, "CC_sum": 1.5, "CC_count": 3, "CC_nan": 0,
         "rows_count": 3, "rows_bad": 0, "fixations_sum": 2.0}
    t = SaliencyModelTable()
    assert t.result() == {}
    t.add(a)
    r = t.result()
    assert r["NSS"] == 1.5 and math.isnan(r["CC"]) and r["fixations_per_row"] == 2.0 and r["rows_bad"] == 1
    t.add(b)
    r = t.result()
    assert r["NSS_sum"] == 3.25 and r["NSS_count"] == 3 and r["NSS"] == 3.25 / 3 and r["NSS_nan"] == 1
    assert r["CC"] == 0.5 and r["CC_count"] == 3 and r["CC_nan"] == 3
    assert r["rows_count"] == 8 and r["rows_bad"] == 1 and r["fixations_sum"] == 12.0 and r["fixations_per_row"] == 1.5
    assert a["NSS_sum"] == 3.0 and "fixations_per_row" not in a                              # the caller's dicts are not written to
    empty = SaliencyModelTable()
    empty.add({"NSS": float("nan"), "NSS_sum": 0.0, "NSS_count": 0, "NSS_nan": 2, "rows_count": 0, "rows_bad": 2, "fixations_sum": 0.0})
    assert math.isnan(empty.result()["NSS"]) and math.isnan(empty.result()["fixations_per_row"])


def test_cell_pixel_restatement_by_hand():
    assert X.cell_pixels((30, 40), (240, 320)).reshape(30, 40)[2, 3] == (2 * 8 + 4) * 320 + 3 * 8 + 4     # the centre of an 8 x 8 cell
    assert X.cell_pixels((1, 1), (75, 100)).tolist() == [37 * 100 + 50]
    assert X.cell_pixels((2, 3), (20, 45), (2, 2)).tolist() == [0, 1, 1, 2, 3, 3]              # x = 7.5, 22.5, 37.5 of 45: 22.5 * 2 / 45 = 1.0
    assert X.cell_pixels((2, 2), (75, 100), (1, 1)).tolist() == [0, 0, 0, 0]
    t = X.cell_pixels((5, 7), (100, 300), (2, 2)).reshape(5, 7)
    assert (np.bincount(t.reshape(-1), minlength=4) > 1).all() and len(np.unique(X.cell_pixels((5, 7), (100, 300)))) == 35


# ---- the restatement against exhaustive enumeration ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("max_steps", ["below", "above"])
@pytest.mark.parametrize("min_length", ["0", "1", "T+1"])
@pytest.mark.parametrize("shape,T", [((1, 1), 3), ((2, 3), 4), ((2, 2), 5)])
def test_restatement_equals_the_exhaustive_enumeration(shape, T, min_length, max_steps, weighted):
    """All (1 + P)^T action sequences under the sampler's rule (terminate masked for t < min_length, the first terminate ends the
    scanpath, only the first max_steps fixations count, fixation t weighs s_t), weighted in exact rationals: every pixel of the map
    and the expected number of fixations, at the frame's own resolution and at an output shape where several cells share a pixel.
    The bound is relative, gamma_n = n u / (1 - n u) with u = 2^-53 and n = (1 + P)^T, the terms the enumeration adds into one entry,
    plus the restatement's own roundings as expected_maps_ref.roundings counts them from the operations (all terms are non-negative;
    the one subtraction, 1.0 - q_t, multiplies the error of q_t by p_0 / Z, which the inputs below keep <= 20: cells >= 0.05, p_0 <= 1,
    asserted).  It is derived, not fitted: the printed worst error is orders of magnitude below it."""
    Hm, Wm = shape
    P = Hm * Wm
    min_length = {"0": 0, "1": 1, "T+1": T + 1}[min_length]
    K = T - 1 if max_steps == "below" else T + 2
    frame = (20, 45) if shape == (2, 3) else (75, 100)
    g = np.random.default_rng(17 * T + P)
    probs = g.uniform(0.05, 1.0, (1, T, 1 + P)).astype(np.float32)       # unnormalised on purpose
    assert (probs[0, :, 0] / probs[0, :, 1:].sum(1)).max() <= 20.0
    weight = g.uniform(0.1, 3.0, (1, T)) if weighted else None
    for out in (None, (1, 2) if P > 1 else (3, 2)):
        H, W = frame if out is None else out
        table = X.cell_pixels(shape, frame, out)
        share = int(np.bincount(table, minlength=H * W).max())
        assert share > 1 or out is None or P == 1
        want, fixations = X.enumerated_map(probs[0], None if weight is None else weight[0], min_length, K, table, H * W)
        wantf = np.array([float(v) for v in want]).reshape(H, W)
        got = X.expected_fixation_maps(probs, weight, [0], 1, min_length, K, table, H, W)
        bound = X.bound(P, T, share, 20.0)
        assert got["bad"].tolist() == [0] and got["maps"].shape == (1, H, W)
        err = np.abs(got["maps"][0] - wantf)
        print(shape, T, min_length, K, out, "worst relative error", float((err / np.maximum(wantf, 1e-300)).max()), "bound", bound)
        assert (err <= bound * wantf).all(), (got["maps"][0], wantf)
        assert abs(got["fixations"][0] - float(fixations)) <= bound * float(fixations)
        assert np.count_nonzero(wantf) == len(np.unique(table)) and (wantf >= 0).all()      # a pixel without a cell is exactly 0
        if weight is None:
            assert abs(wantf.sum() - float(fixations)) <= bound * float(fixations)
            assert float(fixations) <= min(T, K) and (float(fixations) >= min(min_length, T, K))
