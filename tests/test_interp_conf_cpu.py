"""Confidence of interpolated scores, host side: utils.image.confidence_interpolated_host (the float64 specification csrc/scores_confidence.hip
restates) against independent restatements -- labels_interpolated_host, torch's float64 interpolation and softmax, a stable sort of the
interpolated values, confidence_host at the identity geometry; the known answers; the GUARD conditions that let test_interp_conf_gpu.py demand
equality of all five outputs; and the mutant matrix: the case table of interp_conf_ref.py tells the specification apart from each plausible
wrong kernel.  (GPU side: test_interp_conf_gpu.py.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

import interp_conf_ref as ref
import interp_ref as iref
from test_frames_u8_gpu import SMALL
from test_interp_labels_cpu import _mutant_taps

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("accel_scores_confidence_interp", "accel_model_confidence_interp")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _finish(v, is_prob=False, last=False, margin_dtype=np.float64):
    """(labels, conf, margin, second) of values n x ncls x h x w, restated with a stable sort: descending, the earlier index first among equals
    (last: the later index first); margin_dtype: the values are rounded to it before the subtraction"""
    ncls = v.shape[1]
    if last:
        order = ncls - 1 - np.argsort(-v[:, ::-1], axis=1, kind="stable")
    else:
        order = np.argsort(-v, axis=1, kind="stable")
    best, runner = order[:, 0], order[:, 1]
    top1 = np.take_along_axis(v, best[:, None], 1)[:, 0]
    top2 = np.take_along_axis(v, runner[:, None], 1)[:, 0]
    margin = (top1.astype(margin_dtype) - top2.astype(margin_dtype)).astype(np.float32)
    if is_prob:
        scaled = 256.0 * top1
    else:
        scaled = 256.0 / np.exp(v - top1[:, None]).sum(axis=1)
    conf = np.minimum(255.0, np.floor(scaled)).astype(np.uint8)
    return best.astype(np.uint8), conf, margin, runner.astype(np.uint8)


def _values_with(case, ty, tx, dtype=np.float64, whole_map=False):
    """the specification's blend over given taps, in `dtype`"""
    s = ref.scores(case)
    if not whole_map:
        s = s[:, :, :case.out_h, :case.out_w]
    s = s.astype(dtype)
    (y0, y1, fy), (x0, x1, fx) = ty, tx
    fy, fx = fy.astype(dtype)[:, None], fx.astype(dtype)[None, :]
    one = dtype(1)
    r0, r1 = s[:, :, y0], s[:, :, y1]
    top = r0[..., x0] * (one - fx) + r0[..., x1] * fx
    bot = r1[..., x0] * (one - fx) + r1[..., x1] * fx
    v = top * (one - fy) + bot * fy
    assert v.dtype == dtype
    return v


def _spec_taps(case):
    return image.interpolation_taps(case.h, case.out_h), image.interpolation_taps(case.w, case.out_w)


def _some_cases():
    """one operator case per class count and scale, over different geometries"""
    return [ref.small_case(*SMALL[(4 * i + j) % len(SMALL)], ncls=ncls, n=2, scale=s) for i, ncls in enumerate(ref.NCLS) for j, s in enumerate(ref.SCALES)]


def _step16():
    return [c for c in ref.dyadic_cases() if c.kind == "step" and c.h == 16][0]


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from accel_amd import runtime
    from accel_amd.core import results
    hdr = open(os.path.join(ROOT, "include", "accel_hip.h")).read()
    declared = set(re.findall(r"\b(accel_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, "include/accel_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libaccel_hip.so does not export %s" % name
    runtime.lib()
    assert set(ENTRY_POINTS) <= set(runtime.EXPORTS)
    assert len(runtime.EXPORTS["accel_scores_confidence_interp"]) == 20 and len(runtime.EXPORTS["accel_model_confidence_interp"]) == 17
    assert hasattr(runtime.Context, "scores_confidence_interp")
    assert hasattr(runtime.Model, "confidence_interp") and hasattr(runtime.Model, "confidence_interp_device")
    params = inspect.signature(results.confidence).parameters
    assert params["interpolate"].default is False and params["labels"].default is False
    assert list(params)[:6] == ["handle", "like", "margin", "second", "hist", "probabilities"]        # the existing arguments keep their places
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


def test_labels_without_interpolate_is_refused():
    from accel_amd.core import results
    with pytest.raises(ValueError, match="interpolate=True"):
        results.confidence(object(), None, labels=True)


def test_demo_takes_the_flag_combination():
    from accel_amd import demo
    with pytest.raises(SystemExit) as e:
        demo.main(["--raw-frames", "--finish-on-gpu", "--interpolate", "--confidence", "--help"])
    assert e.value.code == 0


# ---- the specification against independent restatements ------------------------------------------------------------------------------------------
def test_the_values_of_this_table_are_those_of_interp_ref():
    for case in ref.near_tie_cases() + ref.dyadic_cases() + _some_cases():
        assert np.array_equal(ref.scores(case), iref.scores(case)) and np.array_equal(ref.values(case), iref.values(case)), ref.ident(case)


@pytest.mark.parametrize("case", _some_cases() + ref.near_tie_cases() + ref.dyadic_cases() + ref.prob_cases()[:4] + ref.known_cases()[:6], ids=ref.ident)
def test_labels_are_those_of_labels_interpolated_host(case):
    want = image.labels_interpolated_host(ref.scores(case), case.out_h, case.out_w, case.h, case.w)
    got = ref.reference(case)[0]
    assert got.dtype == np.uint8 and got.shape == (case.n, case.h, case.w) and np.array_equal(got, want)


@pytest.mark.parametrize("case", _some_cases(), ids=ref.ident)
def test_conf_is_the_softmax_of_torch_interpolate(case):
    """torch's float64 bilinear interpolation rounds differently: its values lie within d = 8e-12 x scale of the specification's (the bound
    test_interp_labels_cpu.py asserts).  A softmax probability moves by at most a factor exp(2 d), so 256 * p by less than 512 d x 1.01: every
    pixel whose 256 * p is farther than that from an integer (or above 255) must have the same byte, the others may be one level off."""
    import torch
    import torch.nn.functional as F
    s = torch.from_numpy(ref.scores(case)[:, :, :case.out_h, :case.out_w].astype(np.float64))
    v = F.interpolate(s, size=(case.h, case.w), mode="bilinear", align_corners=False)
    d = 8e-12 * case.scale
    assert np.abs(v.numpy() - ref.values(case)).max() <= d
    scaled = 256.0 * torch.softmax(v, dim=1).max(dim=1).values.numpy()
    want = np.minimum(255.0, np.floor(scaled)).astype(np.int64)
    conf = ref.reference(case)[1].astype(np.int64)
    eps = 512.0 * d * 1.01
    sure = (np.abs(scaled - np.rint(scaled)) > eps) | (scaled > 255.0 + eps)          # (saturated: 255 whatever the last bits say)
    assert sure.mean() > 0.99
    assert np.array_equal(conf[sure], want[sure]), int(np.count_nonzero(conf[sure] != want[sure]))
    assert np.abs(conf - want).max() <= 1


@pytest.mark.parametrize("case", _some_cases() + ref.near_tie_cases() + ref.dyadic_cases() + ref.prob_cases()[:4], ids=ref.ident)
def test_second_margin_and_conf_are_the_sort_based_restatement(case):
    labels, conf, margin, second, _ = ref.reference(case)
    wl, wc, wm, ws = _finish(ref.values(case), is_prob=ref.is_prob(case))
    assert np.array_equal(labels, wl) and second.dtype == np.uint8 and np.array_equal(second, ws)
    assert margin.dtype == np.float32 and np.array_equal(_bits(margin), _bits(wm)) and (margin >= 0).all()
    # (another summation: numpy's pairwise sum over the classes; equal bytes because of guard condition (a))
    assert np.array_equal(conf, wc)


@pytest.mark.parametrize("case", _some_cases()[:4] + ref.multiblock_cases() + ref.prob_cases()[:2], ids=ref.ident)
def test_hist_counts_the_source_pixels_of_every_level(case):
    conf, hist = ref.reference(case)[1], ref.reference(case)[4]
    assert hist.dtype == np.uint64 and hist.shape == (case.n, 256)
    for f in range(case.n):
        assert np.array_equal(hist[f].astype(np.int64), np.bincount(conf[f].reshape(-1), minlength=256))
        assert int(hist[f].sum()) == case.h * case.w


# ---- the identity geometry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.crop_cases() + [ref.multiblock_cases()[1]] + [ref.small_case(*SMALL[0], ncls=k, n=3, scale=s) for k in ref.NCLS
                                                                                   for s in ref.SCALES], ids=ref.ident)
def test_identity_is_confidence_host_and_the_crop_of_the_argmax(case):
    """every weight is 0: all five outputs are those of the nearest rule -- the margin, there one fp32 subtraction of two stored values, bit for
    bit at all four scales"""
    assert (case.h, case.w) == (case.out_h, case.out_w)
    s = ref.scores(case)
    labels, conf, margin, second, hist = ref.reference(case)
    wc, wm, ws, wh = image.confidence_host(s, case.out_h, case.out_w, case.h, case.w)
    assert np.array_equal(labels, np.argmax(s, axis=1)[:, :case.h, :case.w].astype(np.uint8))
    assert np.array_equal(conf, wc) and np.array_equal(second, ws) and np.array_equal(hist, wh)
    assert np.array_equal(_bits(margin), _bits(wm)), int(np.count_nonzero(_bits(margin) != _bits(wm)))


def test_identity_of_stored_probabilities():
    case = ref.prob_cases()[0]
    assert (case.h, case.w) == (case.out_h, case.out_w) and ref.is_prob(case)
    got = ref.reference(case)
    want = image.confidence_host(ref.scores(case), case.out_h, case.out_w, case.h, case.w, is_prob=True)
    assert np.array_equal(got[1], want[0]) and np.array_equal(_bits(got[2]), _bits(want[1])) and np.array_equal(got[3], want[2])
    assert np.array_equal(got[4], want[3])


# ---- known answers --------------------------------------------------------------------------------------------------------------------------------
def test_the_step_edge_its_levels_and_its_tie():
    """values 4 4 4 3 1 0 0 0 of class 0 against 1 of class 1: p = 1 / (1 + exp(-3)), 1 / (1 + exp(-2)), 1 / 2, 1 / (1 + exp(-1))"""
    labels, conf, margin, second, _ = ref.reference(_step16())
    assert conf[0, 3, 6:14].tolist() == [243, 243, 243, 225, 128, 187, 187, 187]
    assert margin[0, 3, 10] == 0 and second[0, 3, 10] == 1 and labels[0, 3, 10] == 0          # the tie takes the first class
    assert margin[0, 3, 6:14].tolist() == [3, 3, 3, 2, 0, 1, 1, 1] and second[0, 3, 6:14].tolist() == [1, 1, 1, 1, 1, 0, 0, 0]


@pytest.mark.parametrize("case", ref.known_cases(), ids=ref.ident)
def test_known_answers_on_resampled_geometries(case):
    assert (case.h, case.w) != (case.out_h, case.out_w)
    labels, conf, margin, second, hist = ref.reference(case)
    if case.kind == "equal":            # identical planes give identical values: p = 1 / ncls
        assert (conf == {2: 128, 19: 13, 21: 12}[case.ncls]).all() and (margin == 0).all() and (labels == 0).all() and (second == 1).all()
    elif case.kind == "one100":         # p = 1 -> 256 -> 255; the blend of x + 100 is the blend of x, + 100 to within 1e-13: 100 in fp32
        w = ref.known_winner(case)
        assert (conf == 255).all() and (margin == 100).all() and (labels == w).all() and (second == (1 if w == 0 else 0)).all()
    else:                               # a two-way tie at the top: margin 0, the runner-up is the later index
        a, b = ref.known_tie(case)
        assert (margin == 0).all() and (labels == a).all() and (second == b).all()
        assert (conf == int(np.floor(256.0 / (2.0 + (case.ncls - 2) * np.exp(-3.0))))).all()
    assert int(hist.sum()) == case.n * case.h * case.w and (hist[:, conf[0, 0, 0]] == case.h * case.w).all()


def test_padding_never_reaches_the_source_size():
    s = np.full((1, 19, 32, 64), 50.0, np.float32)      # padding: all classes equal -> conf 13
    s[:, :, :29, :50] = 0
    s[:, 4, :29, :50] = 100                            # valid region: saturated on class 4
    labels, conf, margin, second, hist = image.confidence_interpolated_host(s, 29, 50, 58, 75)
    assert (labels == 4).all() and (conf == 255).all() and (margin == 100).all() and (second == 0).all() and int(hist[0, 255]) == 58 * 75


def test_probabilities_are_scaled_not_exponentiated():
    case = ref.prob_cases()[4]          # 45 x 83 from a 48 x 89 region
    assert (case.h, case.w) != (case.out_h, case.out_w)
    conf = ref.reference(case)[1]
    assert np.array_equal(conf, np.minimum(255.0, np.floor(256.0 * ref.values(case).max(axis=1))).astype(np.uint8))
    as_logits = image.confidence_interpolated_host(ref.scores(case), case.out_h, case.out_w, case.h, case.w)[1]
    assert not np.array_equal(conf, as_logits)


# ---- the guard: conditions, not measurements ----------------------------------------------------------------------------------------------------------
def test_guard_conditions_of_the_gpu_inputs():
    """(a) For every input of test_interp_conf_gpu.py, 256 * p is farther than 1e-9 from every integer at every pixel whose byte an exp could
    move: the blend is specified bit for bit, so only the device's exp can differ, by about an ulp per term -- some 3e-13 in 256 * p.
    (b) For every input but the exact ones, neither the two best nor the second and third best values of a pixel are closer than 1e-12 x the
    largest |score|.  Conditions, not tolerances: if a seed violates one, change the seed."""
    cases = ref.all_cases()
    assert len(cases) == len(ref.all_operator_cases()) + 3 + 4 + 2 + 1 + 3 + 12 + len(ref.dyadic_cases()) + 18
    worst_a, worst_b = None, None
    for case in cases:
        v, exact = ref.scaled_float64(case)
        dist = np.abs(v - np.rint(v))
        bad = (dist < ref.CONF_GUARD) & ~exact
        assert not bad.any(), (ref.ident(case), int(bad.sum()), v[bad][:4])
        if not exact.all() and (worst_a is None or dist[~exact].min() < worst_a[0]):
            worst_a = (float(dist[~exact].min()), ref.ident(case))
        if ref.exempt(case):
            continue
        first, third, top = ref.smallest_gaps(case)
        assert first >= ref.GUARD * top and third >= ref.GUARD * top, (ref.ident(case), first, third, top)
        if worst_b is None or min(first, third) / top < worst_b[0]:
            worst_b = (min(first, third) / top, ref.ident(case))
    print("(a) smallest distance %.3g in %s; (b) smallest relative gap %.3g in %s" % (worst_a + worst_b))


# ---- the mutant matrix ------------------------------------------------------------------------------------------------------------------------------------
def _differs(case, got, which=(0, 1, 2, 3)):
    """how many pixels of the outputs `which` (0 labels, 1 conf, 2 margin bits, 3 second) of a mutant differ from the specification's"""
    want = ref.reference(case)
    return sum(int(np.count_nonzero((_bits(got[i]) if i == 2 else got[i]) != (_bits(want[i]) if i == 2 else want[i]))) for i in which)


def test_the_harness_of_the_mutants_is_the_specification_when_nothing_is_mutated():
    for case in ref.near_tie_cases() + ref.dyadic_cases() + ref.known_cases()[:4] + [ref.small_case(*g, ncls=19, n=1, scale=1.0) for g in SMALL]:
        assert _differs(case, _finish(_values_with(case, *_spec_taps(case)))) == 0, ref.ident(case)
        if case.kind != "near":       # (the float coordinate form of the taps agrees on these inputs up to a last bit of a weight: labels, second)
            v = _values_with(case, _mutant_taps(case.h, case.out_h), _mutant_taps(case.w, case.out_w))
            assert _differs(case, _finish(v), which=(0, 3)) == 0, ref.ident(case)


def test_mutant_nearest_rule():
    """confidence_host: the kernel this one stands beside"""
    case = ref.small_case(*SMALL[5], ncls=19, n=1, scale=1.0)                            # 48 x 96 to 60 x 120
    conf, margin, second, hist = image.confidence_host(ref.scores(case), case.out_h, case.out_w, case.h, case.w)
    want = ref.reference(case)
    assert np.count_nonzero(conf != want[1]) > case.h * case.w // 2 and np.count_nonzero(_bits(margin) != _bits(want[2])) > case.h * case.w // 2
    assert np.count_nonzero(second != want[3]) > 0 and not np.array_equal(hist, want[4])


def test_mutant_softmax_before_the_interpolation():
    """the probabilities interpolated instead of the logits: another number wherever the taps disagree"""
    case = ref.small_case(*SMALL[5], ncls=19, n=1, scale=1.0)
    s = ref.scores(case)[:, :, :case.out_h, :case.out_w].astype(np.float64)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = image.confidence_interpolated_host((e / e.sum(axis=1, keepdims=True)).astype(np.float32), case.out_h, case.out_w, case.h, case.w, is_prob=True)
    assert np.count_nonzero(p[1] != ref.reference(case)[1]) > case.h * case.w // 2


def test_mutant_float32_blend():
    """random scores do not pin the precision of the blend; the near-tie cases do: labels and second flip"""
    for case in ref.near_tie_cases():
        got = _finish(_values_with(case, *_spec_taps(case), dtype=np.float32).astype(np.float64))
        assert _differs(case, got, which=(0,)) > 0 and _differs(case, got, which=(3,)) > 0, ref.ident(case)


def test_near_tie_cases_have_their_known_answer():
    for case in ref.near_tie_cases():
        labels, _, margin, second, _ = ref.reference(case)
        assert (labels[0] == 11).all() and (second[0] == 5).all() and (labels[1] == 5).all() and (second[1] == 11).all(), ref.ident(case)
        assert (margin > 0).all()


def test_mutant_margin_of_float32_values():
    """the float64 values rounded to fp32 before the subtraction: the near ties, an fp32 ulp apart, lose their margin or double it"""
    for case in ref.near_tie_cases():
        got = _finish(ref.values(case), margin_dtype=np.float32)
        assert _differs(case, got, which=(0, 1, 3)) == 0 and _differs(case, got, which=(2,)) > 0, ref.ident(case)


def test_mutant_taps_clamped_to_the_map_not_the_region():
    """23 x 150 from a 15 x 96 region of a 16 x 96 map: the last rows would blend with the padded row, whose class 0 is POISON"""
    for ncls in ref.NCLS:
        case = ref.small_case(*SMALL[9], ncls=ncls, n=1, scale=1.0)
        assert case.out_h < case.H and case.h > case.out_h
        v = _values_with(case, _mutant_taps(case.h, case.out_h, limit=case.H), _mutant_taps(case.w, case.out_w, limit=case.W), whole_map=True)
        assert _differs(case, _finish(v), which=(0,)) > 0 and _differs(case, _finish(v), which=(1,)) > 0, ref.ident(case)


def test_mutant_align_corners():
    case = ref.small_case(*SMALL[5], ncls=19, n=1, scale=1.0)
    v = _values_with(case, _mutant_taps(case.h, case.out_h, corners=True), _mutant_taps(case.w, case.out_w, corners=True))
    assert _differs(case, _finish(v), which=(1,)) > 0 and _differs(case, _finish(v), which=(2,)) > 0


def test_mutant_rows_and_columns_swapped():
    for case in [ref.small_case(*SMALL[1], ncls=19, n=1, scale=1.0), ref.small_case(*SMALL[7], ncls=19, n=1, scale=1.0), ref.multiblock_cases()[0]]:
        ty = _mutant_taps(case.h, case.out_h, ratio=(case.out_w, case.w), clamp=case.out_w)
        tx = _mutant_taps(case.w, case.out_w, ratio=(case.out_h, case.h), clamp=case.out_h)
        assert _differs(case, _finish(_values_with(case, ty, tx)), which=(1,)) > 0, ref.ident(case)


def test_mutant_last_maximum():
    case = _step16()
    got = _finish(ref.values(case), last=True)
    assert got[0][0, 3, 10] == 1 and got[3][0, 3, 10] == 0                                # the tied column: label and runner-up change places
    assert _differs(case, got, which=(0,)) == case.h and _differs(case, got, which=(3,)) == case.h and _differs(case, got, which=(1, 2)) == 0
    for case in [c for c in ref.dyadic_cases() if c.kind == "ints"] + [c for c in ref.known_cases() if c.kind in ("equal", "tie2")]:
        assert _differs(case, _finish(ref.values(case), last=True), which=(0, 3)) > 0, ref.ident(case)


def test_mutant_hist_at_map_resolution():
    """the levels of the map's pixels counted instead of the source's"""
    for case in (ref.small_case(*SMALL[5], ncls=19, n=1, scale=1.0), ref.small_case(*SMALL[2], ncls=19, n=1, scale=1.0)):
        at_map = image.confidence_host(ref.scores(case), case.out_h, case.out_w, case.out_h, case.out_w)[3]
        hist = ref.reference(case)[4]
        assert int(at_map.sum()) == case.out_h * case.out_w != case.h * case.w == int(hist.sum())
        assert not np.array_equal(at_map, hist)
