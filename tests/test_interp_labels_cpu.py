"""Labels from interpolated scores, host side: utils.image.labels_interpolated_host (the float64 specification csrc/scores_labels.hip restates)
against np.argmax, an integer restatement and torch's float64 bilinear interpolation; the GUARD condition that lets test_interp_labels_gpu.py
demand equality; and the mutant matrix: the case table of interp_ref.py tells the specification apart from each plausible wrong kernel."""
import numpy as np
import pytest

from accel_amd.utils import image

import interp_ref as ref
from test_frames_u8_gpu import SMALL


# ---- the specification against independent restatements ----------------------------------------------------------------------------------------
def test_taps_are_the_half_pixel_coordinate_clamped_to_the_region():
    for dst, src in [(16, 8), (32, 8), (4, 8), (45, 48), (83, 89), (100, 64), (720, 1024), (2160, 1024), (7, 1), (1, 7), (5, 5)]:
        i0, i1, f = image.interpolation_taps(dst, src)
        c = np.clip((np.arange(dst) + 0.5) * src / dst - 0.5, 0, src - 1)
        assert i0.min() >= 0 and i1.max() <= src - 1 and np.all((i1 == i0 + 1) | (i1 == src - 1))
        assert np.all((f >= 0) & (f < 1)) and np.allclose(i0 + f, c, rtol=0, atol=1e-9), (dst, src)
    i0, i1, f = image.interpolation_taps(5, 5)
    assert np.array_equal(i0, np.arange(5)) and not f.any()
    # the largest sizes of the C ABI stay below 2^31
    assert (2 * 32767 + 1) * 32768 < 2 ** 31 and 2 * 32768 * 32767 < 2 ** 31


@pytest.mark.parametrize("case", ref.crop_cases() + [ref.multiblock_cases()[1]] + [ref.small_case(*SMALL[0], ncls=k, n=3, scale=s) for k in ref.NCLS
                                                                                   for s in ref.SCALES], ids=ref.ident)
def test_identity_is_the_crop_of_the_argmax(case):
    assert (case.h, case.w) == (case.out_h, case.out_w)
    want = np.argmax(ref.scores(case), axis=1)[:, :case.h, :case.w].astype(np.uint8)
    assert np.array_equal(ref.reference(case), want)
    # which is what the nearest rule gives there
    assert np.array_equal(image.labels_to_source_host(np.argmax(ref.scores(case), axis=1).astype(np.uint8), case.out_h, case.out_w, case.h, case.w), want)


@pytest.mark.parametrize("case", ref.dyadic_cases(), ids=ref.ident)
def test_dyadic_cases_equal_the_integer_restatement(case):
    assert np.array_equal(ref.reference(case), ref.integer_labels(case))


def test_the_step_edge_and_its_tie():
    case = [c for c in ref.dyadic_cases() if c.kind == "step" and c.h == 16][0]
    v = ref.values(case)
    assert np.array_equal(v[0, 0, 3, 6:14], [4, 4, 4, 3, 1, 0, 0, 0]) and (v[0, 1] == 1).all()
    lab = ref.reference(case)
    assert v[0, 0, 3, 10] == v[0, 1, 3, 10] == 1 and lab[0, 3, 10] == 0          # the tie takes the first class
    assert (lab[0, :, :11] == 0).all() and (lab[0, :, 11:] == 1).all()


@pytest.mark.parametrize("rows,cols,target,max_size", SMALL)
def test_operator_cases_equal_the_argmax_of_torch_interpolate(rows, cols, target, max_size):
    import torch
    import torch.nn.functional as F
    for ncls in ref.NCLS:
        for n in (1, 3):
            for case in ref.operator_cases(rows, cols, target, max_size, ncls, n):
                s = torch.from_numpy(ref.scores(case)[:, :, :case.out_h, :case.out_w].astype(np.float64))
                v = F.interpolate(s, size=(case.h, case.w), mode="bilinear", align_corners=False).numpy()
                assert np.abs(v - ref.values(case)).max() <= 1e-12 * case.scale * 8, ref.ident(case)
                assert np.array_equal(np.argmax(v, axis=1).astype(np.uint8), ref.reference(case)), ref.ident(case)


def test_near_tie_cases_have_their_known_answer():
    for case in ref.near_tie_cases():
        lab = ref.reference(case)
        assert (case.h, case.w) != (case.out_h, case.out_w)
        assert (lab[0] == 11).all() and (lab[1] == 5).all(), ref.ident(case)


# ---- the guard: a condition, not a measurement ----------------------------------------------------------------------------------------------------
def _smallest_gap(case):
    v = np.sort(ref.values(case), axis=1)
    return float((v[:, -1] - v[:, -2]).min()), float(np.abs(ref.scores(case)[:, :, :case.out_h, :case.out_w]).max())


def test_guard_condition_of_the_gpu_inputs():
    """no pixel of a guarded case has its two best interpolated values within GUARD x the largest |score|: a summation order or an fma
    (1e-16 of the scale) cannot move a label, so the GPU tests demand equality"""
    cases = ref.guarded_cases()
    assert len(cases) == len(ref.all_operator_cases()) + 3 + 4 + 2 + 1 + 3
    worst = None
    for case in cases:
        gap, top = _smallest_gap(case)
        if worst is None or gap / top < worst[0]:
            worst = (gap / top, ref.ident(case))
        assert gap >= ref.GUARD * top, (ref.ident(case), gap, top)
    print("smallest relative gap %.3g in %s" % worst)


# ---- the mutant matrix -------------------------------------------------------------------------------------------------------------------------------
def _mutant_taps(dst, src, limit=None, corners=False, ratio=None, clamp=None):
    """interpolation_taps with a fault: limit (the taps are kept inside another size), corners (align_corners=True coordinates), ratio and
    clamp (the scale and the clamp of the other axis: (src, dst) of it and its src)"""
    limit = src if limit is None else limit
    i = np.arange(dst, dtype=np.float64)
    if corners:
        c = i * (src - 1) / max(dst - 1, 1)
    else:
        rs, rd = ratio or (src, dst)
        c = (i + 0.5) * rs / rd - 0.5
    c = np.clip(c, 0, (limit if clamp is None else min(clamp, limit)) - 1)
    i0 = np.floor(c).astype(np.int64)
    return i0, np.minimum(i0 + 1, limit - 1), c - i0


def _labels_with(case, ty, tx, dtype=np.float64, last=False, whole_map=False):
    """the specification's blend and scan over given taps, in `dtype`, with the first or the last maximum"""
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
    if last:
        return (case.ncls - 1 - np.argmax(v[:, ::-1], axis=1)).astype(np.uint8)
    return np.argmax(v, axis=1).astype(np.uint8)


def _spec_taps(case):
    return image.interpolation_taps(case.h, case.out_h), image.interpolation_taps(case.w, case.out_w)


def _differs(case, got):
    return int(np.count_nonzero(got != ref.reference(case)))


def test_the_harness_of_the_mutants_is_the_specification_when_nothing_is_mutated():
    for case in ref.near_tie_cases() + ref.dyadic_cases() + [ref.small_case(*g, ncls=19, n=1, scale=1.0) for g in SMALL]:
        assert _differs(case, _labels_with(case, *_spec_taps(case))) == 0, ref.ident(case)
        ty = _mutant_taps(case.h, case.out_h)
        tx = _mutant_taps(case.w, case.out_w)
        assert _differs(case, _labels_with(case, ty, tx)) == 0, ref.ident(case)           # the float coordinate form agrees on these inputs


def test_mutant_nearest_rule():
    case = ref.small_case(*SMALL[5], ncls=19, n=1, scale=1.0)                            # 48 x 96 to 60 x 120
    got = image.labels_to_source_host(np.argmax(ref.scores(case), axis=1).astype(np.uint8), case.out_h, case.out_w, case.h, case.w)
    assert _differs(case, got) > case.h * case.w // 2


def test_mutant_align_corners():
    case = ref.small_case(*SMALL[5], ncls=19, n=1, scale=1.0)
    got = _labels_with(case, _mutant_taps(case.h, case.out_h, corners=True), _mutant_taps(case.w, case.out_w, corners=True))
    assert _differs(case, got) > 0


def test_mutant_taps_clamped_to_the_map_not_the_region():
    """a tap can only stray where the map is scaled UP (the last half source pixel lies past the last map pixel's centre) next to padding:
    23 x 150 from a 15 x 96 region of a 16 x 96 map -- the last rows would blend with the padded row"""
    for ncls in ref.NCLS:
        case = ref.small_case(*SMALL[9], ncls=ncls, n=1, scale=1.0)
        assert case.out_h < case.H and case.h > case.out_h
        got = _labels_with(case, _mutant_taps(case.h, case.out_h, limit=case.H), _mutant_taps(case.w, case.out_w, limit=case.W), whole_map=True)
        assert _differs(case, got) > 0, ref.ident(case)


def test_mutant_float32_blend():
    """random scores do not pin the precision of the blend; the near-tie cases do"""
    for case in ref.near_tie_cases():
        got = _labels_with(case, *_spec_taps(case), dtype=np.float32)
        assert _differs(case, got) > 0, ref.ident(case)


def test_mutant_last_maximum():
    case = [c for c in ref.dyadic_cases() if c.kind == "step" and c.h == 16][0]
    got = _labels_with(case, *_spec_taps(case), last=True)
    assert got[0, 3, 10] == 1 and _differs(case, got) == case.h                          # the tied column of every row
    for case in [c for c in ref.dyadic_cases() if c.kind == "ints"]:
        assert _differs(case, _labels_with(case, *_spec_taps(case), last=True)) > 0, ref.ident(case)


def test_mutant_rows_and_columns_swapped():
    """the taps of a row computed with the sizes of the columns and the other way round (scale and clamp): the portrait geometries, where
    the rows past the region's width collapse, and the anisotropic multi-block case"""
    for case in [ref.small_case(*SMALL[1], ncls=19, n=1, scale=1.0), ref.small_case(*SMALL[7], ncls=19, n=1, scale=1.0), ref.multiblock_cases()[0]]:
        ty = _mutant_taps(case.h, case.out_h, ratio=(case.out_w, case.w), clamp=case.out_w)
        tx = _mutant_taps(case.w, case.out_w, ratio=(case.out_h, case.h), clamp=case.out_h)
        assert _differs(case, _labels_with(case, ty, tx)) > 0, ref.ident(case)


# ---- the demo's flag -------------------------------------------------------------------------------------------------------------------------------------
def test_demo_interpolate_needs_finish_on_gpu():
    from accel_amd import demo
    with pytest.raises(ValueError, match="--interpolate needs --finish-on-gpu"):
        demo.main(["--interpolate"])
