"""half_ref.py against the oracle, and its case table against the faults it is there to catch.

 * every exact case is a fair bit-for-bit comparison: sum |x||w| + |res| + |bias| < 2^24 at every output (all fp32 partial sums exact),
   at least 10 % of its outputs are genuinely rounded by the store to half, at least 5 % are exact ties, none overflows (but where the
   case is about that) and the subnormal ladder has outputs on both sides of 2^-14;
 * the expected values are what the oracle gives: oracle.ops.conv2d / deconv2d on the same operands, the epilogue in numpy fp32, the
   store rounded by numpy (exact cases: the same bits; bounded cases: inside the bound / the interval the GPU test asserts);
 * the table covers what it says: ten forms on six tiles, the shapes, the Cout edges, split K, column GEMM, deconvolution;
 * a matrix of mutants -- truncation, ties away from zero, rounding before the activation / before the residual, a half residual
   read as fp32, channel pair and row pair swapped, a half step behind the end of K that is not zero, tap offsets for 4-byte elements,
   deconvolution parity classes permuted, pad channels copied from the residual -- each of which must change the expected bits of at
   least one case of every family it applies to (and leave the interval of a bounded case where it moves values at all)."""
import collections

import numpy as np
import pytest

import conv_ref as R
import half_ref as HR
from oracle import ops as O
from test_conv_ref_cpu import conv32

IDS = lambda c: c.id


def _unique(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


VALUES = lambda c: (c.data_key, c.act)      # cases with the same expected VALUES (tile and storage aside)


def test_the_table_covers_what_it_says():
    ids = [c.id for c in HR.CASES]
    assert len(set(ids)) == len(ids)
    assert len(HR.FORMS) == 10 and ("f", "n", "f") not in HR.FORMS and ("f", "f", "f") not in HR.FORMS
    fam = collections.defaultdict(list)
    for c in HR.CASES:
        fam[c.fam].append(c)
    assert {(c.tile, c.form) for c in fam["forms"]} == {(t, f) for t in HR.TILES for f in HR.FORMS}
    assert {(c.tile, c.form) for c in fam["bounded"]} == {(t, f) for t in (84, 89) for f in HR.FORMS}
    for c in fam["forms"]:      # M odd and ragged for the 128- and 256-pixel tiles, 18 half steps: no multiple of KSUB = 4
        assert c.case.N * c.case.Ho * c.case.Wo == 741 and R.k_pad(c.case) // 16 == 18 and c.Cout == (64 if c.tile == 88 else 136)
    assert {c.act for c in fam["forms"] if c.yh} == {0, 1, 2}
    for name, _ in HR.GEOMETRY:
        cs = [c for c in fam["geometry"] if c.name == name]
        assert [c.tile for c in cs] == [84, 88 if cs[0].Cout <= 64 else 83, None] and all(c.xh for c in cs[:2])
    assert all(c.case.Cin % 16 == 0 for c in HR.CASES)
    g = {c.name: c.case for c in fam["geometry"]}
    assert g["k1cin16"].N * g["k1cin16"].Ho * g["k1cin16"].Wo == 128 and R.k_pad(g["k1cin16"]) == 32
    assert g["k3cin16"].K == 144 and R.k_pad(g["k3cin16"]) == 160 and g["d2"].N * g["d2"].Ho * g["d2"].Wo == 513
    assert g["m257"].N * g["m257"].Ho * g["m257"].Wo == 257 and R.k_pad(g["k1cin48s2"]) == 64
    assert {c.Cout for c in fam["cout"]} == {8, 18, 129, 260} and {c.tile for c in fam["cout"]} == {82, 84, 88}
    assert {c.tile for c in fam["splitk"]} == {82, 84, 88, None} and all(c.case.ksplit and (c.yh or c.res == "h") for c in fam["splitk"])
    assert {c.form for c in fam["splitk"] if c.name == "deep"} == set(HR.HALF_OUT_OR_RES)
    assert {(c.yh, c.kind) for c in fam["cols"] + fam["bounded-cols"]} == {(y, k) for y in (True, False) for k in ("exact", "bounded")}
    assert {(c.case.odd, c.yh) for c in fam["deconv"]} == {(o, y) for o in (True, False) for y in (True, False)}
    assert any(c.case.ksplit and c.case.Cin == 64 for c in fam["deconv"])
    assert {c.special for c in fam["special"]} == {"overflow", "subnormal"}


@pytest.mark.parametrize("hc", _unique(HR.EXACT, VALUES), ids=IDS)
def test_exact_cases_are_fair_and_really_round(hc):
    o, ref = HR.operands(hc), HR.reference(hc)
    unit = 2.0 ** -24 if hc.special == "subnormal" else 1.0
    # 1. every partial sum of the kernel is an integer (of `unit`) below 2^24: exact in fp32 in any order
    total = ref.A + np.abs(ref.res) + np.abs(ref.shift)
    assert total.max() < 2.0 ** 24 * unit, total.max()
    for a in (o["x"], o["w"], o["res"], o["bias"]):
        assert np.array_equal(a, np.round(a / unit) * unit) or a is o["w"] and np.array_equal(a, np.round(a))
    assert HR.is_half_exact(o["x"]).all() and HR.is_half_exact(o["w"]).all() and HR.is_half_exact(o["res"]).all()
    assert np.abs(o["res"]).max() <= 2048 * unit and (np.abs(o["bias"]) <= 2048 * unit).sum() >= hc.Cout - 3
    # 2., 3. the store to half is a real rounding, ties among them
    rounded, ties = float((~HR.is_half_exact(ref.y)).mean()), float(HR.is_tie(ref.y).mean())
    print("%s: %.1f %% rounded, %.1f %% ties" % (hc.id, 100 * rounded, 100 * ties))
    assert rounded >= 0.10 and ties >= 0.05, (rounded, ties)
    # 4. overflow where it is meant only: there on channels that hold finite values as well
    inf = np.isinf(HR.rtne(ref.y))
    if hc.special == "overflow":
        ch = inf.any(axis=(0, 2, 3))
        assert ch.sum() == 3 and all(0.05 < inf[:, c].mean() < 0.95 for c in np.flatnonzero(ch))
        assert (ref.y[inf] >= 65520).all()
    else:
        assert not inf.any()
    if hc.special == "subnormal":
        assert (np.abs(o["x"]) < 2.0 ** -14).all() and np.abs(o["x"]).max() == 64 * 2.0 ** -24
        a = np.abs(ref.y[ref.y != 0])
        assert 0.1 < (a < 2.0 ** -14).mean() < 0.9, "outputs on both sides of the smallest normal half"


def epilogue32(hc, conv):
    """scale / shift / residual / activation in numpy fp32, as the kernels evaluate them"""
    o = HR.operands(hc)
    scale, shift, _, _ = R.epilogue_constants(hc.case, o)
    v = conv * scale[None, :, None, None] + shift[None, :, None, None]
    if hc.res != "n":
        v = v + o["res"]
    assert v.dtype == np.float32
    return np.maximum(v, np.float32(0)) if hc.act == 1 else np.where(v > 0, v, v * np.float32(hc.slope)) if hc.act == 2 else v


@pytest.mark.parametrize("hc", _unique(HR.EXACT, lambda c: (VALUES(c), c.yh)), ids=IDS)
def test_expected_bits_are_the_oracles(hc):
    """the oracle's fp32 convolution of the same operands, its fp32 epilogue, numpy's rounding to half: the same bits"""
    o = HR.operands(hc)
    y = epilogue32(hc, conv32(hc.case, o["x"], o["w"]))
    with np.errstate(over="ignore"):      # (the overflow cases: numpy rounds to infinity, and says so)
        got = HR.nhwc(y).astype(np.float16).view(np.uint16) if hc.yh else HR.nhwc(y).view(np.uint32)
    want = HR.expected(hc)
    assert np.array_equal(got, want[..., :hc.Cout]) and not want[..., hc.Cout:].any()


@pytest.mark.parametrize("hc", _unique(HR.BOUNDED, lambda c: (VALUES(c), c.yh)), ids=IDS)
def test_an_fp32_evaluation_of_a_bounded_case_meets_its_check(hc):
    o, ref = HR.operands(hc), HR.reference(hc)
    assert HR.is_half_exact(o["x"]).all() and HR.is_half_exact(o["res"]).all() and not HR.is_half_exact(o["w"]).all()
    y = epilogue32(hc, conv32(hc.case, o["x"], HR.half(o["w"])))
    ratio = float((np.abs(y - ref.y) / ref.bound).max())
    print("%s: fp32 evaluation at %.3f of the bound" % (hc.id, ratio))
    assert ratio <= 1.0
    if hc.yh:
        lo, hi = HR.interval(hc)
        h = HR.nhwc(y).astype(np.float16)
        assert ((lo <= h) & (h <= hi)).all()


def test_roundings():
    v = np.array([2049.0, 2051.0, -2049.0, 2050.0, 2049.5, 65519.0, 65520.0, 70000.0, 3 * 2.0 ** -25, -2.0 ** -25, 2.0 ** -26, 1025.5 * 2.0 ** -24])
    assert HR.rtne(v).tolist() == [2048.0, 2052.0, -2048.0, 2050.0, 2050.0, 65504.0, np.inf, np.inf, 2.0 ** -23, -0.0, 0.0, 1026 * 2.0 ** -24]
    assert HR.trunc(v).tolist() == [2048.0, 2050.0, -2048.0, 2050.0, 2048.0, 65504.0, 65504.0, 65504.0, 2.0 ** -24, -0.0, 0.0, 1025 * 2.0 ** -24]
    assert HR.ties_away(v).tolist() == [2050.0, 2052.0, -2050.0, 2050.0, 2050.0, 65504.0, np.inf, np.inf, 2.0 ** -23, -2.0 ** -24, 0.0, 1026 * 2.0 ** -24]
    assert HR.is_tie(v).tolist() == [True, True, True, False, False, False, False, False, True, True, False, True]
    assert np.signbit(HR.rtne(np.array([-2.0 ** -26])))[0] and HR.rtne(np.array([HR.NEG_ZERO_BIAS])).view(np.uint16)[0] == 0x8000


def test_the_producers_buffers():
    """what the identity producers leave: the view's values, its pads zero (-0.0 in a residual), a fill whose neighbours differ"""
    for hc in HR.CASES:
        for which, (Cs, c0, C, H, W) in HR.layout(hc).items():
            half_view = {"x": hc.xh, "y": hc.yh, "r": hc.res == "h"}[which]
            assert c0 % (8 if half_view else 4) == 0 and (c0 > 0 or hc.case.mode == "cols") and c0 + HR.r4(C) <= Cs
            if not half_view:
                continue
            assert Cs % 8 == 0
            canvas, bias = HR.half_buffer(hc, which)
            assert canvas.shape == (hc.case.N + 1, H, W, HR.r16(Cs)) and HR.is_half_exact(canvas).all()
            bits = HR.half_buffer_bits(hc, which)
            if which == "y":
                f = bits.view(np.float16).astype(np.float64)
                assert f.min() >= 1 and all((np.diff(f, axis=a) != 0).all() for a in range(4))
            else:
                assert np.array_equal(bits[:-1, :, :, c0:c0 + C].view(np.float16), HR.nhwc(HR.operands(hc)["x" if which == "x" else "res"]).astype(np.float16))
                assert (bits[:-1, :, :, c0 + C:c0 + HR.r4(C)] == (0x8000 if which == "r" else 0)).all()
                pc, pb = HR.half_buffer(hc, which, poison=True)
                assert np.isnan(pc[-1]).all() and np.isfinite(pc[:-1]).all()
                assert np.isnan(pb[:c0]).all() and np.isnan(pb[c0 + HR.r4(C):]).all() and np.isfinite(pb[c0:c0 + HR.r4(C)]).all()
    strides = {tuple(HR.layout(hc)[w][0] for w in ("x", "y", "r")) for hc in HR.CASES if hc.form == ("h", "h", "h") and hc.case.mode == "conv"}
    assert all(len(set(s)) == 3 for s in strides)


@pytest.mark.parametrize("name", HR.MUTANTS)
def test_every_mutant_shows_in_every_family_it_applies_to(name):
    hit, applied = collections.defaultdict(int), collections.defaultdict(int)
    seen = {}
    for hc in HR.EXACT:
        if not HR.applies(hc, name):
            continue
        key = (VALUES(hc), hc.form, hc.tile if name == "ksub_tail" else 0)
        if key not in seen:
            seen[key] = not np.array_equal(HR.mutant(hc, name), HR.expected(hc))
        applied[hc.fam] += 1
        hit[hc.fam] += seen[key]
    print(name, {f: "%d / %d" % (hit[f], applied[f]) for f in sorted(applied)})
    assert applied, "the mutant applies to no case"
    for fam in applied:
        assert hit[fam] >= 1, "no %s case tells %s from the kernel" % (fam, name)
    want = {"deconv_parity": {"deconv"}, "ksub_tail": {"forms", "geometry", "cols", "special"}, "pad_from_res": {"cout", "splitk"}, "round_before_act": {"special"},
            "tap_esize4": {"forms", "geometry", "cout", "splitk", "cols", "special"}}.get(name, {"forms", "geometry", "cout", "splitk", "special"})
    assert set(applied) >= want, (name, sorted(applied))


@pytest.mark.parametrize("name", ["trunc", "chan_pair", "row_pair", "res_as_fp32", "tap_esize4"])
def test_value_moving_mutants_leave_the_interval_of_the_bounded_cases(name):
    """the interval check of a half output is no weaker than it looks: a swapped pair, a residual read as fp32, wrong taps put elements
    outside [h(ref - b), h(ref + b)]; truncation does wherever the reference is not within b of a half value from above.  (Under a
    leaky activation the negative outputs are small, the absolute bound spans several half values there and the roundings show in
    few elements: those faults are the exact cases' to catch.)"""
    n = 0
    for hc in _unique(HR.BOUNDED, lambda c: (VALUES(c), c.form)):
        if not (hc.yh and HR.applies(hc, name)):
            continue
        lo, hi = HR.interval(hc)
        m = HR.mutant(hc, name)[..., :hc.Cout].view(np.float16)
        with np.errstate(invalid="ignore"):
            out = ~((lo <= m) & (m <= hi))
        assert out.mean() > (0.05 if name == "trunc" else 0.3), (hc.id, name, out.mean())
        n += 1
    assert n >= 2
