"""The fp16x2 form octave by octave below the one number that sets its scale.

Every operand of the form is hi + lo, two half terms of the value times a power of two taken from the largest |pixel| of the WHOLE input
tensor (csrc/range.h) or the largest |weight| of the output channel (accel_hip.cpp pack_h2r), so what a value keeps depends on how far
below that maximum it lies.  The other fp16x2 tests divide the largest error by the largest |output| of the whole tensor: they see the
top octaves only.  Here every magnitude is uniform[1, 2) * random sign * 2^-J, a band exactly one octave wide, and every band is judged
by itself:

  pixel ladder by image    8 images in one range slot, image n at octave -J[n], J = (0, 4, 8, 11, 14, 17, 20, 24); one anchor element of
                           image 0 is the tensor's maximum, once 2.0 (the bottom of the scale's window [2^13, 2^14)) and once the float
                           below 4.0 (its top): the same bound plan, the same scale, the bands one octave further below the maximum
  pixel ladder in an image row y of ONE image at octave -J[y] (1x1 readers): one hot pixel decides the scale of everything else
  weight ladder            8 groups of input channels, the weights of group g at octave -J[g] in every output row, image g non-zero only
                           in group g, all pixels of one magnitude (the stem has 3 input channels: no weight ladder for it)

Per band b, E_b(y) = max over the band's outputs of |y - ref| / (|w| conv |x|): ref the float64 convolution of the fp32 inputs, the
denominator the float64 convolution of the absolute values (no cancellation flatters or hurts a band; no denominator is zero).
  1. direct readers (b3r, halo, stem): max |y - model| / (|w| conv |x|) <= A, model = tests/h2_model.py with the scale the plan reports;
     only fp32 accumulation separates the two
  2. E_b(kernel) <= E_b(model) + A; the Winograd readers against 3 x the direct model at the quarter scale s / 4 they split V at
  3. bands wholly within 14 octaves of the maximum: E_b(kernel) <= 2^-22 + A (the "22-23 bits" of range.h, stated directly)
  4. the same plan in the bf16x3 form (exact operands at every octave, the same fp32 accumulation, another code path): E_b <= A
A, the accumulation allowance per sum|a||b|: see the constants below.  A failure of 1 is named by the curve it matches: the model with
half subnormals flushed (what a conversion or a matrix unit that flushed them would leave) or neither.

Measured on an MI355X: the direct readers are the model to within 1.24e-7 in every band down to octave -24 -- the loaders' conversion
and the A/B inputs of v_mfma_f32_32x32x16_f16 both keep half subnormals.
What these tests found: with the largest |U| of a channel in [2^14, 2^15), like the direct planes, the Winograd geometries missed
assertion 2 of test_weight_ladder at octaves -20 and -24 (geometry 41: 1.38e-6 > 3 x 2.68e-7 + A and 1.86e-5 > 3 x 4.65e-6 + A; 42 and
43 alike) -- below 2^-17 of the channel's largest the error of a weight term is the absolute 2^-25 of the scaled value, paid at 16
positions against |V| <= 4 max|x| where the direct form pays it at 9 taps against |x|.  conv_wino_b3_pack_h2 now puts the largest |U|
into the last octave of the half range, [2^15, 65504]: 7.6e-7 and 1.36e-5 for geometry 41 (bars 9.95e-7 and 1.41e-5, the closest
case: 4 % under), 42 and 43 at 0.63 to 0.69 of their bars."""
import numpy as np
import pytest

import h2_model as h2
from accel_amd import runtime
from plan_helpers import Builder, conv64

pytestmark = pytest.mark.gpu

J = (0, 4, 8, 11, 14, 17, 20, 24)
TOP_LO, TOP_HI = np.float32(2.0), np.nextafter(np.float32(4.0), np.float32(0))
WINO = (41, 42, 43)

# A: the fp32 accumulation noise of the matrix cores per sum|a||b|, K <= 1152: 2 x the largest per-band error of the bf16x3 form
# (assertion 4) over every case of this file, measured on an MI355X -- b3r 1.55e-7 (geometry 76, 1x1, K = 128), the halo layers 1.47e-7
# (on geometry 76: the halo geometry has no bf16x3 form), stem 1.34e-7, Winograd 9.4e-8 (per octave: DESIGN.md 5).  2x: three products
# per term instead of six, another order of summation.  The measurement agrees with the 1.5e-7 * sum|a||b| of an fp32 product chain of
# K <= 1024; an A above 5e-7 would be a finding of its own.  (Measured kernel - model, assertion 1: at most 1.24e-7.)
A = {"b3r": 3.1e-7, "halo": 2.9e-7, "stem": 2.7e-7, "wino": 1.9e-7}


def family(tile):
    return "wino" if tile in WINO else "halo" if tile == 78 else "stem" if tile == 51 else "b3r"


def band(rng, shape, j):
    """uniform[1, 2) * random sign * 2^-j, exact in fp32"""
    m = 1.0 + rng.integers(0, 2 ** 23, shape) * 2.0 ** -23
    return (m * np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 2.0 ** -j).astype(np.float32)


def deconv64(x, w):
    """float64 4x4 / stride 2 / pad 1 deconvolution (NCHW; w: (Cin, Cout, 4, 4)); passes float64 arguments through"""
    N, C, h, w_ = x.shape
    out = np.zeros((N, w.shape[1], 2 * h + 2, 2 * w_ + 2))
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky:ky + 2 * h:2, kx:kx + 2 * w_:2] += np.einsum('ck,nchw->nkhw', np.asarray(w[:, :, ky, kx], np.float64), x)
    return out[:, :, 1:1 + 2 * h, 1:1 + 2 * w_]


class Case(object):
    def __init__(self, tile, cin, cout, H, W, k=1, s=1, p=0, d=1, deconv=False):
        self.tile, self.cin, self.cout, self.H, self.W, self.k, self.s, self.p, self.d, self.deconv = tile, cin, cout, H, W, k, s, p, d, deconv

    def id(self):
        return "t%d-%dx%d-%dx%d-k%ds%dd%d%s" % (self.tile, self.cin, self.cout, self.H, self.W, self.k, self.s, self.d, "-deconv2x" if self.deconv else "")

    def f64(self, x, w):
        return deconv64(x, w) if self.deconv else conv64(x, w, self.s, self.p, self.d)

    def out_hw(self):
        if self.deconv:
            return 2 * self.H, 2 * self.W
        return ((self.H + 2 * self.p - self.d * (self.k - 1) - 1) // self.s + 1, (self.W + 2 * self.p - self.d * (self.k - 1) - 1) // self.s + 1)


def run_form(ctx, monkeypatch, form, case, N, w, feeds):
    """one-convolution plan (geometry forced, no K split, no bias, no activation) bound once, run on every input of `feeds`:
    [(output, pixel scale)] -- the scale None in the bf16x3 form, which has no range slots"""
    monkeypatch.setenv("ACCEL_SPLIT", form)
    tile = case.tile
    if form == "b3" and tile == 78:
        tile = 76          # the halo geometry exists in the fp16x2 form only: the implicit-GEMM kernel of the same layer measures A
    b = Builder(N)
    x = b.inp("x", case.cin, case.H, case.W, yr=7)
    Ho, Wo = case.out_hw()
    y = b.buf(case.cout, Ho, Wo)
    if case.deconv:
        b.params["c_w"] = w
        b.lines.append("conv name=c in=%s out=%s w=c_w act=0 cin=%d cout=%d mode=deconv2x tile=%d nosplit=1 xr=7" % (x.ref(), y.ref(), case.cin, case.cout, tile))
    else:
        b.conv("c", x, y, w, tile, case.k, case.s, case.p, case.d, act=0, xr=7, extra="nosplit=1")
    b.out("y", y)
    m = runtime.Model(ctx)
    try:
        m.set_params(b.params)
        plan = m.add_plan("p", b.text())
        plan.finalize()
        op = [o for o in plan.ops() if o["kind"] == "conv"]
        assert len(op) == 1 and op[0]["tile"] == tile and op[0]["mode"] == (3 if form == "h2" else 0) and op[0]["ksplit"] <= 1 and not op[0]["narrow"], op
        got = []
        for xin in feeds:
            m.write("x", np.ascontiguousarray(xin, np.float32))
            plan.run()
            out = m.read("y", b.outputs["y"]).copy()
            s = None
            if form == "h2":
                s, src = plan.ranges()["c"]
                top = float(np.abs(xin).max())
                assert src == 2, src                                        # measured: import_nchw has no range epilogue
                assert 2.0 ** 13 <= s * top < 2.0 ** 14 and s == h2.range_scale(h2.float_bits(top)), (s, top)
            else:
                assert plan.ranges() == {}
            got.append((out, s))
        return got
    finally:
        m.close()


def check(ctx, monkeypatch, case, label, N, w, feeds, bands):
    """feeds: [(tag, x, within14)], all run on ONE bound plan per form; within14: [bool] per band; bands: [index into the
    (N, Cout, Ho, Wo) output] per band.  Prints one line per input and quantity, then asserts 1-4 for every band."""
    fam = family(case.tile)
    a = A[fam]
    assert a <= 5e-7
    cout_axis = 1 if case.deconv else 0
    h2_runs = run_form(ctx, monkeypatch, "h2", case, N, w, [f[1] for f in feeds])
    b3_runs = run_form(ctx, monkeypatch, "b3", case, N, w, [f[1] for f in feeds])
    fails = []
    for (tag, x, within14), (y, s), (yb, _) in zip(feeds, h2_runs, b3_runs):
        ref = case.f64(x.astype(np.float64), w.astype(np.float64))
        den = case.f64(np.abs(x).astype(np.float64), np.abs(w).astype(np.float64))
        assert np.isfinite(y).all() and np.isfinite(yb).all()
        assert (den > 0).all()                                             # no output is excluded
        sm = s / 4 if fam == "wino" else s
        model = h2.conv(x, w, sm, case.f64, cout_axis)
        flushed = h2.conv(x, w, sm, case.f64, cout_axis, flush_subnormals=True)
        E = lambda arr, other, ix: float((np.abs(arr[ix].astype(np.float64) - other[ix]) / den[ix]).max())
        rows = {"gpu": [], "model": [], "b3": [], "gpu-model": [], "gpu-flushed": []}
        for ix in bands:
            rows["gpu"].append(E(y, ref, ix)); rows["model"].append(E(model, ref, ix)); rows["b3"].append(E(yb, ref, ix))
            rows["gpu-model"].append(E(y, model, ix)); rows["gpu-flushed"].append(E(y, flushed, ix))
        for key in ("gpu", "model", "b3", "gpu-model"):
            print("%s %s %s scale 2^%d %-9s %s" % (case.id(), label, tag, int(np.log2(s)), key, " ".join("J%d:%.2e" % (j, v) for j, v in zip(J, rows[key]))))
        for i, j in enumerate(J):
            g, mo, b3, gm, gf = (rows[key][i] for key in ("gpu", "model", "b3", "gpu-model", "gpu-flushed"))
            where = "%s %s %s J=%d" % (case.id(), label, tag, j)
            if fam != "wino" and gm > a:
                fails.append("%s: 1. kernel - model %.3g > A = %.3g (kernel - model with half subnormals flushed: %.3g -- %s)" % (
                    where, gm, a, gf, "the device matches the FLUSHED curve" if gf <= a else "neither curve"))
            bar = 3 * mo + a if fam == "wino" else mo + a
            if g > bar:
                fails.append("%s: 2. E(kernel) %.3g > %.3g (E(model) %.3g, A %.3g)" % (where, g, bar, mo, a))
            if within14[i] and g > 2.0 ** -22 + a:
                fails.append("%s: 3. E(kernel) %.3g > 2^-22 + A" % (where, g))
            if b3 > a:
                fails.append("%s: 4. bf16x3 form %.3g > A = %.3g" % (where, b3, a))
    assert not fails, "\n".join(fails)


# ---- pixel ladder by image ----------------------------------------------------------------------------------------------------------
# 8 images of 5 x 7 (M = 280: ragged against the 128-row tile, every tile straddles images); Cout 40 (ragged against every channel tile)
BY_IMAGE = [Case(t, 128, 40, 5, 7) for t in (76, 77, 79, 80, 81)] + [Case(t, 64, 40, 5, 7, 3, 1, 1, 1) for t in (76, 77, 79, 80, 81)] + [
    Case(76, 64, 40, 9, 11, 3, 2, 2, 2),                   # 3x3 / stride 2 / dilation 2
    Case(77, 40, 40, 5, 7, 3, 1, 1, 1),                    # Cin % 32 != 0: the kernel's general (non-FAST) loader
    Case(81, 72, 40, 5, 7, 1, 1, 0, 1),                    # ... and for a 1x1
    Case(78, 64, 40, 5, 7, 3, 1, 1, 1), Case(78, 64, 40, 5, 7, 3, 1, 2, 2),
    Case(51, 3, 64, 18, 26, 7, 2, 3, 1),
] + [Case(t, 64, 40, 6, 10, 3, 1, 1, 1) for t in WINO]


def ladder_by_image(rng, case, top):
    x = np.concatenate([band(rng, (1, case.cin, case.H, case.W), j) for j in J])
    x[0, case.cin - 1, case.H // 2, case.W // 2] = top
    a = np.abs(x)
    assert a.max() == top and (a == top).sum() == 1
    return x


@pytest.mark.parametrize("case", BY_IMAGE, ids=Case.id)
def test_pixel_ladder_by_image(ctx, monkeypatch, case):
    rng = np.random.default_rng(case.tile * 100 + case.cin + case.k)
    w = band(rng, (case.cout, case.cin, case.k, case.k), 0)
    x = ladder_by_image(rng, case, TOP_LO)
    x2 = x.copy(); x2[np.abs(x2) == TOP_LO] = TOP_HI
    assert np.abs(x2).max() == TOP_HI
    for top, xx in ((TOP_LO, x), (TOP_HI, x2)):      # where each band lies below the maximum: from the values
        for n, j in enumerate(J):
            lo, hi = np.abs(xx[n]).min(), np.abs(np.where(np.abs(xx[n]) == top, 0, xx[n])).max()
            assert 2.0 ** -j <= lo and hi < 2.0 ** (1 - j)
    within = lambda xx: [bool(np.abs(xx[n]).min() >= np.abs(xx).max() * 2.0 ** -14) for n in range(len(J))]
    assert within(x) == [j <= 13 for j in J] and within(x2) == [j <= 12 for j in J]
    bands = [np.s_[n] for n in range(len(J))]
    check(ctx, monkeypatch, case, "pixels/image", len(J), w, [("top=2.0", x, within(x)), ("top<4.0", x2, within(x2))], bands)


def test_one_bound_plan_serves_both_ends_of_the_window(ctx, monkeypatch):
    """the two anchors through ONE bound plan, both orders: the same scale, and every run a function of its own input alone"""
    case = Case(76, 128, 40, 5, 7)
    rng = np.random.default_rng(5)
    w = band(rng, (case.cout, case.cin, 1, 1), 0)
    x = ladder_by_image(rng, case, TOP_LO)
    x2 = x.copy(); x2[np.abs(x2) == TOP_LO] = TOP_HI
    (y1, s1), (y2, s2), (y3, s3) = run_form(ctx, monkeypatch, "h2", case, len(J), w, [x, x2, x])
    assert s1 == s2 == s3 == 2.0 ** 12
    assert np.array_equal(y1, y3) and np.array_equal(y1[1:], y2[1:])      # images 1..7 hold the same values at the same scale


# ---- pixel ladder inside one image -----------------------------------------------------------------------------------------------------
IN_IMAGE = [Case(t, 128, 40, 8, 37) for t in (76, 77, 79, 80, 81)] + [Case(81, 72, 40, 8, 37)]


@pytest.mark.parametrize("case", IN_IMAGE, ids=Case.id)
def test_pixel_ladder_inside_one_image(ctx, monkeypatch, case):
    rng = np.random.default_rng(case.tile * 100 + case.cin + 1)
    w = band(rng, (case.cout, case.cin, 1, 1), 0)
    x = np.concatenate([band(rng, (1, case.cin, 1, case.W), j) for j in J], axis=2)       # M = 296: ragged, rows of 37 pixels
    x[0, 3, 0, case.W - 1] = TOP_LO
    x2 = x.copy(); x2[0, 3, 0, case.W - 1] = TOP_HI
    bands = [np.s_[:, :, r] for r in range(len(J))]
    feeds = []
    for tag, xx, lim in (("top=2.0", x, 13), ("top<4.0", x2, 12)):
        assert (np.abs(xx) == np.abs(xx).max()).sum() == 1
        within = [bool(np.abs(xx[:, :, r]).min() >= np.abs(xx).max() * 2.0 ** -14) for r in range(len(J))]
        assert within == [j <= lim for j in J]
        feeds.append((tag, xx, within))
    check(ctx, monkeypatch, case, "pixels/row", 1, w, feeds, bands)


# ---- weight ladder -----------------------------------------------------------------------------------------------------------------------
# 8 groups of 32 input channels (1x1, deconvolution) or of 16 (3x3: K = 1152)
WEIGHTS = [Case(t, 256, 40, 5, 7) for t in (76, 77, 79, 80, 81)] + [Case(t, 128, 40, 5, 7, 3, 1, 1, 1) for t in (76, 81)] + [
    Case(78, 128, 40, 5, 7, 3, 1, 1, 1)] + [Case(t, 128, 40, 6, 10, 3, 1, 1, 1) for t in WINO] + [
    Case(76, 256, 40, 5, 7, 4, deconv=True)]               # q is taken over all four parity classes of the deconvolution


@pytest.mark.parametrize("case", WEIGHTS, ids=Case.id)
def test_weight_ladder(ctx, monkeypatch, case):
    rng = np.random.default_rng(case.tile * 100 + case.cin + 2 + case.deconv)
    G = len(J)
    g = case.cin // G
    wshape = (case.cin, case.cout, 4, 4) if case.deconv else (case.cout, case.cin, case.k, case.k)
    w = np.zeros(wshape, np.float32)
    x = np.zeros((G, case.cin, case.H, case.W), np.float32)
    for i, j in enumerate(J):
        if case.deconv:
            w[i * g:(i + 1) * g] = band(rng, (g,) + wshape[1:], j)
        else:
            w[:, i * g:(i + 1) * g] = band(rng, (case.cout, g, case.k, case.k), j)
        x[i, i * g:(i + 1) * g] = band(rng, (g, case.H, case.W), 0)
    rows = np.abs(np.moveaxis(w, 1 if case.deconv else 0, 0).reshape(case.cout, G, -1))      # [row][group][...]
    top = rows.max(axis=(1, 2))
    assert (1.0 <= top).all() and (top < 2.0).all()
    within = [bool((rows[:, i].min(axis=1) >= top * 2.0 ** -14).all()) for i in range(G)]
    assert within == [jj <= 13 for jj in J]
    check(ctx, monkeypatch, case, "weights", G, w, [("pixels-in-[1,2)", x, within)], [np.s_[n] for n in range(G)])
