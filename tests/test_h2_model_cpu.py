"""The arithmetic behind the fp16x2 form of the fp32 layers (kernels.h ConvParams::wh2r, csrc/range.h, accel_hip.cpp pack_h2r), restated
in numpy (tests/h2_model.py): every operand as hi + lo, two half terms of the value times a power of two taken from ONE number per
tensor (the largest |pixel|) or per output channel (the largest |weight|), three of the four products kept.  What the form keeps of a
value therefore depends on how far below that one maximum the value lies: the figures per octave asserted here are the ones
range.h, kernels.h, pack_h2r and DESIGN.md 5 quote.  (The GPU side of the claim is tests/test_h2_octaves_gpu.py; the counterpart for
the bf16x3 form is tests/test_bf16x3_cpu.py.)"""
import numpy as np
import pytest

import h2_model as h2

OCTAVES = (0, 4, 8, 10, 12, 14, 15, 16, 17, 20, 24)


def band(rng, n, octave, top):
    """n values of uniform[1, 2) * random sign * top * 2^-octave: one octave wide, `octave` octaves below `top`"""
    return (rng.uniform(1.0, 2.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0) * top * 2.0 ** -octave).astype(np.float32)


def split_curve(top, flush, seed=1, n=200000):
    """largest relative error of the pixel split per octave below a tensor whose largest |pixel| is `top`"""
    s = h2.range_scale(h2.float_bits(top))
    rng = np.random.default_rng(seed)
    out = {}
    for j in OCTAVES:
        v = band(rng, n, j, 1.0)
        hi, lo = h2.split_pixels(v, s, flush)
        out[j] = float((np.abs((hi + lo) / s - v) / np.abs(v)).max())
    return s, out


def test_range_scale_puts_the_largest_value_into_its_window():
    rng = np.random.default_rng(0)
    for v in np.concatenate([np.float32([1.0, 2.0, np.nextafter(np.float32(4.0), np.float32(0)), 255.0, 1e-20, 3e20, 2.0 ** 13, 2.0 ** 14]),
                             (rng.standard_normal(2000) * 2.0 ** rng.integers(-60, 60, 2000)).astype(np.float32)]):
        s = h2.range_scale(h2.float_bits(v))
        assert 2.0 ** 13 <= s * abs(float(v)) < 2.0 ** 14 and np.log2(s) == int(np.log2(s)), (v, s)
    assert h2.range_scale(0) == 1.0
    assert h2.range_scale(h2.float_bits(1e-38)) == 2.0 ** 100 and h2.range_scale(h2.float_bits(3e38)) == 2.0 ** -100      # the clamp


@pytest.mark.parametrize("top", [2.0, float(np.nextafter(np.float32(4.0), np.float32(0)))], ids=["top-of-tensor-at-window-bottom", "at-window-top"])
def test_pixel_split_error_per_octave_below_the_largest(top):
    """range.h: two half terms keep 2^-23 of a pixel down to 2^-15 of the largest pixel when that one sits at the bottom of its window
    [2^13, 2^14) (2^-16 when it sits at the top), 2^-22 one octave further down, and lose a bit per octave from there: the unit of lo
    has reached the half subnormals' 2^-24.  A unit that flushed half subnormals would lose a bit per octave from the 5th octave on."""
    s, kept = split_curve(top, False)
    _, flushed = split_curve(top, True)
    print("pixel split, largest pixel %.9g (scale 2^%d):" % (top, np.log2(s)))
    for j in OCTAVES:
        m = j + 1                             # octaves of the band below the window [2^13, 2^14): band j is [2^-j, 2^(1-j)), s = 2^12
        assert 2.0 ** (13 - m) == s * 2.0 ** -j, (s, m)
        bound, fbound = h2.split_error_bound(m), h2.split_error_bound(m, flush_subnormals=True)
        print("  octave -%-2d kept %.2e (bound %.2e)   flushed %.2e (bound %.2e)" % (j, kept[j], bound, flushed[j], fbound))
        assert kept[j] <= bound, (j, kept[j], bound)
        assert flushed[j] <= fbound, (j, flushed[j], fbound)
        below_top = j + np.log2(top)          # octaves between the band's lower edge and the tensor's largest value
        full = 15 if top == 2.0 else 16       # (the same scaled values lie one octave further below a largest pixel at the window's top)
        if below_top <= full:
            assert kept[j] <= 2.0 ** -23      # the claim of range.h
        if below_top <= full + 1:
            assert kept[j] <= 2.0 ** -22
        if 8 <= j <= 20:                      # the two hypotheses are 10x apart and more: a test at these octaves is decisive
            assert flushed[j] >= 10 * kept[j], (j, kept[j], flushed[j])


def test_weight_split_error_per_octave_below_the_channels_largest():
    """pack_h2r: the largest weight of the channel in [2^14, 2^15): 2^-23 down to 2^-16 of it, then a bit per octave (absolute error
    2^-25 of the scaled value: 2^-39 to 2^-40 of the largest)"""
    rng = np.random.default_rng(2)
    for top in (1.0, float(np.nextafter(np.float32(2.0), np.float32(0)))):
        print("weight split, largest weight of the channel %.9g:" % top)
        for j in OCTAVES:
            w = band(rng, 50000, j, 1.0).reshape(1, -1)
            w[0, 0] = top
            hi, lo, q = h2.split_weights(w)
            assert 2.0 ** 14 <= top * 2.0 ** q[0] < 2.0 ** 15
            rel = float((np.abs((hi + lo) * 2.0 ** -q[0] - w) / np.abs(w)).max())
            m = j + 1                          # band j is [2^-j, 2^(1-j)): m octaves below the window [2^14, 2^15) of a top in [1, 2)
            bound = h2.split_error_bound(m, top_exp=h2.W_TOP_EXP)
            print("  octave -%-2d %.2e (bound %.2e)" % (j, rel, bound))
            assert rel <= bound, (j, rel, bound)
            if j <= 16:
                assert rel <= 2.0 ** -23, (j, rel)
            absolute = float(np.abs((hi + lo) - w.astype(np.float64) * 2.0 ** q[0]).max())
            if j > 16:
                assert absolute <= 2.0 ** -25, (j, absolute)


def test_three_kept_products_against_the_float64_product():
    """dropped: lo * lo, at most 2^-11 * 2^-11 of the product; with the two splits' own 2^-23 each the three kept products are within
    2^-22 + 2^-22 of the float64 product of the fp32 operands, for operands near the top of their tensors"""
    rng = np.random.default_rng(3)
    for jx, jw in ((0, 0), (4, 8), (11, 11), (13, 14)):
        x, w = band(rng, 200000, jx, 1.0), band(rng, 200000, jw, 1.0).reshape(1, -1)
        w[0, 0] = 1.0
        s = h2.range_scale(h2.float_bits(2.0))
        xh, xl = h2.split_pixels(x, s)
        wh, wl, q = h2.split_weights(w)
        kept = h2.kept_products(xh, xl, wh[0], wl[0]) * 2.0 ** -q[0] / s
        exact = x.astype(np.float64) * w[0].astype(np.float64)
        rel = np.abs(kept - exact) / np.abs(exact)
        lolo = np.abs(xl * wl[0]) * 2.0 ** -q[0] / s / np.abs(exact)
        assert float(lolo.max()) <= 2.0 ** -22
        assert float(rel.max()) <= 2.0 ** -22 + 2.0 ** -22, (jx, jw, float(rel.max()))
        # every kept product is exact in fp32 (11 x 11 significant bits): the MFMA's fp32 accumulation is the only rounding left
        for a, b in ((xl, wh[0]), (xh, wl[0]), (xh, wh[0])):
            p = a * b
            assert np.array_equal(p.astype(np.float32).astype(np.float64), p)


def accumulate(planes, K, chunk):
    """fp32 accumulation of the three kept products (lo*hi, hi*lo, hi*hi: the kernels' order).  chunk = K: one rounding per product
    plane, as tests/test_bf16x3_cpu.py emulates it; chunk = 16: one rounding per MFMA, the exact sum of 16 products added to the fp32
    accumulator -- closer to the kernels, 3 K / 16 roundings"""
    (xh, xl), (wh, wl) = planes
    acc = np.zeros((xh.shape[0], wh.shape[1]), np.float32)
    for k0 in range(0, K, chunk):
        sl = slice(k0, k0 + chunk)
        for a, b in ((xl, wh), (xh, wl), (xh, wh)):
            acc = (acc.astype(np.float64) + a[:, sl] @ b[sl]).astype(np.float32)
    return acc.astype(np.float64)


def dot_curve(flush, K=256, seed=5):
    """error of a K-term dot product over sum|x||w| per octave of the pixels below the largest pixel 2.0 (weights at the top of their
    channel), in float64: the split's share alone"""
    rng = np.random.default_rng(seed)
    s = h2.range_scale(h2.float_bits(2.0))
    out = {}
    for j in OCTAVES:
        x = band(rng, 64 * K, j, 1.0).reshape(64, K)
        w = band(rng, K * 32, 0, 1.0).reshape(32, K)
        xh, xl = h2.split_pixels(x, s, flush)
        wh, wl, q = h2.split_weights(w, flush_subnormals=flush)
        got = h2.kept_products(xh, xl, wh.T, wl.T, np.matmul) * 2.0 ** -q[None, :].astype(np.float64) / s
        truth = x.astype(np.float64) @ w.astype(np.float64).T
        den = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T
        out[j] = float((np.abs(got - truth) / den).max())
    return out


# largest error of a 256-term dot product over sum|x||w| per octave of the pixels below the largest pixel: what a device that kept half
# subnormals shows, and what one that flushed them would show (tests/test_h2_octaves_gpu.py names a failure by the curve it matches)
def test_dot_products_per_octave_and_the_flushed_curve():
    kept, flushed = dot_curve(False), dot_curve(True)
    print("K = 256 dot product, error / sum|x||w| per octave below the largest pixel (kept | flushed):")
    for j in OCTAVES:
        print("  octave -%-2d %.2e | %.2e" % (j, kept[j], flushed[j]))
        m = j + 1
        # per element: the pixel's split error + the weight's (2^-23, top of its channel) + the dropped lo * lo (2^-22)
        assert kept[j] <= h2.split_error_bound(m) + 2.0 ** -23 + 2.0 ** -22 + 2.0 ** -40, (j, kept[j])
        if j <= 14:
            assert kept[j] <= 2.0 ** -22, (j, kept[j])             # "22-23 bits", per sum|x||w|
        if 10 <= j <= 20:                      # (at octave -8 only one residual in 2^7 is small enough to be flushed: 2x)
            assert flushed[j] >= 10 * kept[j], (j, kept[j], flushed[j])


@pytest.mark.parametrize("K", [1152, 4608])
def test_long_dot_products_stay_at_fp32_accumulation_noise(K):
    rng = np.random.default_rng(4)
    a = rng.standard_normal((64, K)).astype(np.float32) * 3
    b = (rng.standard_normal((K, 32)) * (2.0 / K) ** 0.5).astype(np.float32)
    s = h2.range_scale(h2.float_bits(np.abs(a).max()))
    xh, xl = h2.split_pixels(a, s)
    wh, wl, q = h2.split_weights(b.T)
    truth = a.astype(np.float64) @ b.astype(np.float64)
    plain = (a @ b).astype(np.float64)                                              # numpy's own fp32 GEMM
    scale = np.abs(truth).max()
    den = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    e32 = np.abs(plain - truth).max() / scale
    for chunk in (K, 16):
        acc = accumulate(((xh, xl), (wh.T, wl.T)), K, chunk) * 2.0 ** -q[None, :].astype(np.float64) / s
        e2 = np.abs(acc - truth).max() / scale
        print("K = %d, one rounding per %d terms: fp16x2 form %.2e of max|truth| (fp32 GEMM %.2e), %.2e of sum|a||b|" % (
            K, chunk, e2, e32, float((np.abs(acc - truth) / den).max())))
        if chunk == K:
            assert e2 <= 5e-7, (e2, e32)                                            # the bars of test_bf16x3_cpu.py, emulated as there
        assert e2 <= 4 * e32 + 2e-7, (chunk, e2, e32)
        # every rounding is at most 2^-24 of a partial sum, itself at most sum|a||b|
        assert float((np.abs(acc - truth) / den).max()) <= (3 * K / chunk) * 2.0 ** -24 + 2.0 ** -21
