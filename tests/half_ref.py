"""Expected values of ONE f16-mode convolution whose views are stored as half (conv_b3d.hip XH forms, conv_epilogue_h, the half branches
of splitk_reduce_kernel), the case table test_half_views_gpu.py runs and test_half_ref_cpu.py holds to the oracle, and the mutants that
table has to tell apart.  No tests in here.

A case is a conv_ref.Case (shape, launch geometry, epilogue) plus a FORM -- where x, the residual and y live: "h" half, "f" fp32,
"n" no residual -- and a kind:

  exact    dyadic operands: x and w integers (half-exact), residual and bias integers of magnitude <= 2048, epilogue bias (scale 1),
           activation none / ReLU / leaky 0.125.  sum |x||w| + |res| + |bias| < 2^24 at every output, so every fp32 partial sum is
           exact in any order and with any split factor and the rounding to half of a half output is the ONLY rounding: expected =
           np.float16(float64 value), compared bit for bit, signs of zero included (an fp32 output: the value itself).
           special "overflow": a bias of 60000 on three channels (expected: RTNE's infinity from 65520 on); "subnormal": x, residual and
           bias scaled by 2^-24, so that x is subnormal in half and the outputs fall on both sides of 2^-14 (expected keeps subnormals).
  bounded  x and residual standard normals rounded to half, w a scaled normal (the reference uses the half-rounded w), bias / bn /
           residual / leaky 0.1 in rotation.  fp32 output: the bound of conv_ref.py with D = 0 (the operands are exactly what the
           kernel multiplies); half output: every element inside [h(ref - b), h(ref + b)], h = RTNE to half (monotone: no cap).

Layout (layout()): all strides differ and no channel offset is 0.  Half x: Cs = Cin + 16 at channel 8 (column GEMM: the dense column
buffer), half y: r8(Cout) + 24 at 16, half residual: r8(Cout) + 16 at 8, each buffer one image longer than the view; fp32 operands as
in test_conv_views_gpu.py.  The host cannot write half views: half_buffer() is the fp32 canvas (and bias) of the identity producer that
fills a half buffer over its whole width -- the view's values, random half-exact integers around them, the view's own pad channels
zero (a residual's: -0.0, which the producer's bias of -2^-30 rounds to: a pad that is copied instead of computed shows), and for an
output buffer a fill pattern whose neighbours along channel, pixel, row and image all differ."""
import functools
import zlib

import numpy as np

import conv_ref as R
from plan_helpers import bn_params, r4

TILES = [82, 83, 84, 85, 88, 89]
KSUB = {82: 2, 83: 4, 84: 2, 85: 2, 88: 4, 89: 4}      # half steps per ring stage of the XH instantiations (launch_conv_b3d)
FORMS = [(x, r, y) for x in "hf" for r in "nhf" for y in "hf" if not (x == "f" and y == "f" and r != "h")]      # minus the two all-fp32 ones
XH_FORMS = [f for f in FORMS if f[0] == "h"]
HALF_OUT_OR_RES = [f for f in FORMS if f[1] == "h" or f[2] == "h"]
NEG_ZERO_BIAS = -2.0 ** -30      # fp32 -> half: -0.0
r8 = lambda c: (c + 7) // 8 * 8
r16 = lambda c: (c + 15) // 16 * 16


def amplitudes(K):
    """(|x| max, |w| max) of an exact case by the depth K of its sum: integers uniform in [-a, a] have a spread of a / sqrt(3), so the
    outputs' spread is about 4000 whatever K is -- most of them between 2^11 and 2^13, where half the integers / a quarter of them are
    not half values and a quarter / an eighth are ties (|x| 16, |w| 16 at K 2304; 44 / 16 at 288; 188 / 16 at 16)"""
    return max(4, int(round(12000.0 / np.sqrt(K) / 16))), 16


class HCase(object):
    """fam: who reports together; name: the shape's; form: (x, residual, y); rot: the epilogue of a bounded case"""

    def __init__(self, fam, name, tile, form, kind="exact", act=0, special=None, amp=None, rot=0, **kw):
        self.fam, self.name, self.form, self.kind, self.special = fam, name, form, kind, special
        self.xh, self.res, self.yh = form[0] == "h", form[1], form[2] == "h"
        if kind == "exact":
            epi, self.slope = "bias", 0.125
        else:
            epi, act = [("bias", 0), ("bn", 2)][rot % 2] if self.res == "n" else [("res", 1), ("bn+res", 2)][rot % 2]
            self.slope = R.SLOPE
        if self.res != "n" and "res" not in epi:
            epi += "+res"
        self.case = c = R.Case(fam, tile, epi=epi, act=act, f16=True, auto=tile is None, **kw)
        self.amp = amp or (amplitudes(c.K) if kind == "exact" else None)
        self.tile, self.act, self.Cout, self.C4 = tile, act, c.Cout, r4(c.Cout)

    @property
    def id(self):
        c = self.case
        return "%s-%s-t%s-x%s-r%s-y%s-%s%s-%s-n%d-%dx%d-%dx%d-act%d%s%s" % (
            self.fam, self.name, "auto" if self.tile is None else self.tile, self.form[0], self.form[1], self.form[2], self.kind,
            "-" + self.special if self.special else "", c.mode, c.N, c.Cin, c.Cout, c.H, c.W, self.act, "-odd" if c.odd else "",
            "-splitk" if c.ksplit else "")

    @property
    def data_key(self):
        return (self.case.data_key, self.kind, self.special, self.amp, tuple(sorted(self.case.epi)))


#        name        shape                                                                what it hits
GEOMETRY = [
    ("k1cin16",   dict(Cin=16, Cout=40, H=8, W=16, N=1, k=1, p=0)),                     # M exactly 128; K 16 in K_pad 32: one real half step
    ("k1cin48s2", dict(Cin=48, Cout=136, k=1, s=2, p=0)),                               # K 48 in 64
    ("k3cin16",   dict(Cin=16, Cout=40, H=9, W=11, N=2)),                               # K 144 in 160: 10 half steps, the last out of range
    ("all4",      dict(Cin=16, Cout=72, H=11, W=17, k=(3, 5), s=(2, 1), p=(1, 3), d=(1, 2))),      # every pair unequal
    ("s2odd",     dict(Cin=32, Cout=136, N=2, s=2)),                                    # strided window on an odd map
    ("d2",        dict(Cin=32, Cout=40, H=9, W=19, p=2, d=2)),                          # M 513 = 4 x 128 + 1
    ("map1x1",    dict(Cin=64, Cout=40, H=1, W=1, amp=(94, 16))),                      # map smaller than the filter (one live tap: K 64 of 576)
    ("m257",      dict(Cin=32, Cout=136, H=1, W=257, N=1, k=1, p=0)),                   # one pixel above the 256-pixel tile
]
DEEP = dict(Cin=256, H=6, W=7, N=1, ksplit=True)
DEEP_ANISO = dict(Cin=256, Cout=136, H=6, W=9, N=1, k=(1, 3), s=(2, 1), p=(0, 1), d=(1, 2), ksplit=True)


def _cases():
    out = []
    # forms: every form on every tile, base shape (Cin 32, 13x19, N 3, 3x3 p1: M 741, 18 half steps)
    for ti, t in enumerate(TILES):
        for fi, f in enumerate(FORMS):
            out.append(HCase("forms", "base", t, f, act=(ti + fi) % 3, Cout=64 if t == 88 else 136))
    for t in (84, 89):
        for fi, f in enumerate(FORMS):
            out.append(HCase("bounded", "base", t, f, kind="bounded", rot=fi + (t == 89)))
    # geometry: each shape on 84 (KSUB 2), on 88 or 83 (KSUB 4, by Cout) with a half x, and with no tile= under any form
    for gi, (name, g) in enumerate(GEOMETRY):
        for ji, t in enumerate((84, 88 if g["Cout"] <= 64 else 83, None)):
            forms = FORMS if t is None else XH_FORMS
            out.append(HCase("geometry", name, t, forms[(2 * gi + ji) % len(forms)], act=(gi + ji) % 3, **g))
    # Cout: 8 the smallest a half layer may have, 18 with pad channels, 129 and 260 ragged
    for ci, Cout in enumerate((8, 18, 129, 260)):
        for ji, t in enumerate((88 if Cout <= 64 else 84, 82)):
            out.append(HCase("cout", "cout%d" % Cout, t, HALF_OUT_OR_RES[(2 * ci + ji) % 8], act=(ci + ji) % 3, Cout=Cout))
    # split over K: the reduce kernel reads the half residual and stores half
    i = 0
    for Cout in (136, 18):
        for t in (82, 84, 88, None):
            out.append(HCase("splitk", "deep", t, HALF_OUT_OR_RES[i % 8], act=i % 3, Cout=Cout, **DEEP))
            i += 1
    out.append(HCase("splitk", "deepaniso", 84, ("h", "h", "h"), act=1, **DEEP_ANISO))
    # column GEMM on a dense half column buffer
    cols = dict(Cin=32, Cout=40, H=9, W=13, N=2, mode="cols")
    for t, f, act in ((84, "hnh", 1), (88, "hnf", 2), (88, "hhh", 0)):
        out.append(HCase("cols", "cols", t, tuple(f), act=act, **cols))
    for i, f in enumerate(("hnh", "hnf")):
        out.append(HCase("bounded-cols", "cols", 84, tuple(f), kind="bounded", rot=i + 1, **cols))
    # deconvolution 4x4 / 2: even and odd (cropped) outputs, one split over K
    dec = dict(Cout=18, H=6, W=9, mode="deconv2x")
    for odd, t, f, act in ((False, 84, "hnh", 2), (False, 88, "hnf", 1), (True, 88, "hnh", 0), (True, 84, "hnf", 2)):
        out.append(HCase("deconv", "deconv", t, tuple(f), act=act, odd=odd, **dec))
    out.append(HCase("deconv", "deconv", 84, ("h", "n", "h"), act=2, odd=True, Cin=64, ksplit=True, **dec))
    # overflow and the subnormal ladder
    out.append(HCase("special", "base", 84, ("h", "n", "h"), special="overflow"))
    out.append(HCase("special", "base", 89, ("f", "f", "h"), special="overflow"))
    out.append(HCase("special", "base", 84, ("h", "h", "h"), special="subnormal", amp=(64, 8), act=2))
    out.append(HCase("special", "base", 88, ("h", "n", "h"), special="subnormal", amp=(64, 8), Cout=64))
    out.append(HCase("special", "base", 83, ("h", "h", "f"), special="subnormal", amp=(64, 8)))
    return out


CASES = _cases()
EXACT = [c for c in CASES if c.kind == "exact"]
BOUNDED = [c for c in CASES if c.kind == "bounded"]


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def half(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _operands(key):
    ckey, kind, special, amp, epi = key
    mode, odd, Cin, Cout, H, W, N = ckey[:7]
    c = R._case_of(ckey)
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    xs = (N, 9 * Cin, H, W) if mode == "cols" else (N, Cin, H, W)
    ws = (Cin, Cout, 4, 4) if mode == "deconv2x" else (Cout, Cin, 3, 3) if mode == "cols" else (Cout, Cin, c.kh, c.kw)
    o = {}
    if kind == "exact":
        ints = lambda a, shape: rng.integers(-a, a + 1, shape).astype(np.float32)
        o["x"], o["w"] = ints(amp[0], xs), ints(amp[1], ws)
        o["res"], o["bias"] = ints(2048, (N, Cout, c.Ho, c.Wo)), ints(2048, Cout)
        if special == "overflow":
            o["bias"][[1, Cout // 2, Cout - 1]] = 60000.0
        if special == "subnormal":
            for n in ("x", "res", "bias"):
                o[n] = o[n] * np.float32(2.0 ** -24)
    else:
        o["x"] = half(rng.standard_normal(xs))
        o["w"] = R.f32(rng.standard_normal(ws) / np.sqrt(c.K))
        o["res"] = half(rng.standard_normal((N, Cout, c.Ho, c.Wo)))
        o["bias"] = R.f32(rng.standard_normal(Cout) * 0.5)
        o["bn"] = bn_params(rng, "bn", Cout, Cout - 1)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def operands(hc):
    """{"x", "w", "res", "bias", "bn"} of a case: shared and read-only (x and res half-exact)"""
    return _operands(hc.data_key)


def act64(v, act, slope):
    return np.maximum(v, 0.0) if act == 1 else np.where(v > 0, v, v * np.float64(np.float32(slope))) if act == 2 else v


class Ref(object):
    pass


def finish(hc, conv, A=None):
    """Ref (float64, (N, Cout, Ho, Wo)) of a case from ANY contraction: pre (conv * scale + shift), v (+ residual), y (activated) and,
    given the same contraction of the absolute values, the bound of conv_ref.py with D = 0"""
    o = operands(hc)
    scale, shift, _, _ = R.epilogue_constants(hc.case, o)
    bc = lambda a: a.astype(np.float64)[None, :, None, None]
    r = Ref()
    r.res = o["res"].astype(np.float64) if hc.res != "n" else np.zeros_like(conv)
    r.pre = conv * bc(scale) + bc(shift)
    r.v = r.pre + r.res
    r.y = act64(r.v, hc.act, hc.slope)
    r.shift = bc(shift) * np.ones_like(conv)
    if A is not None:
        r.A = A
        r.bound = (hc.case.K + 8) * R.U * A * np.abs(bc(scale)) + 2 * R.U * (np.abs(bc(shift)) + np.abs(r.res) + np.abs(r.v))
    return r


@functools.lru_cache(maxsize=None)
def _contraction(key):
    o = _operands(key)
    c = R._case_of(key[0])
    x, w = o["x"].astype(np.float64), half(o["w"]).astype(np.float64)
    return R.plain_conv(c, x, w), R.plain_conv(c, np.abs(x), np.abs(w))


def reference(hc):
    """Ref of a case: pre, res, v, y, A, bound (float64)"""
    return finish(hc, *_contraction(hc.data_key))


# ---- layout and the producers' canvases ---------------------------------------------------------------------------------------------
def layout(hc):
    """{"x" / "y" / "r": (Cs, c0, C, H, W)} of the views of a case: half buffers in elements of 2 bytes, fp32 canvases in words"""
    c = hc.case
    cols = c.mode == "cols"
    Cx = 9 * c.Cin if cols else c.Cin
    out = {"x": ((Cx, 0) if cols and hc.xh else (Cx + 16, 8) if hc.xh else (Cx, 0) if cols else (r4(Cx) + 8, 4)) + (Cx, c.H, c.W),
           "y": ((r8(c.Cout) + 24, 16) if hc.yh else (r4(c.Cout) + 12, 8)) + (c.Cout, c.Ho, c.Wo)}
    if hc.res != "n":
        out["r"] = ((r8(c.Cout) + 16, 8) if hc.res == "h" else (r4(c.Cout) + 8, 4)) + (c.Cout, c.Ho, c.Wo)
    return out


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def fill_pattern(N, H, W, Cs):
    """half-exact, non-zero, and different from its neighbour along channel, pixel, row and image"""
    P = 2029      # prime
    assert all(n % P for n in (17, Cs, W, H))
    return ((np.arange(N * H * W * Cs, dtype=np.int64) * 17) % P + 1).astype(np.float32).reshape(N, H, W, Cs)


def half_buffer(hc, which, poison=False):
    """(canvas, bias) of the identity producer of the half buffer `which` ("x", "r", "y"): canvas (N + 1, H, W, r16(Cs)) fp32 (the
    producer's Cin is a multiple of 16), bias (Cs,) fp32.  poison: NaN -- by the bias on every channel outside the view, by the canvas
    on the whole extra image (a NaN in the canvas of a view's pixel would reach the view's channels through the zero weights)"""
    Cs, c0, C, H, W = layout(hc)[which]
    N = hc.case.N
    bias = np.zeros(Cs, np.float32)
    if which == "y":
        canvas = np.zeros((N + 1, H, W, r16(Cs)), np.float32)
        canvas[..., :Cs] = fill_pattern(N + 1, H, W, Cs)
        return canvas, bias
    rng = np.random.default_rng(zlib.crc32(repr((hc.data_key, which)).encode()))
    canvas = rng.integers(-64, 65, (N + 1, H, W, r16(Cs))).astype(np.float32)
    canvas[:N, :, :, c0:c0 + r4(C)] = 0.0
    canvas[:N, :, :, c0:c0 + C] = nhwc(operands(hc)["x" if which == "x" else "res"])
    if which == "r":
        bias[c0 + C:c0 + r4(C)] = NEG_ZERO_BIAS
    if poison:
        bias[:c0] = np.nan
        bias[c0 + r4(C):] = np.nan
        canvas[N] = np.nan
    return canvas, bias


def half_buffer_bits(hc, which):
    """what the half buffer holds once its producer has run: (N + 1, H, W, Cs) uint16"""
    Cs = layout(hc)[which][0]
    canvas, bias = half_buffer(hc, which)
    return (canvas[..., :Cs].astype(np.float64) + bias.astype(np.float64)).astype(np.float16).view(np.uint16)


# ---- roundings --------------------------------------------------------------------------------------------------------------------
def rtne(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(np.float16)


def trunc(v):
    """towards zero (mutant)"""
    v = np.asarray(v, np.float64)
    h = rtne(v)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(h.astype(np.float64)) > np.abs(v), np.nextafter(h, np.float16(0)), h)


def _neighbours(v):
    """(lo, hi, tie): the half values on either side of v (lo towards zero) and whether v lies exactly half way between them"""
    v = np.asarray(v, np.float64)
    lo = trunc(v)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = np.nextafter(lo, np.copysign(np.float16(np.inf), v).astype(np.float16))
        tie = (lo.astype(np.float64) != v) & (np.abs(v - lo.astype(np.float64)) == np.abs(hi.astype(np.float64) - v))
    return lo, hi, tie


def ties_away(v):
    """nearest, ties away from zero (mutant)"""
    lo, hi, tie = _neighbours(v)
    return np.where(tie, hi, rtne(v))


def is_half_exact(v):
    with np.errstate(invalid="ignore"):
        return rtne(v).astype(np.float64) == v


def is_tie(v):
    return _neighbours(v)[2]


# ---- expected bits and the mutants ----------------------------------------------------------------------------------------------------
def store(hc, y, rnd=rtne):
    """(N, Ho, Wo, r4(Cout)) bits as stored -- uint16 of a half output, uint32 of an fp32 one -- from y (N, Cout, Ho, Wo) float64; the
    pad channels +0"""
    a = nhwc(y)
    out = np.zeros(a.shape[:3] + (hc.C4,), np.uint16 if hc.yh else np.uint32)
    out[..., :hc.Cout] = rnd(a).view(np.uint16) if hc.yh else a.astype(np.float32).view(np.uint32)
    return out


def expected(hc):
    return store(hc, reference(hc).y)


def ksub_tail_applies(hc):
    c = hc.case
    return hc.xh and c.mode != "deconv2x" and KSUB.get(hc.tile) == 4 and (R.k_pad(c) // 16) % 4 != 0 and not c.ksplit


def _gemm_rows(hc, bits, fn):
    """apply fn to the (M, C4) matrix of GEMM rows the kernel's epilogue sees: the pixels in order; a deconvolution: one matrix per
    parity class over the INPUT pixels, rows a cropped output drops marked invalid.  fn(rows, valid) -> rows"""
    c = hc.case
    if c.mode != "deconv2x":
        return fn(bits.reshape(-1, hc.C4), np.ones(bits.size // hc.C4, bool)).reshape(bits.shape)
    full = np.zeros((c.N, 2 * c.H, 2 * c.W, hc.C4), bits.dtype)
    ok = np.zeros((c.N, 2 * c.H, 2 * c.W), bool)
    full[:, :c.Ho, :c.Wo], ok[:, :c.Ho, :c.Wo] = bits, True
    for py in (0, 1):
        for px in (0, 1):
            rows = fn(np.ascontiguousarray(full[:, py::2, px::2]).reshape(-1, hc.C4), np.ascontiguousarray(ok[:, py::2, px::2]).reshape(-1))
            full[:, py::2, px::2] = rows.reshape(c.N, c.H, c.W, hc.C4)
    return np.ascontiguousarray(full[:, :c.Ho, :c.Wo])


def _swap_row_pairs(rows, valid):
    """odd lanes (odd channels) hold rows e and e + 1 the other way round"""
    out = rows.copy()
    M = rows.shape[0] // 2 * 2
    both = valid[0:M:2] & valid[1:M:2]
    a, b = rows[0:M:2, 1::2], rows[1:M:2, 1::2]
    out[0:M:2, 1::2] = np.where(both[:, None], b, a)
    out[1:M:2, 1::2] = np.where(both[:, None], a, b)
    return out


def _x_with_4_byte_taps(hc):
    """the input every tap reads when the tap table's byte offsets are computed for 4-byte elements on a half view: element
    2 * ((ky dh W + kx dw) xCs + ci) behind the window's first one, zero outside the buffer; which taps are in range is decided by
    (dy, dx) as before.  Returns (N, Ho, Wo, taps, Cin) float64"""
    c = hc.case
    Cs, c0, C, H, W = layout(hc)["x"]
    buf = half_buffer_bits(hc, "x").view(np.float16).astype(np.float64).reshape(-1)
    cols = c.mode == "cols"
    kh, kw, Cin = (1, 1, C) if cols else (c.kh, c.kw, c.Cin)
    sh, sw, ph, pw, dh, dw = (1, 1, 0, 0, 1, 1) if cols else (c.sh, c.sw, c.ph, c.pw, c.dh, c.dw)
    n, oy, ox = np.meshgrid(np.arange(c.N), np.arange(c.Ho), np.arange(c.Wo), indexing="ij")
    iy0, ix0 = oy * sh - ph, ox * sw - pw
    base = ((n * H + iy0) * W + ix0) * Cs + c0
    out = np.zeros((c.N, c.Ho, c.Wo, kh * kw, Cin))
    for ky in range(kh):
        for kx in range(kw):
            ok = (iy0 + ky * dh >= 0) & (iy0 + ky * dh < H) & (ix0 + kx * dw >= 0) & (ix0 + kx * dw < W)
            idx = base[..., None] + 2 * ((ky * dh * W + kx * dw) * Cs + np.arange(Cin))
            inside = ok[..., None] & (idx >= 0) & (idx < buf.size)
            out[:, :, :, ky * kw + kx] = np.where(inside, buf[np.clip(idx, 0, buf.size - 1)], 0.0)
    return out


MUTANTS = ["trunc", "ties_away", "round_before_act", "round_before_res", "res_as_fp32", "chan_pair", "row_pair", "ksub_tail",
           "tap_esize4", "deconv_parity", "pad_from_res"]


def applies(hc, mutant):
    """does the mutant model something the case's kernel does at all"""
    c = hc.case
    # (a leaky slope of 0.125 commutes with the rounding of a normal half: rounding before the activation shows only where the
    # activated value is subnormal, and under the slope 0.1 of the bounded cases)
    return {"trunc": hc.yh, "ties_away": hc.yh, "round_before_act": hc.yh and hc.act == 2 and (hc.kind == "bounded" or hc.special == "subnormal"),
            "round_before_res": hc.yh and hc.res != "n",
            "res_as_fp32": hc.res == "h", "chan_pair": hc.yh or hc.res == "h", "row_pair": hc.yh or hc.res == "h",
            "ksub_tail": ksub_tail_applies(hc), "tap_esize4": hc.xh and c.mode != "deconv2x", "deconv_parity": c.mode == "deconv2x",
            "pad_from_res": hc.res == "h" and hc.Cout % 4 != 0}[mutant]


def mutant(hc, name):
    """the bits a kernel with the named fault would store (same shape and type as expected())"""
    assert applies(hc, name), (hc.id, name)
    c, o, ref = hc.case, operands(hc), reference(hc)
    conv = _contraction(hc.data_key)[0]
    if name == "trunc":
        return store(hc, ref.y, trunc)
    if name == "ties_away":
        return store(hc, ref.y, ties_away)
    if name == "round_before_act":
        return store(hc, act64(rtne(ref.v).astype(np.float64), hc.act, hc.slope))
    if name == "round_before_res":
        return store(hc, act64(rtne(ref.pre).astype(np.float64) + ref.res, hc.act, hc.slope))
    if name == "res_as_fp32":      # the residual's bytes at (pixel * Cs + c0) * 2 + 4 * channel
        Cs, c0, C, H, W = layout(hc)["r"]
        flat = half_buffer_bits(hc, "r").reshape(-1).astype(np.uint32)
        idx = (np.arange(c.N * H * W)[:, None] * Cs + c0 + 2 * np.arange(C)).reshape(c.N, H, W, C)
        res = (flat[idx] | (flat[idx + 1] << 16)).view(np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            return store(hc, act64(ref.pre + np.transpose(res, (0, 3, 1, 2)), hc.act, hc.slope))
    if name == "chan_pair":
        return np.ascontiguousarray(expected(hc)[..., np.arange(hc.C4) ^ 1])
    if name == "row_pair":
        return _gemm_rows(hc, expected(hc), _swap_row_pairs)
    if name == "ksub_tail":      # the half step behind the last one of K_pad repeats it instead of multiplying zeros
        K, Kp = c.K, R.k_pad(c)
        w = o["w"].astype(np.float64)
        flat = np.transpose(w, (0, 2, 3, 1)).reshape(c.Cout, -1).copy()      # k = tap * Cin + ci
        flat[:, :Kp - 16] = 0.0
        wl = np.transpose(flat.reshape(c.Cout, w.shape[2], w.shape[3], w.shape[1]), (0, 3, 1, 2))
        return store(hc, finish(hc, conv + R.plain_conv(c, o["x"].astype(np.float64), wl)).y)
    if name == "tap_esize4":
        g = _x_with_4_byte_taps(hc)
        w = o["w"].astype(np.float64)
        wt = np.transpose(w, (2, 3, 1, 0)).reshape(g.shape[3], -1, c.Cout) if c.mode != "cols" else \
            np.transpose(w, (2, 3, 1, 0)).reshape(1, -1, c.Cout)
        return store(hc, finish(hc, np.einsum("nhwtc,tck->nkhw", g, wt)).y)
    if name == "deconv_parity":      # the row parity classes the other way round
        full = R.deconv64(o["x"].astype(np.float64), o["w"].astype(np.float64))
        sw = np.empty_like(full)
        sw[:, :, 0::2], sw[:, :, 1::2] = full[:, :, 1::2], full[:, :, 0::2]
        return store(hc, finish(hc, sw[:, :, :c.Ho, :c.Wo]).y)
    if name == "pad_from_res":
        out = expected(hc)
        out[..., hc.Cout:] = 0x8000 if hc.yh else 0x80000000
        return out
    raise KeyError(name)


def interval(hc):
    """(lo, hi) of a bounded case with a half output as half values (N, Ho, Wo, Cout): h(ref - b), h(ref + b)"""
    ref = reference(hc)
    return rtne(nhwc(ref.y - ref.bound)), rtne(nhwc(ref.y + ref.bound))
