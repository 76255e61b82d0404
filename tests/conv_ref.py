"""float64 reference of one plan `conv` line on channel sub-views, the bounds an fp32 evaluation of it has to meet, and the case table
that test_conv_ref_cpu.py (the reference against the oracle and torch) and test_conv_views_gpu.py (every convolution kernel against
the reference) share.  No tests in here.

    v  = conv(x, w) * scale + shift (+ residual)        scale / shift as accel_hip.cpp finalize_conv folds them, in fp32
    y  = act(v)                                         act: 0 none, 1 ReLU, 2 leaky 0.1
    y2 = relu(y * scale2 + shift2)                      the dual output of the pre-activation trunk

Bounds (u = 2^-24, K = taps x Cin, A = sum |x| |w| of the output = the same convolution of the absolute values):

    |y - ref|   <= ((K + 8) u A + D) |scale| + 2 u (|shift| + |res| + |v|)
    |y2 - ref2| <= |scale2| (bound of y) + 2 u |y2|

the worst case of an fp32 sum in any order and with any split factor; D is what a split-operand form drops: bf16x3 2^-21 A (the six
kept products, test_bf16x3_cpu.py), fp16x2 the distance of the form's exact model (h2_model.py, pixel scale from the view's maximum)
from the convolution.  An f16-mode layer is specified on operands rounded to half (test_b3d_gpu.py).  Cases with K <= 576 meet the
bars the suite already holds these kernels to as well: 1e-6 max|ref| (direct forms), 3e-6 max|ref| (Winograd), 1e-5 max(1, max|ref|)
(f16 mode).  Winograd evaluations are held to the bars alone; a deep-K one (K > 576) to four times the error of an fp32 restatement of
F(2x2, 3x3) on the same inputs (wino32 below), never less than 3e-6.

Kernel size, stride, padding and dilation of a case are each an int or an (h, w) pair.  Beside CASES (224 lines: 217 run, 7 refused)
the geometry sweep crosses the 26 shapes of GEOMETRY with the 22 rows of GEOMETRY_KERNELS: 572 pairs, of which 507 run, 50 must be
refused (RULES: a K step of 64, the DMA ring's Cin % 32, conv_b3d's Cin % 16) and 15 are f16-mode requests the layer declines (padded
Cin % 8: it stays fp32, GEOMETRY_DEMOTED) -- 11 % not run.  With the narrow kernel on the 11 anisotropic shapes, the split-K reduce on
one deep anisotropic K and the refusals of the kernels that demand square geometry: GEOMETRY_RUN 524, GEOMETRY_REFUSED 57.

The Winograd block sweep crosses the 13 shapes of WINO_GEOMETRY (all 3x3 / 1 / pad 1: what varies is how the map falls into blocks of
tiles, the K loop and its split -- wino_blocks, wino_split and wino_slices restate the launchers and conv_plan_split) with the 7 rows
of WINO_KERNELS (40 in fp32, 41-43 as bf16x3 and as fp16x2), once on the Gaussian operands of every other case and once on DYADIC
operands (Case.dyadic, part of data_key: integer pixels in [-4, 4], weights in {-8, -4, 0, 4, 8}, integer bias and residual, no batch
norm, leaky slope or second output), on which every intermediate of F(2x2, 3x3) in every form is an integer below 2^24 and the result
has no tolerance: WINO_RUN 182, WINO_REFUSED 7 (an odd side, Cin off the K step, pad 0)."""
import collections
import functools
import zlib

import numpy as np

import h2_model as H2
from plan_helpers import bn_params, conv64, deconv64, pair, r4

U = 2.0 ** -24
SLOPE = 0.1
DYADIC_X = 4            # dyadic operand set: integer pixels in [-4, 4], weights in {-8, -4, 0, 4, 8}


def f32(a):
    return np.asarray(a, np.float32)


def conv_out(n, k, s, p, d):
    """output size along one axis (n an int), or (Ho, Wo) of an (H, W) map with k, s, p, d each an int or an (h, w) pair"""
    if np.ndim(n) == 0:
        return (n + 2 * p - d * (k - 1) - 1) // s + 1
    return tuple(conv_out(n[i], pair(k)[i], pair(s)[i], pair(p)[i], pair(d)[i]) for i in (0, 1))


def _g(v):
    return "%d" % v if np.ndim(v) == 0 else "%dx%d" % tuple(v)


class Case(object):
    """One conv line: family (who reports the error ratios together), launch geometry (None: the narrow kernels take none; with
    auto=True: no tile= at all, the heuristic chooses), the view's shape (H x W: the INPUT map), kernel size / stride / padding /
    dilation (each an int or an (h, w) pair), the epilogue ("bias", "bn", "res", "dual" joined by +) and what ops() must report."""

    def __init__(self, fam, tile, Cin=32, Cout=136, H=13, W=19, N=3, k=3, s=1, p=1, d=1, epi="", act=0, split="b3", f16=False, mode="conv",
                 ksplit=False, narrow=None, odd=False, raises=False, auto=False, dyadic=False):
        self.fam, self.tile, self.Cin, self.Cout, self.H, self.W, self.N = fam, tile, Cin, Cout, H, W, N
        k, s, p, d = (v if np.ndim(v) == 0 else tuple(int(e) for e in v) for v in (k, s, p, d))      # hashable: part of data_key
        self.k, self.s, self.p, self.d, self.act, self.split, self.f16, self.mode = k, s, p, d, act, split, f16, mode
        self.epi = frozenset(t for t in epi.split("+") if t)
        assert self.epi <= {"bias", "bn", "res", "dual"}, epi
        self.ksplit, self.narrow, self.odd, self.raises, self.auto, self.dyadic = ksplit, narrow, odd, raises, auto, dyadic
        assert not auto or (tile is None and not narrow)
        assert not dyadic or (self.epi <= {"bias", "res"} and act in (0, 1) and mode == "conv")      # nothing that rounds
        (self.kh, self.kw), (self.sh, self.sw), (self.ph, self.pw), (self.dh, self.dw) = pair(k), pair(s), pair(p), pair(d)
        if mode == "deconv2x":
            self.Ho, self.Wo, self.K = 2 * H - odd, 2 * W - odd, 4 * Cin
        elif mode == "cols":
            self.Ho, self.Wo, self.K = H, W, 9 * Cin
        else:
            self.Ho, self.Wo = conv_out((H, W), k, s, p, d)
            self.K = self.kh * self.kw * Cin
        self.wino = tile in (40, 41, 42, 43)

    @property
    def id(self):
        return "%s-t%s-%s%s-n%d-%dx%d-%dx%d-%s%s-act%d-%s%s%s%s" % (
            self.fam, "auto" if self.auto else "none" if self.tile is None else self.tile, "f16" if self.f16 else self.split,
            "" if self.mode == "conv" else "-" + self.mode, self.N, self.Cin, self.Cout, self.H, self.W,
            "k%ss%sp%sd%s" % (_g(self.k), _g(self.s), _g(self.p), _g(self.d)), "-odd" if self.odd else "", self.act,
            "+".join(sorted(self.epi)) or "plain", "-splitk" if self.ksplit else "", "-dyadic" if self.dyadic else "",
            "-refused" if self.raises else "")

    @property
    def data_key(self):
        """cases with the same key share inputs, weights and epilogue constants (and so the float64 convolution); a dyadic case
        (small-integer operands: WINO_GEOMETRY) has one element more, so every other key keeps its repr and its seed"""
        key = (self.mode, self.odd, self.Cin, self.Cout, self.H, self.W, self.N, self.k, self.s, self.p, self.d)
        return key + ("dyadic",) if self.dyadic else key


def _case_of(key, **kw):
    return Case("", 0, *key[2:11], mode=key[0], odd=key[1], dyadic=len(key) > 11, **kw)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# Launch geometries conv_tile_valid() accepts in the shipped build, each in at least one case that runs the canary, pad-zero, value
# and NaN-independence assertions (86 / 87 are accepted by conv_tile_valid but retired in launch_conv_b3d: they must be refused):
#   fp32 MFMA tiles      0-4 | 5-9 | 10-12 | 13, 15 (14 with 10-12: the pipelined 8-wavefront schedule) | 16-19 (LDS-DMA) | 31-35
#   Winograd             40 (fp32), 41, 42, 43 (bf16x3 and fp16x2)
#   stem                 50 (fp32), 51 (bf16x3 and fp16x2)
#   weight-stationary    60
#   bf16x3 / fp16x2      70-75 (conv_igemm.hip; bf16x3 under either setting), 76, 77, 79, 80, 81 (conv_b3r.hip), 78 (halo, fp16x2 only)
#   f16 mode             76, 77, 79, 80, 81 and 82, 83, 84, 85, 88, 89 (conv_b3d.hip)
#   no geometry          conv_narrow_kernel (pixel), conv_narrow3x3_kernel<4> and <8>; splitk_reduce_kernel behind 0, 40-43, 76 and
#                        the deconvolution
ALL_TILES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 31, 32, 33, 34, 35]      # test_ops_gpu.ALL_TILES
CLASSES = {"s0": [0, 1, 2, 3, 4], "s5": [5, 6, 7, 8, 9], "s10": [10, 11, 12, 14], "s13": [13, 15], "s16": [16, 17, 18, 19], "s31": [31, 32, 33, 34, 35]}
ROT = [("bias", 0), ("bn", 2), ("res", 1), ("res+dual", 0)]      # bias; bn + leaky; residual + ReLU; dual behind a residual
B3_TILES = [70, 71, 72, 73, 74, 75, 76, 77, 79, 80, 81]
F16_TILES = [76, 77, 79, 80, 81, 82, 83, 84, 85, 88, 89]


def _cases():
    out = []
    # fp32 MFMA tiles: 3x3 s1 p1 per id, then per schedule class a pad case (Cout 18), 3x3 s2 p2 d2 and 1x1 s2 (ktab with xCs != Cin);
    # the epilogue rotates over the cases of a class.  Geometry 13 works in K steps of 64: Cin 64
    for cls, ids in CLASSES.items():
        shapes = [dict(tile=t) for t in ids] + [dict(tile=ids[0], Cout=18), dict(tile=ids[-1], s=2, p=2, d=2), dict(tile=ids[1], k=1, s=2, p=0)]
        for i, kw in enumerate(shapes):
            epi, act = ROT[i % 4]
            out.append(Case("igemm-" + cls, Cin=64 if kw["tile"] == 13 else 32, epi=epi, act=act, **kw))
    # bf16x3 / fp16x2 forms; Cin 40: K = 360, K_pad = 384 -- the out-of-range granules of ktab, the kernels' Cin % 32 != 0 loaders
    for split in ("b3", "h2"):
        for i, t in enumerate(B3_TILES):
            epi, act = ROT[i % 4]
            out.append(Case("split-" + split, t, epi=epi, act=act, split=split))
            epi, act = ROT[(i + 2) % 4]
            out.append(Case("split-" + split, t, Cin=40, epi=epi, act=act, split=split))
        out.append(Case("split-" + split, 76, Cout=18, epi="bn", act=2, split=split))
    # Winograd F(2x2, 3x3): even maps
    for t, split in [(40, "b3"), (41, "b3"), (42, "b3"), (43, "b3"), (41, "h2"), (42, "h2"), (43, "h2")]:
        for epi, act in ROT:
            out.append(Case("wino-" + ("fp32" if t == 40 else split), t, Cout=72, H=12, W=18, epi=epi, act=act, split=split))
        out.append(Case("wino-" + ("fp32" if t == 40 else split), t, Cout=18, H=12, W=18, epi="bn", act=2, split=split))
    # ... split over K (conv_plan_split: at least 8 K steps -- of 8 channels for 40, of 16 for 41-43), finished by the split-K reduce
    out.append(Case("wino-splitk", 40, Cin=64, Cout=72, H=8, W=8, N=1, epi="res+dual", ksplit=True))
    for t in (41, 42, 43):
        out.append(Case("wino-splitk", t, Cin=128, Cout=72, H=8, W=8, N=1, epi=ROT[t % 4][0], act=ROT[t % 4][1], ksplit=True))
    # stem: a 3-channel NHWC view (Cs 12 at channel 4), 7x7 / 2
    for t, split in [(50, "b3"), (51, "b3"), (51, "h2")]:
        for epi, act in (("bias", 0), ("bn", 1)):
            out.append(Case("stem", t, Cin=3, Cout=64, H=26, W=38, k=7, s=2, p=3, epi=epi, act=act, split=split))
    out.append(Case("stem", 50, Cin=3, Cout=64, H=26, W=38, k=7, s=2, p=3, epi="res", raises=True))
    out.append(Case("stem", 51, Cin=3, Cout=64, H=26, W=38, k=7, s=2, p=3, epi="res+dual", raises=True))
    # weight-stationary 1x1
    for Cin, Cout in ((64, 256), (128, 128)):
        for epi, act in (("", 0), ("", 1), ("bn+res", 1)):
            out.append(Case("ws", 60, Cin=Cin, Cout=Cout, k=1, p=0, epi=epi, act=act))
    out.append(Case("ws", 60, Cin=64, Cout=256, k=1, p=0, act=2, raises=True))
    out.append(Case("ws", 60, Cin=64, Cout=256, k=1, p=0, epi="res+dual", raises=True))
    # halo (fp16x2 form only)
    for d in (1, 2):
        for epi, act in (("bn", 0), ("", 2)):
            out.append(Case("halo", 78, Cin=64, Cout=18, H=12, W=18, p=d, d=d, epi=epi, act=act, split="h2"))
    out.append(Case("halo", 78, Cin=64, Cout=18, H=12, W=18, epi="res", split="h2", raises=True))
    # narrow kernels: bn + residual + leaky, the output the last slice of its canvas
    out.append(Case("narrow", None, Cout=2, k=1, s=2, p=0, epi="bn+res", act=2, narrow="pixel"))
    out.append(Case("narrow", None, Cout=3, k=1, s=2, p=0, epi="bn+res", act=2, narrow="pixel"))
    out.append(Case("narrow", None, Cout=2, epi="bn+res", act=2, narrow="pixel"))
    out.append(Case("narrow", None, Cout=2, H=48, W=62, epi="bn+res", act=2, narrow="strip4"))
    out.append(Case("narrow", None, Cout=1, H=96, W=130, epi="bn+res", act=2, narrow="strip8"))
    # split-K reduce: low resolution, deep K (Winograd needs an even map: 6x8)
    for t, split, W in [(0, "b3", 7), (76, "b3", 7), (76, "h2", 7), (41, "b3", 8), (41, "h2", 8)]:
        fam = "splitk-wino" if t == 41 else "splitk"
        for epi, act in ROT:
            out.append(Case(fam, t, Cin=256, H=6, W=W, N=1, epi=epi, act=act, split=split, ksplit=True))
        out.append(Case(fam, t, Cin=256, Cout=18, H=6, W=W, N=1, epi="bn", act=2, split=split, ksplit=True))
    # deconvolution 4x4 / 2: even and odd (cropped) outputs
    for odd in (False, True):
        for t, split in [(0, "b3"), (76, "b3"), (76, "h2")]:
            out.append(Case("deconv", t, Cout=18, H=6, W=9, mode="deconv2x", epi="bias", act=2, split=split, odd=odd))
    out.append(Case("deconv", 0, Cin=64, Cout=18, H=6, W=9, mode="deconv2x", epi="bias", act=2, odd=True, ksplit=True))
    # column GEMM (the deformable convolutions): a dense column buffer, the output a sub-view
    for split in ("b3", "h2"):
        out.append(Case("cols", 81, Cout=40, H=9, W=13, mode="cols", epi="bn", act=2, split=split))
    # f16 mode on fp32 views
    F16_EPI = [("bias", 1), ("res", 0), ("res+dual", 0)]
    for i, t in enumerate(F16_TILES):
        for j, kw in enumerate((dict(), dict(s=2), dict(k=1, p=0))):
            epi, act = F16_EPI[(i + j) % 3]
            out.append(Case("f16", t, Cout=64 if t == 88 else 136, epi=epi, act=act, f16=True, **kw))
    out.append(Case("f16", 84, Cout=18, epi="bias", act=1, f16=True))
    for t in (86, 87):
        out.append(Case("f16", t, epi="bias", act=1, f16=True, raises=True))
    return out


CASES = _cases()
RUN_CASES = [c for c in CASES if not c.raises]
REFUSED = [c for c in CASES if c.raises]


# ---- the geometry sweep -----------------------------------------------------------------------------------------------------------
# GEOMETRY: shapes only (no kernel ids); every one exercises at least one of: a pair with unequal members (each pair once on its
# own, once all four together on a non-square map), a geometry of the networks at small size, a map smaller than its filter, an edge
# of the K loop (K_pad = roundup(taps x roundup(Cin, 4), 32), in steps of 32), of the pixel tile (64 / 128 / 256 pixels) or of the
# channel tile (32 / 64 / 128 / 256 channels).  The epilogue rotates over the shapes with ROT.
#        name            Cin Cout  H   W  N  k       s       p       d             what it is for
_G = [
    ("k1x3",             12,   5,  9, 11, 2, (1, 3), 1,      1,      1),         # K 36 in K_pad 64, Cin % 8 == 4, Cout 5
    ("k3x1",             32,  40,  9, 11, 2, (3, 1), 1,      1,      1),         # three steps (the DMA ring's unequal filter)
    ("k1x7",             36,  33,  7, 14, 2, (1, 7), 1,      1,      1),         # K 252 in 256 (8 steps), Cin % 8 == 4, Cout 33
    ("k5x3",             40,  40, 10,  9, 2, (5, 3), 1,      1,      1),         # K 600 in 608: 19 steps
    ("s1x2",             64, 129, 11, 13, 2, 3,      (1, 2), 1,      1),         # Cout 129; 18 steps (geometry 13 takes it)
    ("s2x1",             32,  40, 11, 14, 2, 3,      (2, 1), 1,      1),
    ("p0x1",             64,  40, 11, 14, 2, 3,      1,      (0, 1), 1),
    ("p2x0",             64, 260,  9, 12, 1, 3,      1,      (2, 0), 1),         # Cout 260 (every kernel takes it)
    ("d1x2",             20,  40, 11, 14, 2, 3,      1,      1,      (1, 2)),    # K 180 in 192, Cin % 8 == 4
    ("d2x1",             64,  40, 11, 14, 2, 3,      1,      1,      (2, 1)),
    ("all4",             16,  72, 11, 17, 3, (3, 5), (2, 1), (1, 3), (1, 2)),    # every pair unequal, 11 x 17 -> 6 x 15
    ("net7x7s2",          6,  33, 13, 17, 2, 7,      2,      3,      1),         # the stem's geometry on a 6-channel view (padded to 8): 13 steps
    ("net5x5s2",         32,  40, 13, 17, 1, 5,      2,      2,      1),         # K 800: 25 steps; M 63: below every tile
    ("net3x3s2odd",      32,  40, 13, 19, 2, 3,      2,      1,      1),
    ("net3x3s2even",     16,  40, 12, 16, 2, 3,      2,      1,      1),
    ("net1x1s2",         64,  40, 13, 19, 3, 1,      2,      0,      1),         # two steps
    ("net3x3d2",         32,  40,  9, 19, 3, 3,      1,      2,      2),         # M 513 = 4 x 128 + 1, tiles straddle the three images
    ("net3x3p0",         32,  40, 10, 18, 2, 3,      1,      0,      1),         # Ho != H; M exactly 256
    ("map1x1",           64,  40,  1,  1, 3, 3,      1,      1,      1),         # maps smaller than the filter
    ("map2x3",           16,   5,  2,  3, 3, 3,      1,      1,      1),
    ("map1xW",           32,  40,  1, 19, 2, 3,      1,      1,      1),
    ("map4x5k7",          8,  40,  4,  5, 3, 7,      2,      3,      1),
    ("k1step",           32, 129,  8, 16, 1, 1,      1,      0,      1),         # one K step; M exactly 128
    ("k1cin4",            4,  40,  8, 16, 2, 1,      1,      0,      1),         # K 4 in K_pad 32
    ("k3x3cin4",          4, 260,  5,  7, 1, 3,      1,      1,      1),         # K 36 in K_pad 64
    ("k3steps",          96,  40,  8, 16, 3, 1,      1,      0,      1),         # an odd number of steps at Cin 96; M 384
]
GEOMETRY = collections.OrderedDict((g[0], dict(zip(("Cin", "Cout", "H", "W", "N", "k", "s", "p", "d"), g[1:]))) for g in _G)
ANISOTROPIC = ["k1x3", "k3x1", "k1x7", "k5x3", "s1x2", "s2x1", "p0x1", "p2x0", "d1x2", "d2x1", "all4"]
# the sides on which NO tap of any output pixel falls outside the map (nothing there for a loader to get wrong): no padding on that
# axis, or a strided window that ends inside an even map; every other shape has out-of-range taps on all four sides
EDGE_FREE = {"p0x1": "tb", "p2x0": "lr", "net3x3s2even": "br", "net1x1s2": "tblr", "net3x3p0": "tblr", "k1step": "tblr", "k1cin4": "tblr",
             "k3steps": "tblr"}


def k_pad(case):
    """accel_hip.cpp finalize_conv: K_pad = roundup(kh kw roundup(Cin, 4), 32)"""
    return (case.kh * case.kw * r4(case.Cin) + 31) // 32 * 32


# What a kernel's launcher rules out, restated once each as a predicate on the case:
RULES = {
    None: lambda c: True,
    # conv_igemm.hip launch_conv_igemm: `if (p.K_pad % conv_tile_bk(tile)) return hipErrorInvalidValue;` -- geometry 13 steps K by 64
    "bk64": lambda c: k_pad(c) % 64 == 0,
    # conv_igemm.hip launch_conv_igemm: `if (p.Cin % 32) return hipErrorInvalidValue;   // DMA variants need wave-uniform taps per K step`
    "dma": lambda c: r4(c.Cin) % 32 == 0,
    # accel_hip.cpp finalize_conv: `c.f16 = (want_f16 && c.Cin % (want_f16 == 2 ? 4 : 8) == 0 && cout_store > 4) ? want_f16 : 0;` -- the layer
    # is then an fp32 layer (ops() reports mode 0 or 3, never 1): nothing is refused, the fp32 rows already run that pair (DEMOTED)
    "f16": lambda c: r4(c.Cin) % 8 == 0,
    # conv_b3d.hip `bool conv_b3d_eligible(const ConvParams& p) { return p.Cin % 16 == 0 && p.ktab != nullptr; }`, and launch_conv_igemm's
    # `if (!p.wb3r || p.f16 != 1) return hipErrorInvalidValue;` for the layers the rule above made fp32
    "b3d": lambda c: r4(c.Cin) % 16 == 0,
}
# one launch geometry per kernel template and loader path: (family, id, ACCEL_SPLIT, f16 mode, rule)
GEOMETRY_KERNELS = [
    ("geo-igemm", 0, "b3", False, None), ("geo-igemm", 5, "b3", False, None), ("geo-igemm", 10, "b3", False, None),
    ("geo-igemm", 13, "b3", False, "bk64"), ("geo-igemm", 31, "b3", False, None), ("geo-igemm", 16, "b3", False, "dma"),
    ("geo-b3", 70, "b3", False, None), ("geo-b3", 75, "b3", False, None),
    ("geo-b3r-b3", 76, "b3", False, None), ("geo-b3r-b3", 77, "b3", False, None), ("geo-b3r-b3", 80, "b3", False, None),
    ("geo-b3r-h2", 76, "h2", False, None), ("geo-b3r-h2", 77, "h2", False, None), ("geo-b3r-h2", 80, "h2", False, None),
    ("geo-f16", 0, "b3", True, "f16"), ("geo-f16", 10, "b3", True, "f16"), ("geo-f16-b3r", 76, "b3", True, "f16"),
    ("geo-f16-b3d", 82, "b3", True, "b3d"), ("geo-f16-b3d", 84, "b3", True, "b3d"), ("geo-f16-b3d", 88, "b3", True, "b3d"),
    # no tile= at all: conv_pick_tile chooses (and conv_plan_split splits K where it likes)
    ("geo-auto", None, "b3", False, None), ("geo-auto", None, "h2", False, None),
]
# the ids conv_tile_valid() accepts (conv_igemm.hip)
VALID_TILES = set(range(0, 20)) | set(range(31, 36)) | {40, 41, 42, 43, 50, 51, 60, 78} | set(range(70, 78)) | {79, 80, 81} | set(range(82, 90))


def _geometry_cases():
    run, refused, demoted = [], [], []
    for i, (name, g) in enumerate(GEOMETRY.items()):
        epi, act = ROT[i % 4]
        for fam, tile, split, f16, rule in GEOMETRY_KERNELS:
            c = Case(fam, tile, epi=epi, act=act, split=split, f16=f16, auto=tile is None, **g)
            if RULES[rule](c):
                run.append(c)
            elif rule == "f16":
                demoted.append(c)
            else:
                c.raises = True
                refused.append(c)
    # the narrow pixel kernel (no geometry id) on the anisotropic shapes, Cout 2 and 3 in turn; it has no second output
    for i, name in enumerate(ANISOTROPIC):
        epi, act = [("bias", 0), ("bn+res", 2), ("res", 1)][i % 3]
        run.append(Case("geo-narrow", None, epi=epi, act=act, narrow="pixel", **dict(GEOMETRY[name], Cout=2 + i % 2)))
    # ... and the split forms are not offered to narrow outputs (accel_hip.cpp finalize_conv: "the bf16x3 kernel takes layers with
    # more than 4 output channels only")
    for t, split in ((70, "b3"), (76, "b3"), (76, "h2")):
        refused.append(Case("geo-narrow", t, epi="bias", split=split, raises=True, **dict(GEOMETRY["k1x3"], Cout=3)))
    # the split-K reduce behind 0 and behind 76 on one deep-K shape with every pair unequal: 6 x 9 -> 3 x 7, K 768 in 24 steps
    deep = dict(Cin=256, Cout=136, H=6, W=9, N=1, k=(1, 3), s=(2, 1), p=(0, 1), d=(1, 2))
    for t, split in ((0, "b3"), (76, "b3"), (76, "h2")):
        for epi, act in (ROT[3], ROT[1]):
            run.append(Case("geo-splitk", t, epi=epi, act=act, split=split, ksplit=True, **deep))
    # kernels that demand square geometry in their *_eligible functions: Winograd, stem, halo, weight-stationary
    refused.append(Case("geo-square", 40, Cout=72, H=12, W=18, k=(3, 1), p=(1, 0), epi="bias", raises=True))
    refused.append(Case("geo-square", 50, Cin=3, Cout=64, H=26, W=38, k=7, s=(1, 2), p=3, epi="bias", raises=True))
    refused.append(Case("geo-square", 78, Cin=64, Cout=18, H=12, W=18, s=(1, 2), epi="bn", split="h2", raises=True))
    refused.append(Case("geo-square", 60, Cin=64, Cout=256, k=1, p=0, s=(1, 2), raises=True))
    return run, refused, demoted


GEOMETRY_RUN, GEOMETRY_REFUSED, GEOMETRY_DEMOTED = _geometry_cases()


# ---- the Winograd block sweep -------------------------------------------------------------------------------------------------------
# The Winograd kernels take one filter geometry (3x3 / 1 / pad 1, even maps); what they can get wrong is the decomposition of the map
# into blocks of tiles (2x2 output pixels each), the K loop and its split.  Both are restated here in plain Python.
WINO_TILES = (40, 41, 42, 43)


def wino_bhs(tile, TH):
    """log2 of the block height of the rectangular forms:
    conv_wino_b3.hip conv_wino_b3u_blocks: `const int s = TH >= 8 ? 3 : TH >= 4 ? 2 : 1;` (block = (1 << s) x (64 >> s) tiles)
    conv_wino_b3s.hip conv_wino_b3s_blocks: `const int s = TH >= 4 ? 2 : 1;` (block = (1 << s) x (32 >> s) tiles)"""
    return (3 if TH >= 8 else 2 if TH >= 4 else 1) if tile == 42 else (2 if TH >= 4 else 1)


def wino_blocks(tile, H, W, N):
    """(block height, block width, blocks per image or None, MT) in tiles, of an N x H x W map:
    40 / 41 -- conv_wino.hip launch_conv_wino, conv_wino_b3.hip launch_conv_wino_b3: `p.wino_T = p.M / 4; p.MT = (p.wino_T + TT - 1) /
    TT;` with TT = 64, the kernels' `const int tg = m0 + tl; ... const int n = tt / THW, rem = tt - n * THW; const int ty = rem / TW`:
    64 consecutive tiles in (n, ty, tx) order, a block straddles rows and images;
    42 / 43 -- conv_wino_b3u_blocks / conv_wino_b3s_blocks: `return n * ((TH + BH - 1) / BH) * ((TW + BW - 1) / BW);` and the kernels'
    `const int BX = (TW + BWm) >> bws, BY = (TH + (1 << bhs) - 1) >> bhs; un = mt / (BX * BY);`: a block never leaves its image."""
    TH, TW = H // 2, W // 2
    if tile in (40, 41):
        return 1, 64, None, (N * TH * TW + 63) // 64
    BH = 1 << wino_bhs(tile, TH)
    BW = (64 if tile == 42 else 32) // BH
    per = ((TH + BH - 1) // BH) * ((TW + BW - 1) // BW)
    return BH, BW, per, N * per


def wino_rows(cout_store):
    """conv_wino.hip `int conv_wino_rows(int cout_store) { return (cout_store + KK - 1) / KK * KK; }`, KK = 64"""
    return (cout_store + 63) // 64 * 64


def wino_nt(case):
    """launch_conv_wino*: `p.NT = p.wino_rows / KK;`"""
    return wino_rows(r4(case.Cout)) // 64


def wino_kstep(tile):
    """channels per K step: conv_wino.hip `constexpr int BKC = 8;`, conv_wino_b3.hip `BKC = 16`, conv_wino_b3s.hip `BKS = 16`"""
    return 8 if tile == 40 else 16


def wino_split(tile, case):
    """(ksplit, kt_per_split) of conv_igemm.hip conv_plan_split's two Winograd branches with no split_target set:
        if (p.no_split || p.narrow) return 0;
        const long blocks = <MT> * (long)conv_wino_rows(p.Cout_store) / 64;         MT as wino_blocks
        const int KT = p.Cin / 8 [40] or p.Cin / 16 [41-43], min_steps = 4;
        if (blocks >= 256 || KT < 2 * min_steps) return 0;
        int want = (int)((512 + blocks - 1) / blocks);
        int ks = want < KT / min_steps ? want : KT / min_steps;
        if (ks < 2) return 0;
        p.kt_per_split = ((KT + ks - 1) / ks + 1) / 2 * 2 [40: even, the K loop is unrolled by 2] or (KT + ks - 1) / ks [41-43];
        p.ksplit = (KT + p.kt_per_split - 1) / p.kt_per_split;
        if (p.ksplit < 2) { p.ksplit = 1; p.kt_per_split = 0; return 0; }"""
    if not case.ksplit:      # the plan line says nosplit=1
        return 1, 0
    blocks = wino_blocks(tile, case.H, case.W, case.N)[3] * wino_rows(r4(case.Cout)) // 64
    KT = case.Cin // wino_kstep(tile)
    if blocks >= 256 or KT < 8:
        return 1, 0
    ks = min((512 + blocks - 1) // blocks, KT // 4)
    if ks < 2:
        return 1, 0
    per = (KT + ks - 1) // ks
    if tile == 40:
        per = (per + 1) // 2 * 2
    ksplit = (KT + per - 1) // per
    return (ksplit, per) if ksplit >= 2 else (1, 0)


def wino_slices(tile, case):
    """the K steps of every slice, as the kernels take them: `nk = p.ksplit > 1 ? min(p.kt_per_split, nk_all - kb) : nk_all`"""
    KT = case.Cin // wino_kstep(tile)
    ksplit, per = wino_split(tile, case)
    return [KT] if ksplit == 1 else [min(per, KT - i * per) for i in range(ksplit)]


# WINO_GEOMETRY: shapes only, all 3x3 / 1 / pad 1; TH x TW = H / 2 x W / 2 tiles.  Every block class of 42 (8x8 for TH >= 8, 4x16 for
# 4 <= TH < 8, 2x32 below) and of 43 (4x8 for TH >= 4, 2x16 below) meets a map it fits exactly, one ragged in the tile rows alone, one
# in the tile columns alone and one in both with a ONE-tile corner block (test_conv_ref_cpu.py asserts it, and the rest of what this
# column says).  The epilogue rotates over the shapes with ROT.
#        name          Cin Cout  H    W  N     what it is for
_WG = [
    ("onetile",         16,   5,  2,   2, 1),  # one tile; one K step on 41-43 (two on 40); Cout_store 8; nblk 1
    ("strip",           32,  40,  2,  66, 3),  # TH 1: 2x32 / 2x16 with the lower tile row invalid, TW 33 = 32 + 1 = 16 + 16 + 1 (one-tile
                                               # corner blocks); 42's raw patch copy at its largest; linear blocks straddle the images
    ("th3w32",          48,  68,  6,  64, 2),  # two-row blocks ragged in the rows alone (the second has one valid row); three K steps;
                                               # a second channel block with 4 channels in use
    ("fit",             32,  64,  8,  32, 1),  # exact fit: 42 one 4x16 block, 43 two 4x8 blocks, 40 / 41 one block of 64 tiles; Cout 64
    ("th5w17",          64,  72, 10,  34, 2),  # 4 + 1 tile rows, 16 + 1 and 8 + 8 + 1 tile columns (one-tile corners); four K steps
    ("th2w32",          16, 132,  4,  64, 3),  # 2x32 (one block an image) and 2x16 exactly; Cout 2 x 64 + 4; linear blocks end with the image
    ("th8",             32,  40, 16,  16, 2),  # 42 switches to 8x8, exactly one block an image; 43: two 4x8 blocks an image
    ("th9w9",           80,  40, 18,  18, 1),  # 8x8 and 4x8 ragged by one both ways: the corner block holds ONE tile; five K steps;
                                               # K = 720 > 576: the wino32 bar; a linear block covers more than seven tile rows
    ("tall",            32,  40, 34,  16, 1),  # TH 17 = 2 x 8 + 1 = 4 x 4 + 1 with TW 8: 8x8 and 4x8 ragged in the rows alone
    ("wide",            16,  40, 16, 130, 1),  # TW 65 = 8 x 8 + 1: 8x8 and 4x8 ragged in the columns alone, the last column one tile wide
    ("deep",           512,  72,  4,   8, 2),  # nosplit=1: 32 (64 on 40) K steps in one slice; TH 2, TW 4: 2x32 / 2x16 ragged in the columns alone
    ("split54",        144,  72,  8,   8, 1),  # split over K: 41-43 KT 9 -> 5 + 4, 40 KT 18 -> 6 + 6 + 6; 4x16 / 4x8 ragged in the columns alone
    ("split_ragged",   176,  72, 14,  32, 2),  # split over K on blocks ragged in the rows (TH 7, the last 4-row class of 42): 41-43 KT 11
                                               # -> 6 + 5, 40 KT 22 -> 6 + 6 + 6 + 4: a short last slice in every kernel
]
WINO_GEOMETRY = collections.OrderedDict((g[0], dict(zip(("Cin", "Cout", "H", "W", "N"), g[1:]))) for g in _WG)
WINO_SPLIT_SHAPES = ("split54", "split_ragged")      # the only ones without nosplit=1
# (family, id, ACCEL_SPLIT): 40 in fp32, 41-43 as bf16x3 and as fp16x2
WINO_KERNELS = [("wino-geo-fp32", 40, "b3"), ("wino-geo-b3", 41, "b3"), ("wino-geo-b3", 42, "b3"), ("wino-geo-b3", 43, "b3"),
                ("wino-geo-h2", 41, "h2"), ("wino-geo-h2", 42, "h2"), ("wino-geo-h2", 43, "h2")]
# the epilogues of the dyadic operand set: nothing that rounds (no batch norm, no leaky slope, no second output)
DYADIC_ROT = [("bias", 0), ("", 1), ("res", 1), ("res", 0)]


def wino_case(name, fam, tile, split, dyadic=False, index=None):
    i = list(WINO_GEOMETRY).index(name) if index is None else index
    epi, act = (DYADIC_ROT if dyadic else ROT)[i % 4]
    ksplit = name in WINO_SPLIT_SHAPES
    return Case("wino-geo-splitk" if ksplit else fam, tile, epi=epi, act=act, split=split, ksplit=ksplit, dyadic=dyadic, **WINO_GEOMETRY[name])


def _wino_cases():
    run = [wino_case(name, fam, tile, split, dyadic) for dyadic in (False, True) for name in WINO_GEOMETRY for fam, tile, split in WINO_KERNELS]
    # what conv_wino_eligible / conv_wino_b3_eligible rule out, on sub-views: an odd side, input channels off the K step, no padding
    refused = [Case("wino-geo", 40, Cout=40, H=12, W=17, epi="bias", raises=True),
               Case("wino-geo", 43, Cout=40, H=11, W=18, epi="bias", raises=True),
               Case("wino-geo", 43, Cout=40, H=11, W=18, epi="bias", split="h2", raises=True),
               Case("wino-geo", 41, Cin=24, Cout=40, H=12, W=18, epi="bias", raises=True),
               Case("wino-geo", 40, Cin=8, Cout=40, H=12, W=18, epi="bias", raises=True),
               Case("wino-geo", 40, Cout=40, H=12, W=18, p=0, epi="bias", raises=True),
               Case("wino-geo", 42, Cout=40, H=12, W=18, p=0, epi="bias", raises=True)]
    return run, refused


WINO_RUN, WINO_REFUSED = _wino_cases()


# ---- operands ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operands(key):
    mode, odd, Cin, Cout, H, W, N, k, s, p, d = key[:11]
    c = _case_of(key)
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    o = {}
    if c.dyadic:
        # integers all the way: every intermediate of F(2x2, 3x3) (G g G^T of multiples of 4, B^T d B, the sums over the channels,
        # A^T m A), every term of a split operand and the epilogue are integers far below 2^24 -- an evaluation in ANY order is exact
        o["x"] = f32(rng.integers(-DYADIC_X, DYADIC_X + 1, (N, Cin, H, W)))
        o["w"] = f32(4 * rng.integers(-2, 3, (Cout, Cin, c.kh, c.kw)))
        o["res"] = f32(rng.integers(-64, 65, (N, Cout, c.Ho, c.Wo)))
        o["bias"] = f32(rng.integers(-16, 17, Cout))
        o["bn"] = o["bn2"] = {}
    elif mode == "cols":
        o["x"] = f32(rng.standard_normal((N, 9 * Cin, H, W)))          # the column buffer [pixel][tap][c] as NCHW planes
        o["w"] = f32(rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(c.K))
    elif mode == "deconv2x":
        o["x"] = f32(rng.standard_normal((N, Cin, H, W)))
        o["w"] = f32(rng.standard_normal((Cin, Cout, 4, 4)) / np.sqrt(c.K))
    else:
        o["x"] = f32(rng.standard_normal((N, Cin, H, W)))
        o["w"] = f32(rng.standard_normal((Cout, Cin, c.kh, c.kw)) / np.sqrt(c.K))
    if not c.dyadic:
        o["res"] = f32(rng.standard_normal((N, Cout, c.Ho, c.Wo)))
        o["bias"] = f32(rng.standard_normal(Cout) * 0.5)
        o["bn"] = bn_params(rng, "bn", Cout, Cout - 1)
        o["bn2"] = bn_params(rng, "bn2", Cout, Cout - 1, negative=True)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def operands(case):
    """{"x": (N, Cin, H, W) values of the input view, "w", "res", "bias", "bn", "bn2"}: shared and read-only"""
    return _operands(case.data_key)


def bn_fold32(bn, name, eps):
    """accel_hip.cpp bn_fold, in fp32"""
    g, b, mu, var = (bn[name + s] for s in ("_gamma", "_beta", "_moving_mean", "_moving_var"))
    sd = np.sqrt(var + np.float32(eps), dtype=np.float32)
    return g / sd, b - (g * mu) / sd


def epilogue_constants(case, o):
    """(scale, shift, scale2, shift2) as finalize_conv uploads them: fp32 (bias * scale added to shift)"""
    scale, shift = np.ones(case.Cout, np.float32), np.zeros(case.Cout, np.float32)
    if "bn" in case.epi:
        scale, shift = bn_fold32(o["bn"], "bn", 1e-5)
    if "bias" in case.epi:
        shift = shift + o["bias"] * scale
    s2 = b2 = None
    if "dual" in case.epi:
        s2, b2 = bn_fold32(o["bn2"], "bn2", 1e-5)
    return f32(scale), f32(shift), s2, b2


def plain_conv(case, x, w):
    """the float64 contraction of a case on any operands (linear in both; nothing is rounded)"""
    if case.mode == "deconv2x":
        return deconv64(x, w)[:, :, :case.Ho, :case.Wo]
    if case.mode == "cols":
        return conv64(x, np.transpose(w, (0, 2, 3, 1)).reshape(case.Cout, 9 * case.Cin, 1, 1))
    return conv64(x, w, case.s, case.p, case.d)


@functools.lru_cache(maxsize=None)
def _core(key, form):
    """(conv, A, D): the float64 contraction, the same on absolute values, what the form `form` ("", "b3", "h2", "f16") drops"""
    case = _case_of(key)
    o = _operands(key)
    x, w = o["x"].astype(np.float64), o["w"].astype(np.float64)
    if form == "f16":
        x, w = H2.half(x), H2.half(w)
    conv, A = plain_conv(case, x, w), plain_conv(case, np.abs(x), np.abs(w))
    D = np.zeros_like(A)
    if form == "b3":
        D = 2.0 ** -21 * A
    elif form == "h2":
        s = H2.range_scale(H2.float_bits(np.abs(o["x"]).max()))
        model = H2.conv(o["x"], o["w"], s, lambda a, b: plain_conv(case, a, b), cout_axis=1 if case.mode == "deconv2x" else 0)
        D = np.abs(model - conv)
    return conv, A, D


def form_of(case):
    """which arithmetic the case's kernel runs: "" fp32 products, "b3" / "h2" split operands, "f16" half operands"""
    if case.f16:
        return "f16"
    if case.tile in (41, 42, 43, 51) or (case.tile is not None and 70 <= case.tile <= 81):
        return "b3" if case.tile in (70, 71, 72, 73, 74, 75) else case.split
    return ""


def act64(v, act):
    return np.maximum(v, 0.0) if act == 1 else np.where(v > 0, v, v * np.float64(np.float32(SLOPE))) if act == 2 else v


def finish64(case, conv):
    """y of a case in float64 from ANY contraction `conv` (N, Cout, Ho, Wo): scale, shift, residual and activation of the case"""
    o = operands(case)
    scale, shift, _, _ = epilogue_constants(case, o)
    bc = lambda a: a.astype(np.float64)[None, :, None, None]
    res = o["res"].astype(np.float64) if "res" in case.epi else 0.0
    return act64(conv * bc(scale) + bc(shift) + res, case.act)


class Ref(object):
    pass


@functools.lru_cache(maxsize=None)
def _reference(key, form, epi, act):
    case = _case_of(key, epi="+".join(epi), act=act)
    o = _operands(key)
    conv, A, D = _core(key, form)
    scale, shift, s2, b2 = epilogue_constants(case, o)
    bc = lambda a: a.astype(np.float64)[None, :, None, None]
    res = o["res"].astype(np.float64) if "res" in case.epi else np.zeros_like(conv)
    r = Ref()
    r.A, r.K = A, case.K
    r.v = conv * bc(scale) + bc(shift) + res
    r.y = finish64(case, conv)
    r.bound = ((case.K + 8) * U * A + D) * np.abs(bc(scale)) + 2 * U * (np.abs(bc(shift)) + np.abs(res) + np.abs(r.v))
    r.y2 = r.bound2 = None
    if s2 is not None:
        r.y2 = np.maximum(r.y * bc(s2) + bc(b2), 0.0)
        r.bound2 = np.abs(bc(s2)) * r.bound + 2 * U * np.abs(r.y2)
    return r


def reference(case):
    """Ref of a case: v, y, y2 (None without a dual output), bound, bound2, A, K -- float64, (N, Cout, Ho, Wo); shared, do not write"""
    return _reference(case.data_key, form_of(case), tuple(sorted(case.epi)), case.act)


def bar(case, ref):
    """the bar of the suite for the case's kernel at this size relative to max|ref| (None: K > 576, no bar), as a function of max|ref|"""
    if case.wino:
        rel = 3e-6 if case.K <= 576 else max(3e-6, 4 * wino32_error(case))
        return lambda m: rel * m
    if case.K > 576:
        return None
    if case.f16:
        return lambda m: 1e-5 * max(1.0, m)
    return lambda m: 1e-6 * m


def check(case, got, got2, what=""):
    """Hold y (and y2) -- (N, Cout, Ho, Wo) -- to the case's bound and bar; returns the largest error-to-bound ratio (Winograd: to bar)"""
    ref = reference(case)
    worst = 0.0
    for name, g, want, bound in (("y", got, ref.y, ref.bound), ("y2", got2, ref.y2, ref.bound2)):
        if want is None:
            continue
        assert g.shape == want.shape, (case.id, name, g.shape, want.shape)
        assert np.isfinite(g).all(), (case.id, name, "not finite")
        err = np.abs(g.astype(np.float64) - want)
        b = bar(case, ref)
        m = float(np.abs(want).max())
        if b is not None:
            ratio_bar = float(err.max()) / b(m)
            if case.wino:
                worst = max(worst, ratio_bar)
            assert ratio_bar <= 1.0, "%s %s%s: max error %.3g above the bar %.3g" % (case.id, name, what, err.max(), b(m))
        if not case.wino:
            ratio = err / bound
            worst = max(worst, float(ratio.max()))
            at = np.unravel_index(np.argmax(ratio), ratio.shape)
            assert ratio.max() <= 1.0, "%s %s%s: error %.3g at %s is %.3f of its bound" % (case.id, name, what, err[at], at, ratio.max())
    return worst


# ---- Winograd F(2x2, 3x3) in fp32 ---------------------------------------------------------------------------------------------------
def wino32(x, w):
    """fp32 restatement of the Winograd kernels: U = G g G^T in double rounded once to fp32 (conv_wino_pack), V = B^T d B, the products
    summed over the channels and Y = A^T m A in fp32.  x (N, C, H, W) with even H, W (pad 1), w (K, C, 3, 3) -> (N, K, H, W) fp32"""
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
    Bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float32)
    At = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float32)
    N, C, H, W = x.shape
    Uw = np.einsum('ia,kcab,jb->kcij', G, w.astype(np.float64), G).astype(np.float32)
    xp = np.zeros((N, C, H + 2, W + 2), np.float32); xp[:, :, 1:-1, 1:-1] = x
    d = np.stack([np.stack([xp[:, :, i:i + H:2, j:j + W:2] for j in range(4)], -1) for i in range(4)], -2)      # (N, C, H/2, W/2, 4, 4)
    V = np.einsum('ia,nctuab->nctuib', Bt, d)
    V = np.einsum('nctuib,jb->nctuij', V, Bt)
    M = np.zeros((N, w.shape[0], H // 2, W // 2, 4, 4), np.float32)
    for c in range(C):      # channel by channel: every product and every sum rounded to fp32
        M += Uw[None, :, c, None, None] * V[:, None, c]
    Y = np.einsum('ia,nktuab->nktuib', At, M)
    Y = np.einsum('nktuib,jb->nktuij', Y, At)
    return np.ascontiguousarray(Y.transpose(0, 1, 2, 4, 3, 5)).reshape(N, w.shape[0], H, W)


@functools.lru_cache(maxsize=None)
def _wino32_error(key):
    o = _operands(key)
    conv = _core(key, "")[0]
    return float(np.abs(wino32(o["x"], o["w"]) - conv).max() / np.abs(conv).max())


def wino32_error(case):
    """largest error of wino32 on the case's inputs, relative to the largest |output|"""
    return _wino32_error(case.data_key)
