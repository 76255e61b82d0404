"""Every input the confidence tests feed the GPU (test_confidence_gpu.py), generated here so that the host side (test_confidence_cpu.py) can
state the condition under which the GPU tests may demand EQUALITY of the conf byte: no pixel of the float64 reference has 256 * p within
GUARD of an integer, apart from the pixels whose byte does not depend on the last bits of any exp.

A case is a plain tuple; `scores(case)` builds its tensor (deterministic), `reference(case)` is utils.image.confidence_host of it, computed
once per process and shared (read-only) by the tests that need it."""
import collections
import functools

import numpy as np

from accel_amd.utils import image

from test_frames_u8_gpu import SMALL

STRIDE = 16
GUARD = 1e-9
NCLS = (19, 2, 21)
SCALES = (1e-3, 1.0, 30.0, 1e4)
CROPS = [(48, 90), (31, 50), (17, 33), (16, 20)]

# kind: "normal" (standard normal * scale), "prob" (softmax of that, stored as fp32: is_prob), or a known answer
Case = collections.namedtuple("Case", "kind n ncls H W out_h out_w h w scale seed")


def geo(rows, cols, target, max_size, stride=STRIDE):
    """(out_h, out_w, H, W): the valid region and the padded size of the map a rows x cols frame gives"""
    return image.resize_geometry(rows, cols, target, max_size, stride)[1:]


def small_case(rows, cols, target, max_size, ncls, n, scale, kind="normal"):
    out_h, out_w, H, W = geo(rows, cols, target, max_size)
    seed = (rows * 4096 + cols) * 64 + ncls * 2 + n + int(1000 * np.log10(scale) + 5000) * 100003
    return Case(kind, n, ncls, H, W, out_h, out_w, rows, cols, scale, seed)


def operator_cases(rows, cols, target, max_size, ncls, n):
    """test 1: one geometry, class count and batch at the four scales"""
    return [small_case(rows, cols, target, max_size, ncls, n, s) for s in SCALES]


def crop_case(rows, cols):
    """test 4: the identity geometry with a valid region narrower than the map"""
    H, W = (rows + 15) // 16 * 16, (cols + 15) // 16 * 16
    return Case("normal", 2, 19, H, W, rows, cols, rows, cols, 1.0, 77 + cols)


def multiblock_cases():
    """test 6: more than one block per frame, through the vector and the scalar path"""
    return [Case("normal", 2, 19, 256, 512, 256, 512, 256, 512, 1.0, 601), Case("normal", 2, 19, 256, 512, 250, 512, 200, 333, 1.0, 602)]


def prob_cases():
    """test 7: probabilities stored as fp32"""
    out = []
    for (rows, cols, target, max_size), ncls in zip(SMALL[:6], (19, 2, 21, 19, 21, 2)):
        for scale in (1.0, 30.0):
            out.append(small_case(rows, cols, target, max_size, ncls, 2, scale, kind="prob"))
    return out


KNOWN = ("equal", "one100", "tie2")


def known_cases():
    """test 5: all scores equal / one class 100 above the rest / a two-way tie at the top, for every class count and through both paths
    (32 x 64 at identity; a 29 x 50 source of a 31 x 54 region)"""
    out = []
    for kind in KNOWN:
        for ncls in NCLS:
            out.append(Case(kind, 2, ncls, 32, 64, 32, 64, 32, 64, 1.0, ncls))
            out.append(Case(kind, 2, ncls, 32, 64, 31, 54, 29, 50, 1.0, ncls + 1))
    return out


def pitched_cases():
    """tests 2 and 3: the first, third and sixth small geometry (identity, padded columns, down) at scale 1"""
    return [small_case(*SMALL[i], ncls=19, n=2, scale=1.0) for i in (0, 2, 5)]


def all_cases():
    out = []
    for g in SMALL:
        for ncls in NCLS:
            for n in (1, 3):
                out += operator_cases(*g, ncls=ncls, n=n)
    out += [crop_case(r, c) for r, c in CROPS] + multiblock_cases() + prob_cases() + known_cases() + pitched_cases()
    return out


def scores(case):
    """the n x ncls x H x W fp32 tensor of a case"""
    rng = np.random.default_rng(case.seed)
    shape = (case.n, case.ncls, case.H, case.W)
    if case.kind in ("normal", "prob"):
        s = (rng.standard_normal(shape) * case.scale).astype(np.float32)
        if case.kind == "prob":
            d = s.astype(np.float64)
            e = np.exp(d - d.max(axis=1, keepdims=True))
            s = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        return s
    # another level at every pixel, the same for every class: quarters in -8 .. 8, so that adding 3 or 100 in fp32 is exact
    base = (rng.integers(-32, 33, (case.n, 1, case.H, case.W)) / 4.0).astype(np.float32)
    s = np.ascontiguousarray(np.broadcast_to(base, shape))
    if case.kind == "one100":
        s[:, known_winner(case)] += np.float32(100.0)
    elif case.kind == "tie2":
        a, b = known_tie(case)
        s[:, a] += np.float32(3.0)
        s[:, b] += np.float32(3.0)
    return s


def known_winner(case):
    return case.ncls // 2


def known_tie(case):
    """(the earlier, the later index) of the two classes tied at the top"""
    return (0, case.ncls - 1) if case.ncls == 2 else (1, case.ncls - 2)


def is_prob(case):
    return case.kind == "prob"


@functools.lru_cache(maxsize=None)
def reference(case):
    """(conf, margin, second, hist) of utils.image.confidence_host: computed once, handed out read-only"""
    out = image.confidence_host(scores(case), case.out_h, case.out_w, case.h, case.w, is_prob=is_prob(case))
    for a in out:
        a.setflags(write=False)
    return out


def scaled_float64(case):
    """(256 * p of every MAP pixel of the valid region in float64, mask of the pixels whose byte no exp can move): a pixel is exact when
    every difference l_k - l_max is 0 or below -800 (exp gives exactly 1 or exactly 0: p = 1 / m), and the byte is 255 whatever the last
    bits say once 256 * p >= 255.5 (saturation: min(255, .)).  For probabilities 256 * float64(p) is exact everywhere: no rounding at all."""
    s = scores(case)[:, :, :case.out_h, :case.out_w].astype(np.float64)
    if is_prob(case):
        v = 256.0 * s.max(axis=1)
        return v, np.ones(v.shape, bool)
    d = s - s.max(axis=1, keepdims=True)
    v = 256.0 / np.exp(d).sum(axis=1)
    exact = np.all((d == 0) | (d < -800.0), axis=1) | (v >= 255.5)
    return v, exact
