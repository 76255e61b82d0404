"""Every input the interpolated-label tests feed the GPU (test_interp_labels_gpu.py), generated here so that the host side
(test_interp_labels_cpu.py) can state the condition under which the GPU tests may demand EQUALITY of every label: no pixel of the float64
reference has its two best interpolated values closer than GUARD x the largest |score| of the case -- apart from the dyadic cases, whose
arithmetic is exact (ties included) and whose answers come from an integer restatement.

A case is a plain tuple; `scores(case)` builds its tensor (deterministic), `reference(case)` is utils.image.labels_interpolated_host of it,
computed once per process and shared (read-only) by the tests that need it."""
import collections
import functools

import numpy as np

from accel_amd.utils import image

from confidence_ref import CROPS, geo
from test_frames_u8_gpu import SMALL

GUARD = 1e-12
NCLS = (19, 2, 21)
SCALES = (1e-3, 1.0, 30.0, 1e4)
POISON = np.float32(1e30)          # class 0 of every padded map pixel: a tap that strays into the padding changes labels

# kind: "normal" (standard normal * scale), "near" (class 11 one fp32 ulp above class 5 in frame 0, one below in frame 1, both above the
# rest), or a dyadic known answer: "ints" (integers in -8 .. 8: ties everywhere), "step" (the step edge of two classes)
Case = collections.namedtuple("Case", "kind n ncls H W out_h out_w h w scale seed")


def small_case(rows, cols, target, max_size, ncls, n, scale, kind="normal"):
    out_h, out_w, H, W = geo(rows, cols, target, max_size)
    seed = (rows * 4096 + cols) * 64 + ncls * 2 + n + int(1000 * np.log10(scale) + 5000) * 100019
    return Case(kind, n, ncls, H, W, out_h, out_w, rows, cols, scale, seed)


def operator_cases(rows, cols, target, max_size, ncls, n):
    """one geometry, class count and batch at the four scales"""
    return [small_case(rows, cols, target, max_size, ncls, n, s) for s in SCALES]


def all_operator_cases():
    return [c for g in SMALL for ncls in NCLS for n in (1, 3) for c in operator_cases(*g, ncls=ncls, n=n)]


# down (a 48 x 89 region to 45 x 83), up (48 x 96 to 60 x 120), portrait (64 x 48 to 100 x 75)
NEAR_GEOMETRIES = [SMALL[2], SMALL[5], SMALL[7]]


def near_tie_cases():
    """the cases that pin the float64 blend: known answer 11 everywhere in frame 0, 5 everywhere in frame 1"""
    return [small_case(*g, ncls=19, n=2, scale=1.0, kind="near") for g in NEAR_GEOMETRIES]


DYADIC_SOURCES = (16, 32, 4)       # of an 8 x 8 region: 2x up, 4x up, 2x down -- every weight is a multiple of 1/8


def dyadic_cases():
    out = []
    for s in DYADIC_SOURCES:
        out.append(Case("step", 1, 2, 16, 16, 8, 8, s, s, 1.0, s))
        for ncls in NCLS:
            out.append(Case("ints", 2, ncls, 16, 16, 8, 8, s, s, 1.0, 100 * ncls + s))
    return out


def crop_case(rows, cols):
    """the identity geometry with a valid region narrower than the map"""
    H, W = (rows + 15) // 16 * 16, (cols + 15) // 16 * 16
    return Case("normal", 2, 19, H, W, rows, cols, rows, cols, 1.0, 177 + cols)


def crop_cases():
    return [crop_case(r, c) for r, c in CROPS]


def multiblock_cases():
    """more than one block per frame, through the general and the identity path"""
    return [Case("normal", 2, 19, 256, 512, 250, 512, 200, 333, 1.0, 702), Case("normal", 2, 19, 256, 512, 256, 512, 256, 512, 1.0, 701)]


def full_case():
    """a 720p camera against its bound size: a 1024 x 1820 region padded to 1024 x 1824"""
    out_h, out_w, H, W = geo(720, 1280, 1024, 2048)
    return Case("normal", 1, 19, H, W, out_h, out_w, 720, 1280, 1.0, 720)


def pitched_cases():
    """identity (the dword path where the pitch allows), padded columns, up"""
    return [small_case(*SMALL[i], ncls=19, n=2, scale=1.0) for i in (0, 2, 5)]


def guarded_cases():
    """every case whose labels rest on float64 rounding: all but the dyadic ones"""
    return all_operator_cases() + near_tie_cases() + crop_cases() + multiblock_cases() + [full_case()] + pitched_cases()


def ident(case):
    return "%s-n%d-ncls%d-%dx%d-of-%dx%d-to-%dx%d-s%g" % (case.kind, case.n, case.ncls, case.H, case.W, case.out_h, case.out_w, case.h, case.w, case.scale)


def scores(case):
    """the n x ncls x H x W fp32 tensor of a case"""
    rng = np.random.default_rng(case.seed)
    shape = (case.n, case.ncls, case.H, case.W)
    if case.kind == "normal":
        s = (rng.standard_normal(shape, dtype=np.float32) * np.float32(case.scale)).astype(np.float32)
    elif case.kind == "near":
        s = (rng.standard_normal(shape) * (0.5 * case.scale)).astype(np.float32)                     # |.| < 3 x scale: below class 5
        top = (4.0 * case.scale * (1.0 + np.abs(rng.standard_normal((case.H, case.W))))).astype(np.float32)
        s[:, 5] = top
        s[0, 11] = np.nextafter(top, np.float32(np.inf))
        s[1:, 11] = np.nextafter(top, np.float32(-np.inf))
    elif case.kind == "ints":
        s = rng.integers(-8, 9, shape).astype(np.float32)
    elif case.kind == "step":
        s = np.zeros(shape, np.float32)
        s[:, 0, :, :5] = 4.0
        s[:, 1] = 1.0
    else:
        raise ValueError(case.kind)
    s[:, 0, case.out_h:, :] = POISON
    s[:, 0, :, case.out_w:] = POISON
    return s


def values(case):
    """the interpolated values of every class, float64 n x ncls x h x w: the arithmetic of image.labels_interpolated_host, kept"""
    s = scores(case)[:, :, :case.out_h, :case.out_w].astype(np.float64)
    y0, y1, fy = image.interpolation_taps(case.h, case.out_h)
    x0, x1, fx = image.interpolation_taps(case.w, case.out_w)
    fy, fx = fy[:, None], fx[None, :]
    r0, r1 = s[:, :, y0], s[:, :, y1]
    top = r0[..., x0] * (1 - fx) + r0[..., x1] * fx
    bot = r1[..., x0] * (1 - fx) + r1[..., x1] * fx
    return top * (1 - fy) + bot * fy


@functools.lru_cache(maxsize=None)
def reference(case):
    """labels n x h x w uint8 of utils.image.labels_interpolated_host: computed once, handed out read-only"""
    out = image.labels_interpolated_host(scores(case), case.out_h, case.out_w, case.h, case.w)
    out.setflags(write=False)
    return out


def integer_labels(case):
    """The dyadic cases restated in integers: with nx = num_x - 2 w x0 (the numerator of fx) and ny alike, 4 h w v_k =
    (a00 (2w - nx) + a01 nx) (2h - ny) + (a10 (2w - nx) + a11 nx) ny exactly; the label is the first maximum.  Shares no code with
    image.interpolation_taps."""
    s = scores(case)[:, :, :case.out_h, :case.out_w]
    a = s.astype(np.int64)
    assert np.array_equal(a.astype(np.float32), s)
    out = np.zeros((case.n, case.h, case.w), np.uint8)
    for y in range(case.h):
        ny = min(max((2 * y + 1) * case.out_h - case.h, 0), 2 * case.h * (case.out_h - 1))
        y0 = ny // (2 * case.h)
        ny -= 2 * case.h * y0
        y1 = min(y0 + 1, case.out_h - 1)
        for x in range(case.w):
            nx = min(max((2 * x + 1) * case.out_w - case.w, 0), 2 * case.w * (case.out_w - 1))
            x0 = nx // (2 * case.w)
            nx -= 2 * case.w * x0
            x1 = min(x0 + 1, case.out_w - 1)
            top = a[:, :, y0, x0] * (2 * case.w - nx) + a[:, :, y0, x1] * nx
            bot = a[:, :, y1, x0] * (2 * case.w - nx) + a[:, :, y1, x1] * nx
            v = top * (2 * case.h - ny) + bot * ny                       # n x ncls
            out[:, y, x] = np.argmax(v, axis=1)                          # the first maximum
    return out
