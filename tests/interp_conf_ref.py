"""Every input the tests of the confidence of interpolated scores feed the GPU (test_interp_conf_gpu.py), generated here so that the host side
(test_interp_conf_cpu.py) can state the conditions under which the GPU tests may demand EQUALITY of all five outputs.  The blend is specified
bit for bit, so of the whole computation only the device's exp can differ from the host's:
  (a) no pixel of the float64 reference has 256 * p within confidence_ref.GUARD = 1e-9 of an integer, unless its byte cannot depend on an exp
      (the exactness rule of confidence_ref.scaled_float64, applied to the interpolated values v_k);
  (b) and, should a blend ever be reordered, neither the two best nor the second and the third best v_k of a pixel are closer than
      interp_ref.GUARD = 1e-12 x the largest |score| of the case: a last bit cannot move `labels` or `second`.
The dyadic cases and the known answers are exempt from (b): their arithmetic is exact or runs on identical planes, ties included.

A case is interp_ref's plain tuple.  The operator, near-tie, dyadic, crop, multi-block, pitched and 720p cases ARE interp_ref's (the same
tensors, POISON in class 0 of the padding); this file adds stored probabilities ("prob": is_prob) and the known answers of confidence_ref
("equal", "one100", "tie2") on resampled geometries.  `scores(case)` builds a tensor (deterministic), `reference(case)` is
utils.image.confidence_interpolated_host of it, computed once per process and shared (read-only) by the tests that need it."""
import functools

import numpy as np

from accel_amd.utils import image

import confidence_ref as cref
import interp_ref as iref
from interp_ref import Case, GUARD, NCLS, POISON, SCALES, ident          # noqa: F401  (the vocabulary of the tests)
from test_frames_u8_gpu import SMALL

CONF_GUARD = cref.GUARD
KNOWN = cref.KNOWN
# a 29 x 50 source of a 31 x 54 region (down; confidence_ref's second geometry) and a 45 x 80 source of it (up), both of a 32 x 64 map
KNOWN_SOURCES = ((29, 50), (45, 80))

operator_cases = iref.operator_cases
all_operator_cases = iref.all_operator_cases
near_tie_cases = iref.near_tie_cases
dyadic_cases = iref.dyadic_cases
crop_cases = iref.crop_cases
multiblock_cases = iref.multiblock_cases
pitched_cases = iref.pitched_cases
full_case = iref.full_case
small_case = iref.small_case


def prob_cases():
    """probabilities stored as fp32, as confidence_ref.prob_cases: six geometries and class counts at two scales.  The softmax of
    standard-normal scores x 1 and x 4; at confidence_ref's x 30 the runner-up probabilities lie below 1e-12, where condition (b), which is
    stated against the largest stored value (here ~1), cannot hold"""
    out = []
    for (rows, cols, target, max_size), ncls in zip(SMALL[:6], (19, 2, 21, 19, 21, 2)):
        for scale in (1.0, 4.0):
            out.append(small_case(rows, cols, target, max_size, ncls, 2, scale, kind="prob"))
    return out


def known_cases():
    """all scores equal / one class 100 above the rest / a two-way tie at the top, for every class count, down and up"""
    return [Case(kind, 2, ncls, 32, 64, 31, 54, h, w, 1.0, ncls + h) for kind in KNOWN for ncls in NCLS for h, w in KNOWN_SOURCES]


known_winner = cref.known_winner
known_tie = cref.known_tie


def exempt(case):
    """exact by construction, ties included: condition (b) does not apply"""
    return case.kind in ("ints", "step") + KNOWN


def guarded_cases():
    """every case the GPU tests use whose outputs rest on float64 rounding"""
    return iref.guarded_cases() + prob_cases()


def all_cases():
    return guarded_cases() + dyadic_cases() + known_cases()


def is_prob(case):
    return case.kind == "prob"


def scores(case):
    """the n x ncls x H x W fp32 tensor of a case; class 0 of every padded map pixel is POISON"""
    if case.kind in ("normal", "near", "ints", "step"):
        return iref.scores(case)
    s = cref.scores(case)                   # "prob" and the known answers: confidence_ref's construction
    s[:, 0, case.out_h:, :] = POISON
    s[:, 0, :, case.out_w:] = POISON
    return s


def values(case):
    """the interpolated values of every class, float64 n x ncls x h x w: interp_ref.values (the arithmetic of
    image.labels_interpolated_host, kept) for any kind of case"""
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
    """(labels, conf, margin, second, hist) of utils.image.confidence_interpolated_host: computed once, handed out read-only"""
    out = image.confidence_interpolated_host(scores(case), case.out_h, case.out_w, case.h, case.w, is_prob=is_prob(case))
    for a in out:
        a.setflags(write=False)
    return out


def scaled_float64(case):
    """confidence_ref.scaled_float64 on the interpolated values: (256 * p of every SOURCE pixel in float64, mask of the pixels whose byte no
    exp can move): every difference v_k - v_best is 0 or below -800 (exp gives exactly 1 or exactly 0), or 256 * p >= 255.5 (saturation).
    For probabilities 256 * v_best is exact everywhere: no exp at all."""
    v = values(case)
    if is_prob(case):
        s = 256.0 * v.max(axis=1)
        return s, np.ones(s.shape, bool)
    d = v - v.max(axis=1, keepdims=True)
    s = 256.0 / np.exp(d).sum(axis=1)
    return s, np.all((d == 0) | (d < -800.0), axis=1) | (s >= 255.5)


def smallest_gaps(case):
    """(the smallest best - second, the smallest second - third (inf for two classes), the largest |score| of the valid region)"""
    v = np.sort(values(case), axis=1)
    third = float((v[:, -2] - v[:, -3]).min()) if case.ncls > 2 else float("inf")
    return float((v[:, -1] - v[:, -2]).min()), third, float(np.abs(scores(case)[:, :, :case.out_h, :case.out_w]).max())
