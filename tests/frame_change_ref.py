"""The cases of the frame-change tests and what accel_amd/utils/image.py frame_signature_host / frame_change_host -- the specification the kernel is
held to -- say about them.  Shared by test_frame_change_cpu.py (the specification against a scalar restatement, and the power of this table to tell
wrong kernels from the right one) and test_frame_change_gpu.py (the kernel against the specification, bit for bit)."""
import collections
import functools

import numpy as np

from accel_amd.utils import image

Shape = collections.namedtuple("Shape", "n H W out_h out_w cell")
Case = collections.namedtuple("Case", "shape values level_q")

# the smallest shapes at which the kernel can go wrong
SHAPES = (
    Shape(1, 16, 16, 16, 16, 8),          # whole cells only
    Shape(3, 48, 80, 37, 70, 16),         # ragged in both axes; the padding holds NaN and 3e38: a read or a count outside the valid region shows
    Shape(2, 40, 50, 40, 50, 8),          # W % 4 != 0: the scalar path
    Shape(1, 64, 132, 64, 129, 64),       # the largest cell; a last column of cells one pixel wide
    Shape(2, 8, 200, 5, 200, 32),         # the region is lower than a cell
    Shape(1, 32, 4112, 32, 4100, 16),     # a row wider than one block's reach
    Shape(8, 32, 64, 32, 64, 32),         # the frame index
)
VALUES = ("uniform", "ties", "extremes", "max", "dyadic")
DYADIC_LEVEL_Q = 192                      # 3 grey levels: the level of the pairs made to sit on the threshold


def level_q_of(shape, values):
    """dyadic: the level the pair was made for; random pairs: about 0.7 standard deviations of a cell's difference, so that both outcomes occur"""
    return DYADIC_LEVEL_Q if values == "dyadic" else 3600 // shape.cell


CASES = tuple(Case(s, v, level_q_of(s, v)) for s in SHAPES for v in VALUES if v != "max" or s.cell == 64)


def case_id(case):
    s = case.shape
    return "%dx%dx%d-%dx%d-c%d-%s" % (s.n, s.H, s.W, s.out_h, s.out_w, s.cell, case.values)


def _seed(case, salt):
    s = case.shape
    return [s.n, s.H, s.W, s.out_h, s.out_w, s.cell, VALUES.index(case.values), salt]


def _pad(x, shape):
    """what lies outside the valid region is never looked at: two NaN for every 3e38 (-4096 and +4096 if they were read: they would not cancel)"""
    fill = np.where((np.arange(shape.H)[:, None] + np.arange(shape.W)[None, :]) % 3 == 0, np.float32(3e38), np.float32(np.nan)).astype(np.float32)
    out = np.broadcast_to(fill, x.shape).copy()
    out[:, :, :shape.out_h, :shape.out_w] = x[:, :, :shape.out_h, :shape.out_w]
    return out


def _draw(case, salt):
    s = case.shape
    rng = np.random.default_rng(_seed(case, salt))
    size = (s.n, 3, s.H, s.W)
    if case.values == "uniform":
        x = rng.uniform(-130.0, 160.0, size).astype(np.float32)
    elif case.values == "ties":            # (k + 0.5) / 8 of both signs: q is a tie, rounded to even
        x = ((rng.integers(-1100, 1100, size).astype(np.float64) + 0.5) / 8.0).astype(np.float32)
    elif case.values == "extremes":
        pool = np.array([600.0, -600.0, np.inf, -np.inf, np.nan, 3e38, -3e38, 512.0, -512.0, 511.9375, 17.25, -3.0], np.float32)
        x = pool[rng.integers(0, len(pool), size)]
    elif case.values == "max":             # the largest |S|: every value at the clamp (the key frame at the other one)
        x = np.full(size, 512.0 if salt == 0 else -512.0, np.float32)
    else:
        raise AssertionError(case.values)
    return x


@functools.lru_cache(maxsize=None)
def frames(case):
    """(current, key): two image inputs n x 3 x H x W fp32 of the case, read-only"""
    s = case.shape
    if case.values != "dyadic":
        cur, key = _draw(case, 0), _draw(case, 1)
    else:
        # multiples of 1/8, so every q is the value times 8: cell (cy, cx) of the current frame differs from the key frame by exactly
        # level_q * area (cy + cx = 0 mod 3: NOT changed), by one unit more (1 mod 3: changed), or not at all (2 mod 3)
        rng = np.random.default_rng(_seed(case, 0))
        q = rng.integers(-800, 800, (s.n, 3, s.H, s.W))
        qc = q.copy()
        gh, gw = image.frame_cells(s.out_h, s.out_w, s.cell)
        for f in range(s.n):
            for cy in range(gh):
                for cx in range(gw):
                    kind = (cy + cx + f) % 3
                    if kind == 2:
                        continue
                    y0, x0 = cy * s.cell, cx * s.cell
                    y1, x1 = min(y0 + s.cell, s.out_h), min(x0 + s.cell, s.out_w)
                    sign = -1 if (cy + 2 * cx) % 2 else 1
                    qc[f, 2, y0:y1, x0:x1] += sign * DYADIC_LEVEL_Q          # the B plane has weight 1
                    if kind == 1:
                        qc[f, 2, y1 - 1, x1 - 1] += sign
        cur, key = (qc / 8.0).astype(np.float32), (q / 8.0).astype(np.float32)
    cur, key = _pad(cur, s), _pad(key, s)
    cur.setflags(write=False)
    key.setflags(write=False)
    return cur, key


Expected = collections.namedtuple("Expected", "sig sig_key changed sad mask")


@functools.lru_cache(maxsize=None)
def expected(case):
    """what the specification says of the case: computed once, shared, read-only"""
    s = case.shape
    cur, key = frames(case)
    sig = image.frame_signature_host(cur, s.out_h, s.out_w, s.cell)
    sig_key = image.frame_signature_host(key, s.out_h, s.out_w, s.cell)
    changed, sad, mask = image.frame_change_host(sig, sig_key, s.out_h, s.out_w, s.cell, case.level_q)
    for a in (sig, sig_key, changed, sad, mask):
        a.setflags(write=False)
    return Expected(sig, sig_key, changed, sad, mask)
