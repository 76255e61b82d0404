"""The cases of the trimap tests and what accel_amd/utils/image.py boundary_distance_host and band_hist_host -- the specification the kernels of
csrc/labels_band.hip are held to -- say about them.  Shared by test_labels_band_cpu.py (the specification against scalar restatements, and the power of
this table to tell wrong kernels from the right one) and test_labels_band_gpu.py (the kernels against the specification, bit for bit)."""
import collections
import functools

import numpy as np

from accel_amd.utils import image

Shape = collections.namedtuple("Shape", "n H W out_h out_w h w ncls widths")
Case = collections.namedtuple("Case", "shape values pred")

# the smallest shapes at which the kernel can go wrong
TINY = (
    Shape(1, 8, 8, 8, 8, 8, 8, 2, (1,)),                             # whole, identity
    Shape(1, 3, 5, 3, 5, 3, 5, 3, (16,)),                            # a frame smaller than the halo
)
SHAPES = TINY + (
    Shape(3, 48, 80, 37, 70, 37, 70, 19, (1, 2, 4, 8)),              # a crop; the padding holds valid ids
    Shape(2, 40, 52, 40, 50, 91, 173, 19, (2, 3, 5, 16)),            # enlarged by non-integer ratios
    Shape(2, 64, 128, 60, 121, 23, 47, 21, (1, 16)),                 # reduced: rows and columns of the map are dropped
    Shape(1, 32, 4112, 32, 4100, 32, 4100, 19, (4, 12)),             # a row wider than one block's reach
    Shape(8, 32, 64, 32, 64, 32, 64, 32, (13, 14, 15, 16)),          # the frame index, the largest tables, adjacent widths
)
LATTICE = Shape(1, 96, 300, 96, 300, 96, 300, 19, (1, 2, 4, 16))     # lone pixels every 37 rows and 41 columns: coprime to any power-of-two tile
VALUES = ("blocks", "blocks+ignored", "flat", "noise")
PREDS = ("independent", "equal", "ignored")
GAP = 13                                                             # the pitched form of a ground truth: rows of w bytes, w + GAP apart

CASES = tuple(Case(s, v, p) for s in SHAPES for v in VALUES for p in PREDS) + tuple(Case(LATTICE, "lattice", p) for p in PREDS)
ALL_SHAPES = SHAPES + (LATTICE,)


def case_id(case):
    s = case.shape
    return "%s-%s-%s-%s" % ("x".join(str(v) for v in s[:8]), ".".join(str(v) for v in s.widths), case.values, case.pred)


def _seed(shape, values, salt):
    return list(shape[:8]) + list(shape.widths) + [len(values), salt]


def maps_of(shape):
    """the ground-truth kinds a shape is tested with"""
    return ("lattice",) if shape == LATTICE else VALUES


@functools.lru_cache(maxsize=None)
def ground_truth(shape, values):
    """the ground-truth maps n x h x w of a shape and a value kind, read-only"""
    s = shape
    rng = np.random.default_rng(_seed(s, values, 0))
    size = (s.n, s.h, s.w)
    if values in ("blocks", "blocks+ignored"):
        # a background class with two or three rectangles per frame.  They stay inside two fifths of the width -- the left ones in even frames, the
        # right ones in odd frames -- so that every frame has pixels further than 16 from any of them, as it has pixels at every smaller distance
        g = np.empty(size, np.uint8)
        reach = max(s.w * 2 // 5, 2)
        for f in range(s.n):
            g[f] = rng.integers(0, s.ncls)
            part = np.zeros((s.h, reach), np.uint8)
            part[...] = g[f, 0, 0]
            for _ in range(int(rng.integers(2, 4))):
                y0, x0 = int(rng.integers(0, s.h)), int(rng.integers(0, reach))
                part[y0:y0 + int(rng.integers(1, s.h // 2 + 2)), x0:x0 + int(rng.integers(1, reach // 2 + 2))] = (g[f, 0, 0] + rng.integers(1, s.ncls)) % s.ncls
            if values == "blocks+ignored":
                y0, x0 = int(rng.integers(0, s.h)), int(rng.integers(0, reach))
                part[y0:y0 + int(rng.integers(1, s.h // 3 + 2)), x0:x0 + int(rng.integers(1, reach // 3 + 2))] = 255
                pick = rng.random(part.shape) < 0.02
                part[pick] = rng.integers(s.ncls, 256, int(pick.sum()), dtype=np.uint8)
            if f % 2:
                g[f, :, s.w - reach:] = part[:, ::-1]
            else:
                g[f, :, :reach] = part
    elif values == "lattice":
        g = np.full(size, 3, np.uint8)
        g[:, ::37, ::41] = 5
    elif values == "flat":
        g = np.full(size, 1 % s.ncls, np.uint8)
    elif values == "noise":
        g = rng.integers(0, s.ncls, size, dtype=np.uint8)
    else:
        raise AssertionError(values)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def ground_truth_pitched(shape, values):
    """the same maps as n x h x (w + GAP) bytes, read-only.  The bytes between the rows differ from the rows' ends: the first ones from the last pixel of
    their row, the last one from the first pixel of the next row.  A kernel that takes the gap for a neighbour then shows"""
    g = ground_truth(shape, values)
    n, h, w = g.shape
    out = np.empty((n, h, w + GAP), np.uint8)
    out[:, :, :w] = g
    out[:, :, w:] = ((g[:, :, -1].astype(np.int64) + 1) % 256).astype(np.uint8)[:, :, None]
    after = np.roll(g.reshape(n * h, w)[:, 0], -1).reshape(n, h)
    out[:, :, -1] = ((after.astype(np.int64) + 1) % 256).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def labels(case):
    """the label maps n x H x W of a case, read-only.  What lies outside the valid region holds valid ids"""
    s = case.shape
    rng = np.random.default_rng(_seed(s, case.values, 1 + PREDS.index(case.pred)))
    size = (s.n, s.H, s.W)
    a = rng.integers(0, s.ncls, size, dtype=np.uint8)
    if case.pred == "equal":
        # the ground truth taken to the map's valid region: equal to it under the nearest rule wherever the map is not enlarged
        g = ground_truth(s, case.values)
        a[:, :s.out_h, :s.out_w] = g[:, image.nearest_index(s.out_h, s.h), :][:, :, image.nearest_index(s.out_w, s.w)]
    elif case.pred == "ignored":
        inside = a[:, :s.out_h, :s.out_w]
        pick = rng.random(inside.shape) < 0.25
        inside[pick] = rng.integers(s.ncls, 256, int(pick.sum()), dtype=np.uint8)
        inside[:, s.out_h // 2, s.out_w // 2] = 255
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def distance(shape, values):
    """what the specification says of a ground truth at cap = the largest width: computed once, shared, read-only"""
    d = image.boundary_distance_host(ground_truth(shape, values), shape.widths[-1])
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(case):
    """the buckets the specification gives for a case, (K + 1) x ncls x ncls uint64: computed once, shared, read-only"""
    s = case.shape
    out = image.band_hist_host(labels(case), s.out_h, s.out_w, ground_truth(s, case.values), s.ncls, s.widths)
    out.setflags(write=False)
    return out
