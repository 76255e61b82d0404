"""The cases of the label-summary tests and what accel_amd/utils/image.py labels_summary_host -- the specification the kernel is held to -- says about
them.  Shared by test_labels_summary_cpu.py (the specification against a scalar restatement, and the power of this table to tell wrong kernels from
the right one) and test_labels_summary_gpu.py (the kernel against the specification, bit for bit)."""
import collections
import functools

import numpy as np

from accel_amd.utils import image

Shape = collections.namedtuple("Shape", "n H W out_h out_w h w ncls")
Case = collections.namedtuple("Case", "shape values prev")

# the smallest shapes at which the kernel can go wrong
SHAPES = (
    Shape(1, 8, 8, 8, 8, 8, 8, 2),                  # whole, identity
    Shape(3, 48, 80, 37, 70, 37, 70, 19),           # a crop; the padding holds valid ids: a read or a count outside the region shows
    Shape(2, 40, 52, 40, 50, 91, 173, 19),          # enlarged by non-integer ratios; w % 4 != 0
    Shape(2, 64, 128, 60, 121, 23, 47, 21),         # reduced: rows and columns of the map are dropped
    Shape(1, 32, 4112, 32, 4100, 32, 4100, 19),     # a row wider than one block's reach
    Shape(8, 32, 64, 32, 64, 32, 64, 32),           # the frame index; the largest ncls
)
WIDE = Shape(1, 16, 32768, 16, 32768, 16, 32768, 2)       # all one class: sum_x = 8 589 672 448 > 2^32
TALL = Shape(1, 8, 16, 8, 16, 32768, 16, 1)               # the same value for sum_y, at the largest enlargement
VALUES = ("uniform", "runs", "single", "one")
PREVS = ("independent", "equal", "ignored")

CASES = tuple(Case(s, v, p) for s in SHAPES for v in VALUES for p in PREVS) + tuple(Case(s, "one", p) for s in (WIDE, TALL) for p in PREVS)


def case_id(case):
    return "%s-%s-%s" % ("x".join(str(v) for v in case.shape), case.values, case.prev)


def _seed(case, salt):
    return list(case.shape) + [VALUES.index(case.values), salt]


def _some_ignored(rng, a, ncls, share, rows, cols):
    """`share` of the entries of `a` replaced by ids >= ncls, 255 among them (inside the first rows x cols of every map)"""
    pick = rng.random(a.shape) < share
    a[pick] = rng.integers(ncls, 256, int(pick.sum()), dtype=np.uint8)
    a[:, rows // 2, cols // 2] = 255
    return a


@functools.lru_cache(maxsize=None)
def labels(shape, values):
    """the label maps n x H x W of a shape and a value kind, read-only.  What lies outside the valid region holds valid ids"""
    s = shape
    rng = np.random.default_rng(_seed(Case(s, values, PREVS[0]), 0))
    size = (s.n, s.H, s.W)
    if values == "uniform":                 # random ids, a quarter of them >= ncls, 255 among them
        a = _some_ignored(rng, rng.integers(0, s.ncls, size, dtype=np.uint8), s.ncls, 0.25, s.out_h, s.out_w)
    elif values == "runs":                  # long runs, and rectangles on top of them: valid ids only
        lengths = rng.integers(1, 4097, s.n * s.H * s.W // 512 + 8)
        a = np.repeat(rng.integers(0, s.ncls, lengths.size, dtype=np.uint8), lengths)[:s.n * s.H * s.W].reshape(size).copy()
        for f in range(s.n):
            for _ in range(3):
                y0, x0 = int(rng.integers(0, s.out_h)), int(rng.integers(0, s.out_w))
                a[f, y0:y0 + int(rng.integers(1, s.out_h + 1)), x0:x0 + int(rng.integers(1, s.out_w + 1))] = rng.integers(0, s.ncls)
    elif values == "single":
        # the even classes at one map pixel each -- class 0 where source pixel (0, 0) looks, the largest even class where (h - 1, w - 1) looks --
        # every odd class absent, everything else ignored (255)
        a = np.full(size, 255, np.uint8)
        ys, xs = image.nearest_index(s.h, s.out_h), image.nearest_index(s.w, s.out_w)
        present = list(range(0, s.ncls, 2))
        for f in range(s.n):
            taken = {(0, 0), (int(ys[-1]), int(xs[-1]))}
            a[f, 0, 0] = 0
            a[f, ys[-1], xs[-1]] = present[-1]
            for k in present[1:-1]:
                while True:
                    at = (int(ys[rng.integers(0, s.h)]), int(xs[rng.integers(0, s.w)]))
                    if at not in taken:
                        break
                taken.add(at)
                a[f][at] = k
    elif values == "one":
        a = np.full(size, s.ncls - 1, np.uint8)
    else:
        raise AssertionError(values)
    pad = rng.integers(0, s.ncls, size, dtype=np.uint8)
    pad[:, :s.out_h, :s.out_w] = a[:, :s.out_h, :s.out_w]
    pad.setflags(write=False)
    return pad


@functools.lru_cache(maxsize=None)
def previous(case):
    """the previous frame's labels at the source size, n x h x w, read-only"""
    s = case.shape
    rng = np.random.default_rng(_seed(case, 1 + PREVS.index(case.prev)))
    if case.prev == "equal":
        p = image.labels_to_source_host(labels(s, case.values), s.out_h, s.out_w, s.h, s.w).copy()
    else:
        p = rng.integers(0, s.ncls, (s.n, s.h, s.w), dtype=np.uint8)
        if case.prev == "ignored":
            p = _some_ignored(rng, p, s.ncls, 0.3, s.h, s.w)
    p.setflags(write=False)
    return p


Expected = collections.namedtuple("Expected", "stats box trans kept")


@functools.lru_cache(maxsize=None)
def expected(case):
    """what the specification says of the case: computed once, shared, read-only"""
    s = case.shape
    out = image.labels_summary_host(labels(s, case.values), s.out_h, s.out_w, s.h, s.w, s.ncls, prev=previous(case))
    for a in out:
        a.setflags(write=False)
    return Expected(*out)
