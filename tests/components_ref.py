"""The cases of the connected-component tests and what accel_amd/utils/image.py labels_components_host -- the specification the kernels are held to --
says about them.  Shared by test_labels_components_cpu.py (the specification against a scalar flood fill and scipy, the coverage of this table and its
power to tell wrong kernels from the right one) and test_labels_components_gpu.py (the kernels against the specification, bit for bit)."""
import collections
import functools

import numpy as np

from accel_amd.utils import image

Shape = collections.namedtuple("Shape", "n H W out_h out_w h w ncls")
# trunc: the case is BUILT to have more components than records; every other case has count <= max_components in every frame
Case = collections.namedtuple("Case", "shape pattern connectivity min_area max_components trunc")

# small, and larger than any plausible tile in both directions: 150 x 300 stays ragged against every tile up to 64 x 128
IDENT = Shape(1, 150, 300, 150, 300, 150, 300, 19)          # whole, identity
CROP = Shape(2, 160, 320, 150, 300, 150, 300, 19)           # a crop; the padding holds valid ids: a read outside the region shows
LARGER = Shape(1, 70, 110, 67, 101, 150, 301, 19)           # enlarged by non-integer ratios; w % 4 != 0
SMALLER = Shape(1, 200, 400, 190, 390, 100, 203, 21)        # reduced: rows and columns of the map are dropped
ROW = Shape(1, 32, 4112, 32, 4100, 32, 4100, 19)            # a row wider than one block's reach
BATCH = Shape(8, 72, 136, 72, 136, 72, 136, 32)             # the SAME picture in every frame: a join across frames shows; the largest ncls
SHAPES = (IDENT, CROP, LARGER, SMALLER, ROW, BATCH)
WIDE = Shape(1, 16, 32768, 16, 32768, 16, 32768, 2)         # all one class: sum_x = 8 589 672 448 > 2^32
TALL = Shape(1, 8, 16, 8, 16, 32768, 16, 1)                 # the same value for sum_y, at the largest enlargement

EVERYWHERE = ("uniform", "runs", "comb")                    # the patterns every shape is given
PICTURES = ("serpentine", "serpentine_cut", "spiral", "checker", "diagonals", "one", "background", "interleaved", "sizes")
PATTERNS = EVERYWHERE + PICTURES
MANY = ("uniform", "checker", "diagonals")                  # patterns with thousands of components: records for all of them
SIZE = 7                                                    # `sizes`: objects of SIZE - 1, SIZE and SIZE + 1 pixels


def _records(shape, pattern):
    if pattern in MANY and shape is not ROW:
        return 65536
    if pattern == "comb" and shape is ROW:                  # a thousand teeth
        return 4096
    return 1024


def _cases():
    out = []
    for conn in (4, 8):
        for s in SHAPES:
            for p in EVERYWHERE:
                out.append(Case(s, p, conn, 1, _records(s, p), s is ROW and p == "uniform"))
        for s in (IDENT, LARGER, BATCH):
            for p in PICTURES:
                if p == "sizes" and s is LARGER:            # its objects are sized in source pixels: the identity geometry only
                    continue
                out.append(Case(s, p, conn, 1, _records(s, p), False))
        for s in (WIDE, TALL):
            out.append(Case(s, "one", conn, 1, 1024, False))
        # the subset with other parameters: min_area at the sizes of `sizes`, a filter on ordinary maps, records below and just above the count
        out.append(Case(IDENT, "sizes", conn, SIZE, 1024, False))
        out.append(Case(BATCH, "sizes", conn, SIZE + 1, 1024, False))
        out.append(Case(CROP, "uniform", conn, 3, 65536, False))
        out.append(Case(LARGER, "runs", conn, 50, 1024, False))
        out.append(Case(IDENT, "checker", conn, 1, 1024, conn == 4))
        out.append(Case(IDENT, "uniform", conn, 1, 7, True))
        out.append(Case(BATCH, "comb", conn, 1, 3, True))
        out.append(Case(SMALLER, "comb", conn, 2, 1, True))
    return tuple(out)


CASES = _cases()
# the cases whose ids are also asked for at a padded pitch (test_labels_components_gpu.py)
PITCHED = tuple(c for c in CASES if c.shape in (LARGER, CROP) and c.pattern in ("runs", "comb") and c.min_area == 1)


def case_id(case):
    return "%s-%s-c%d-a%d-m%d" % ("x".join(str(v) for v in case.shape), case.pattern, case.connectivity, case.min_area, case.max_components)


def _spiral(oh, ow, k):
    """a one-pixel spiral of class k on background, arms one background pixel apart"""
    a = np.full((oh, ow), 255, np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    a[0, 0] = k
    for _ in range(oh * ow):                                # every step marks a pixel or turns; two turns in a row end it
        turned = 0
        while turned < 2:
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            free = 0 <= ny < oh and 0 <= nx < ow and a[ny, nx] == 255 and not (0 <= ay < oh and 0 <= ax < ow and a[ay, ax] != 255)
            if free:
                break
            dy, dx = dx, -dy
            turned += 1
        if turned == 2:
            break
        y, x = y + dy, x + dx
        a[y, x] = k
    return a


def _picture(rng, s, pattern):
    """one frame of the valid region, out_h x out_w uint8"""
    oh, ow, ncls = s.out_h, s.out_w, s.ncls
    yy, xx = np.mgrid[0:oh, 0:ow]
    a = np.full((oh, ow), 255, np.uint8)
    if pattern == "uniform":                # random ids, a quarter of them background, 255 among them
        a = rng.integers(0, ncls, (oh, ow), dtype=np.uint8)
        pick = rng.random((oh, ow)) < 0.25
        a[pick] = rng.integers(ncls, 256, int(pick.sum()), dtype=np.uint8)
        a[oh // 2, ow // 2] = 255
    elif pattern == "runs":                 # long runs with rectangles on top, a few of them background
        lengths = rng.integers(1, 2 * ow + 2, oh * ow // 64 + 8)
        a = np.repeat(rng.integers(0, ncls + 2, lengths.size, dtype=np.uint8), lengths)[:oh * ow].reshape(oh, ow).copy()
        for _ in range(4):
            y0, x0 = int(rng.integers(0, oh)), int(rng.integers(0, ow))
            a[y0:y0 + int(rng.integers(1, oh + 1)), x0:x0 + int(rng.integers(1, ow + 1))] = rng.integers(0, ncls + 1)
        a[a >= ncls] = 255
    elif pattern in ("serpentine", "serpentine_cut"):
        # full even rows joined alternately at the right and the left end: one component, a chain as long as the map; the twin is cut in two
        a[0::2] = 1
        a[1::4, ow - 1] = 1
        a[3::4, 0] = 1
        if pattern == "serpentine_cut":
            a[(oh // 2) & ~1, ow // 2] = 255
    elif pattern == "spiral":
        a = _spiral(oh, ow, 2)
    elif pattern == "comb":
        # teeth of class 2 in every fourth column that join only in the LAST row: the anchor is in the first tile, the join in the last one; and
        # between them U shapes of class 3 that close three rows above the bottom and cut the teeth they cross
        a[:, 0::4] = 2
        a[oh - 1, :] = 2
        if oh > 6:
            a[1:oh - 3, 2::4] = 3
            a[oh - 3, (xx[0] % 8 >= 2) & (xx[0] % 8 <= 6)] = 3
    elif pattern == "checker":              # every pixel a component under 4, two components under 8
        a = ((yy + xx) % 2).astype(np.uint8)
    elif pattern == "diagonals":            # many components under 4, one per line under 8: both diagonal directions
        left = xx < ow // 2
        a[left & ((xx - yy) % 5 == 0)] = 4 % ncls
        a[~left & ((xx + yy) % 5 == 0)] = 5 % ncls
    elif pattern == "one":
        a[...] = ncls - 1
    elif pattern == "background":           # nothing to find: ids >= ncls only
        a[0::3] = ncls
    elif pattern == "interleaved":          # blocks of 10 x 9 of two classes: equal-shaped neighbours of different classes must not join
        a = ((xx // 9 + yy // 10) % 2).astype(np.uint8)
    elif pattern == "sizes":                # bars of SIZE - 1, SIZE and SIZE + 1 pixels, three rows apart
        for i, y in enumerate(range(1, oh - 1, 3)):
            length = SIZE - 1 + i % 3
            x0 = (i * 11) % max(1, ow - length - 1)
            a[y, x0:x0 + length] = i % ncls
            a[y, min(ow - 1, x0 + length + 1):min(ow, x0 + length + 3)] = (i + 1) % ncls       # a shorter neighbour of another class
    else:
        raise AssertionError(pattern)
    return a


@functools.lru_cache(maxsize=None)
def labels(shape, pattern):
    """the label maps n x H x W of a shape and a pattern, read-only.  What lies outside the valid region holds valid ids"""
    s = shape
    rng = np.random.default_rng(list(s) + [PATTERNS.index(pattern)])
    pad = rng.integers(0, s.ncls, (s.n, s.H, s.W), dtype=np.uint8)
    for f in range(s.n):
        if f == 0 or s is not BATCH:
            pic = _picture(rng, s, pattern)
        pad[f, :s.out_h, :s.out_w] = pic
    pad.setflags(write=False)
    return pad


Expected = collections.namedtuple("Expected", "count comp sums ids")


@functools.lru_cache(maxsize=None)
def expected(case):
    """what the specification says of the case: computed once, shared, read-only"""
    s = case.shape
    out = image.labels_components_host(labels(s, case.pattern), s.out_h, s.out_w, s.h, s.w, s.ncls, connectivity=case.connectivity,
                                       min_area=case.min_area, max_components=case.max_components, ids=True)
    for a in out:
        a.setflags(write=False)
    return Expected(*out)
