"""Connected components of finished frames, host side: utils.image.labels_components_host -- the specification csrc/labels_components.hip is held to --
equals a scalar flood fill and scipy.ndimage.label on every case of components_ref; the table covers what it claims to cover and tells a list of
named wrong kernels from the right one; the helpers do what they say; and the C ABI declares and exports the entry points.  (GPU side:
test_labels_components_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

import components_ref as ref

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("accel_labels_components", "accel_model_labels_components", "accel_model_scores_components")


def test_header_declares_and_library_exports_the_entry_points():
    from accel_amd import runtime
    from accel_amd.core import results
    hdr = open(os.path.join(ROOT, "include", "accel_hip.h")).read()
    declared = set(re.findall(r"\b(accel_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, "include/accel_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libaccel_hip.so does not export %s" % name
    runtime.lib()
    assert set(ENTRY_POINTS) <= set(runtime.EXPORTS)
    assert len(runtime.EXPORTS["accel_labels_components"]) == 18
    assert len(runtime.EXPORTS["accel_model_labels_components"]) == 16 and len(runtime.EXPORTS["accel_model_scores_components"]) == 16
    assert hasattr(runtime.Context, "labels_components")
    for name in ("labels_components", "labels_components_device", "scores_components", "scores_components_device"):
        assert hasattr(runtime.Model, name), name
    for name in ("components", "Components", "components_centroids", "components_of"):
        assert hasattr(results, name), name
    assert results.Components._fields == ("count", "comp", "sums", "ids")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


def test_components_of_a_non_handle_is_an_accel_error():
    from accel_amd import runtime
    from accel_amd.core import results
    with pytest.raises(runtime.AccelError, match="not a label handle"):
        results.components(np.zeros((1, 8, 8), np.uint8), None)
    with pytest.raises(runtime.AccelError, match="logits"):
        results.components(np.zeros((1, 19, 8, 8), np.float32), None, interpolate=True)


# ---- a scalar restatement: flood fill from every unseen pixel in raster order, with the flaws of wrong kernels on request --------------------------------
def _flood(L, ncls, conn, flaw=None):
    """the components of one h x w map as [(class, [linear indices, the anchor first])], in anchor order"""
    h, w = L.shape
    lab = L.ravel().tolist()
    seen = bytearray(h * w)
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    if conn == 8:
        steps += [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    kind, arg = flaw if flaw else (None, None)
    comps = []
    for p in range(h * w):
        if seen[p] or lab[p] >= ncls:
            continue
        k = lab[p]
        seen[p] = 1
        stack, pix = [p], []
        while stack:
            q = stack.pop()
            pix.append(q)
            y, x = divmod(q, w)
            for dy, dx in steps:
                ny, nx = y + dy, x + dx
                if not (0 <= ny < h and 0 <= nx < w):
                    continue
                r = ny * w + nx
                if kind == "across background" and lab[r] >= ncls:          # a background pixel between two pixels of the class does not separate
                    ny, nx = ny + dy, nx + dx
                    if not (0 <= ny < h and 0 <= nx < w):
                        continue
                    r = ny * w + nx
                if seen[r] or (lab[r] >= ncls if kind == "across classes" else lab[r] != k):
                    continue
                if kind == "vertical seam" and dx and max(x, nx) % arg == 0:
                    continue
                if kind == "horizontal seam" and dy and max(y, ny) % arg == 0:
                    continue
                if kind == "seam corner" and dx and dy and max(x, nx) % arg[1] == 0 and max(y, ny) % arg[0] == 0:
                    continue
                seen[r] = 1
                stack.append(r)
        pix[1:] = sorted(pix[1:])
        comps.append((k, pix))
    return comps


def _one_pass(L, ncls, conn):
    """the one-pass labeller: a pixel takes the smallest provisional label among the neighbours already visited, and nothing is ever merged"""
    h, w = L.shape
    lab = L.ravel().tolist()
    prov = [-1] * (h * w)
    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if conn == 8 else [])
    groups = []
    for p in range(h * w):
        if lab[p] >= ncls:
            continue
        y, x = divmod(p, w)
        best = -1
        for dy, dx in back:
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w and lab[ny * w + nx] == lab[p]:
                c = prov[ny * w + nx]
                best = c if best < 0 or c < best else best
        if best < 0:
            best = len(groups)
            groups.append((lab[p], []))
        prov[p] = best
        groups[best][1].append(p)
    return groups


def _restate(case, flaw=None):
    """(count, comp, sums, ids) of a case by flood fill; flaw = (name, argument) makes it one of the wrong kernels"""
    s = case.shape
    kind, arg = flaw if flaw else (None, None)
    conn, min_area, maxc = case.connectivity, case.min_area, case.max_components
    if kind == "connectivity":
        conn = 12 - conn
    src = image.labels_to_source_host(ref.labels(s, case.pattern), s.out_h, s.out_w, s.h, s.w)
    n, h, w = src.shape
    ys, xs = image.nearest_index(h, s.out_h), image.nearest_index(w, s.out_w)
    count = np.zeros(n, np.int32)
    comp = np.full((n, maxc, 8), -1, np.int32)
    sums = np.zeros((n, maxc, 2), np.uint64)
    ids = np.full((n, h, w), -1, np.int32)
    if kind == "across frames":                     # no frame offset in the parent index: the frames are one tall map
        stacked = _flood(src.reshape(n * h, w), s.ncls, conn)
        per_frame = [[] for _ in range(n)]
        for k, pix in stacked:
            per_frame[pix[0] // (h * w)].append((k, pix))
    for f in range(n):
        if kind == "across frames":
            comps = per_frame[f]
        elif kind == "one pass":
            comps = _one_pass(src[f], s.ncls, conn)
        else:
            comps = _flood(src[f], s.ncls, conn, flaw)
        recs = []
        for k, pix in comps:
            p = np.asarray(pix, np.int64) - (f * h * w if kind == "across frames" else 0)
            y, x = p // w, p % w
            area = p.size
            if kind == "map area":
                area = np.unique(ys[np.clip(y, 0, h - 1)] * s.out_w + xs[x]).size
            anchor = p[-1] if kind == "last anchor" else p[0]
            recs.append(((k, area, x.min(), y.min(), x.max(), y.max(), anchor % w, anchor // w), (int(x.sum()), int(y.sum())), p))
        limit = min_area + 1 if kind == "min_area above" else min_area - 1 if kind == "min_area below" else min_area
        kept = [r for r in recs if r[0][1] >= limit]
        count[f] = min(len(kept), maxc) if kind == "count clipped" else len(kept)
        if kind == "order by area":
            kept.sort(key=lambda r: -r[0][1])
        if kind == "keep largest":
            big = sorted(range(len(kept)), key=lambda i: -kept[i][0][1])[:maxc]
            kept = [kept[i] for i in sorted(big)]
        if kind == "ids of filtered":
            for i, r in enumerate(recs):
                q = r[2][(r[2] >= 0) & (r[2] < h * w)]
                ids[f].reshape(-1)[q] = min(i, maxc - 1)
        for i, (rec, sm, p) in enumerate(kept[:maxc]):
            comp[f, i] = rec
            sums[f, i] = sm
            q = p[(p >= 0) & (p < h * w)]
            ids[f].reshape(-1)[q] = i
    return count, comp, sums, ids


def _equal(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_the_specification_equals_a_scalar_flood_fill(case):
    got, want = ref.expected(case), _restate(case)
    for name, a, b in zip(ref.Expected._fields, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, a.shape)
        assert np.array_equal(a, b), (name, int(np.count_nonzero(a != b)))


@pytest.mark.parametrize("case", [c for c in ref.CASES if c.min_area == 1 and not (c.trunc and c.shape is not ref.ROW)], ids=ref.case_id)
def test_the_specification_equals_scipy(case):
    """scipy.ndimage.label per class with the 4- and the 8-structure: the area multiset, the boxes and the anchor order after sorting scipy's
    components by their first pixel"""
    ndimage = pytest.importorskip("scipy.ndimage")
    s = case.shape
    src = image.labels_to_source_host(ref.labels(s, case.pattern), s.out_h, s.out_w, s.h, s.w)
    structure = ndimage.generate_binary_structure(2, 1 if case.connectivity == 4 else 2)
    count, comp, sums = image.labels_components_host(ref.labels(s, case.pattern), s.out_h, s.out_w, s.h, s.w, s.ncls,
                                                     connectivity=case.connectivity, max_components=65536)
    for f in range(s.n):
        found = []
        for k in np.unique(src[f]):
            if k >= s.ncls:
                continue
            lab, m = ndimage.label(src[f] == k, structure=structure)
            first = np.unique(lab, return_index=True)[1][-m:]                 # the first pixel of the labels 1 .. m, in raster order
            areas = np.bincount(lab.ravel(), minlength=m + 1)[1:]
            for i, box in enumerate(ndimage.find_objects(lab)):
                found.append((int(first[i]), int(k), int(areas[i]), box[1].start, box[0].start, box[1].stop - 1, box[0].stop - 1))
        found.sort()
        assert count[f] == len(found)
        rec, _ = image.components_of((count, comp, sums), f)
        want = np.array([(k, a, x0, y0, x1, y1, p % s.w, p // s.w) for p, k, a, x0, y0, x1, y1 in found[:65536]], np.int32).reshape(-1, 8)
        assert sorted(rec[:, 1].tolist()) == sorted(want[:, 1].tolist())
        assert np.array_equal(rec, want)


# ---- what the table covers ------------------------------------------------------------------------------------------------------------------------------------
def test_truncation_is_where_the_table_says_and_nowhere_else():
    assert any(c.trunc for c in ref.CASES)
    for c in ref.CASES:
        count = ref.expected(c).count
        if c.trunc:
            assert (count > c.max_components).any(), ref.case_id(c)
        else:
            assert (count <= c.max_components).all(), ref.case_id(c)          # no comparison passes on padding alone


def test_a_component_spans_three_by_three_large_tiles():
    spans = []
    for c in ref.CASES:
        comp = ref.expected(c).comp
        used = comp[comp[..., 0] >= 0]
        spans.append(int(((used[:, 5] // 64 - used[:, 3] // 64 >= 2) & (used[:, 4] // 128 - used[:, 2] // 128 >= 2)).sum()))
    assert max(spans) > 0 and sum(1 for v in spans if v) >= 10


def test_every_record_field_takes_several_values():
    seen = [set() for _ in range(10)]
    for c in ref.CASES:
        e = ref.expected(c)
        used = e.comp[..., 0] >= 0
        for i in range(8):
            seen[i].update(np.unique(e.comp[used][:, i]).tolist()[:50])
        seen[8].update(np.unique(e.sums[used][:, 0]).tolist()[:50])
        seen[9].update(np.unique(e.sums[used][:, 1]).tolist()[:50])
    assert all(len(v) >= 2 for v in seen), [len(v) for v in seen]
    assert any(int(ref.expected(c).sums.max()) > 1 << 32 for c in ref.CASES if c.shape in (ref.WIDE, ref.TALL))       # the 64-bit sums are needed
    assert {int(ref.expected(c).count.max()) for c in ref.CASES} >= {0, 1, 2}
    assert any((ref.expected(c).ids[0] == -1).any() and (ref.expected(c).ids[0] >= 0).any() for c in ref.CASES)


def test_the_hand_made_pictures_are_what_they_are_meant_to_be():
    def count(shape, pattern, conn, min_area=1):
        return [int(v) for v in ref.expected(next(c for c in ref.CASES if (c.shape, c.pattern, c.connectivity, c.min_area) ==
                                                  (shape, pattern, conn, min_area))).count]
    s = ref.IDENT
    assert count(s, "serpentine", 4) == [1] and count(s, "serpentine_cut", 4) == [2] and count(s, "spiral", 4) == [1]
    assert count(s, "checker", 4)[0] == s.h * s.w and count(s, "checker", 8) == [2]
    assert count(s, "diagonals", 4)[0] > 20 * count(s, "diagonals", 8)[0]
    assert count(s, "background", 8) == [0] and count(s, "one", 4) == [1]
    assert count(s, "interleaved", 4)[0] > 100 and count(s, "interleaved", 8) == [2]
    assert count(ref.BATCH, "comb", 8) == count(ref.BATCH, "comb", 8)[:1] * 8
    serp = ref.expected(next(c for c in ref.CASES if c.shape is s and c.pattern == "serpentine" and c.connectivity == 4))
    assert serp.comp[0, 0].tolist() == [1, (s.h // 2) * s.w + s.h // 2, 0, 0, s.w - 1, s.h - 1, 0, 0]
    comb = ref.expected(next(c for c in ref.CASES if c.shape is s and c.pattern == "comb" and c.connectivity == 4 and not c.trunc))
    assert comb.comp[0, 0, 5] == s.h - 1 and comb.comp[0, 0, 4] == s.w - 1        # the first component reaches the last row, where its arms join
    every, some = count(s, "sizes", 8), count(s, "sizes", 8, ref.SIZE)
    sizes = ref.expected(next(c for c in ref.CASES if c.shape is s and c.pattern == "sizes" and c.connectivity == 8 and c.min_area == 1))
    areas = sizes.comp[0, :every[0], 1]
    assert {ref.SIZE - 1, ref.SIZE, ref.SIZE + 1} <= set(areas.tolist()) and some[0] == int((areas >= ref.SIZE).sum()) < every[0]


# ---- the power of the table: wrong kernels ----------------------------------------------------------------------------------------------------------------------
def _on(shape=None, pattern=None, conn=None, **kw):
    def pick(c):
        return ((shape is None or c.shape is shape) and (pattern is None or c.pattern == pattern) and (conn is None or c.connectivity == conn)
                and all(getattr(c, k) == v for k, v in kw.items()))
    return pick


# name -> (the flaw, the cases it is tried on: it must differ from the specification on at least one of them)
FLAWS = {
    "4 for 8": (("connectivity", None), _on(ref.IDENT, "checker", 8, max_components=65536)),
    "8 for 4": (("connectivity", None), _on(ref.IDENT, "diagonals", 4)),
    "joins across background": (("across background", None), _on(ref.IDENT, "serpentine_cut", 4)),
    "joins across classes": (("across classes", None), _on(ref.IDENT, "interleaved", 4)),
    "misses the vertical seam, tiles 32 wide": (("vertical seam", 32), _on(ref.LARGER, "one", 4)),
    "misses the vertical seam, tiles 64 wide": (("vertical seam", 64), _on(ref.IDENT, "one", 4)),
    "misses the vertical seam, tiles 128 wide": (("vertical seam", 128), _on(ref.BATCH, "one", 8)),
    "misses the horizontal seam, tiles 8 high": (("horizontal seam", 8), _on(ref.BATCH, "one", 4)),
    "misses the horizontal seam, tiles 16 high": (("horizontal seam", 16), _on(ref.IDENT, "one", 8)),
    "misses the horizontal seam, tiles 32 high": (("horizontal seam", 32), _on(ref.LARGER, "one", 8)),
    "misses the horizontal seam, tiles 64 high": (("horizontal seam", 64), _on(ref.BATCH, "one", 4)),
    "misses the diagonals at a corner of 16 x 64 tiles": (("seam corner", (16, 64)), _on(ref.IDENT, "diagonals", 8)),
    "misses the diagonals at a corner of 8 x 32 tiles": (("seam corner", (8, 32)), _on(ref.IDENT, "diagonals", 8)),
    "misses the diagonals at a corner of 64 x 128 tiles": (("seam corner", (64, 128)), _on(ref.IDENT, "diagonals", 8)),
    "one pass, no upward propagation": (("one pass", None), _on(ref.BATCH, "comb", 4, max_components=1024)),
    "anchor is the last pixel": (("last anchor", None), _on(ref.BATCH, "runs", 8)),
    "joins across frames": (("across frames", None), _on(ref.BATCH, "one", 4)),
    "area in map pixels": (("map area", None), _on(ref.LARGER, "runs", 8, min_area=1)),
    "min_area one too large": (("min_area above", None), _on(ref.IDENT, "sizes", 8, min_area=ref.SIZE)),
    "min_area one too small": (("min_area below", None), _on(ref.IDENT, "sizes", 8, min_area=ref.SIZE)),
    "truncation keeps the largest": (("keep largest", None), _on(ref.BATCH, "comb", 8, max_components=3)),
    "order by area": (("order by area", None), _on(ref.BATCH, "comb", 8, max_components=1024)),
    "count clipped to max_components": (("count clipped", None), _on(ref.BATCH, "comb", 4, max_components=3)),
    "ids of filtered components not -1": (("ids of filtered", None), _on(ref.BATCH, "sizes", 4, min_area=ref.SIZE + 1)),
}


@pytest.mark.parametrize("name", sorted(FLAWS))
def test_the_table_tells_a_wrong_kernel_from_the_right_one(name):
    flaw, pick = FLAWS[name]
    cases = [c for c in ref.CASES if pick(c)]
    assert cases, "no case of the table is tried on %s" % name
    assert any(not _equal(_restate(c, flaw), ref.expected(c)) for c in cases), "%s passes every case it is tried on" % name


# ---- the helpers -----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_helpers_on_a_hand_made_map():
    a = np.full((2, 4, 6), 255, np.uint8)
    a[0, 0, 0:2] = 3            # two pixels
    a[0, 2:4, 4:6] = 1          # a square of four
    a[0, 3, 0] = 3              # a single pixel
    a[1, 1, 1] = 0
    a[1, 2, 2] = 0              # joined to it under 8 only
    count, comp, sums, ids = image.labels_components_host(a, 4, 6, 4, 6, 19, max_components=4, ids=True)
    assert count.tolist() == [3, 1] and count.dtype == np.int32 and comp.dtype == np.int32 and sums.dtype == np.uint64 and ids.dtype == np.int32
    assert comp[0].tolist() == [[3, 2, 0, 0, 1, 0, 0, 0], [1, 4, 4, 2, 5, 3, 4, 2], [3, 1, 0, 3, 0, 3, 0, 3], [-1] * 8]
    assert sums[0].tolist() == [[1, 0], [18, 10], [0, 3], [0, 0]]
    assert comp[1, 0].tolist() == [0, 2, 1, 1, 2, 2, 1, 1] and (comp[1, 1:] == -1).all()
    assert ids[0].tolist() == [[0, 0, -1, -1, -1, -1], [-1] * 6, [-1, -1, -1, -1, 1, 1], [2, -1, -1, -1, 1, 1]]
    assert image.labels_components_host(a, 4, 6, 4, 6, 19, connectivity=4)[0].tolist() == [3, 2]
    count2, comp2, _, ids2 = image.labels_components_host(a, 4, 6, 4, 6, 19, min_area=2, max_components=1, ids=True)
    assert count2.tolist() == [2, 1] and comp2[0, 0].tolist() == [3, 2, 0, 0, 1, 0, 0, 0] and (ids2[0] >= 0).sum() == 2 and ids2[0].max() == 0
    cen = image.components_centroids(comp, sums)
    assert cen.shape == (2, 4, 2) and cen[0, :3].tolist() == [[0.5, 0.0], [4.5, 2.5], [0.0, 3.0]] and np.isnan(cen[0, 3]).all() and np.isnan(cen[1, 1:]).all()
    rec, sm = image.components_of((count, comp, sums), 0)
    assert rec.shape == (3, 8) and sm.shape == (3, 2) and image.components_of((count2, comp2, sums[:, :1]), 0)[0].shape == (1, 8)
    # one map is a batch of one; an enlargement counts source pixels
    one = image.labels_components_host(a[0], 4, 6, 8, 12, 19)
    assert one[0].tolist() == [3] and one[1][0, 1].tolist() == [1, 16, 8, 4, 11, 7, 8, 4]


def test_argument_errors_of_the_specification():
    a = np.zeros((1, 4, 6), np.uint8)
    for kw, word in ((dict(ncls=0), "ncls"), (dict(ncls=33), "ncls"), (dict(connectivity=6), "connectivity"), (dict(min_area=0), "min_area"),
                     (dict(max_components=0), "max_components"), (dict(max_components=65537), "max_components"), (dict(out_h=5), "out_h"),
                     (dict(w=32769), "h x w")):
        args = dict(out_h=4, out_w=6, h=4, w=6, ncls=19)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            image.labels_components_host(a, **args)
    with pytest.raises(ValueError, match="H x W"):
        image.labels_components_host(np.zeros(4, np.uint8), 1, 1, 1, 1, 1)
