"""Trimap evaluation, host side: utils.image.boundary_distance_host and band_hist_host -- the integer specification the GPU kernels are tested against --
equal scalar, pixel-by-pixel restatements; the case table of band_ref.py fills every bucket and tells each of a list of plausible wrong kernels from the
right one; TrimapEvaluator's host arithmetic does what it says; and the C ABI declares and exports the entry points.  (GPU side: test_labels_band_gpu.py.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

import band_ref as ref

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("accel_boundary_distance", "accel_labels_band_hist", "accel_model_band_hist_add", "accel_model_scores_band_hist_add",
                "accel_model_band_hist_read")
SCALAR_PIXELS = 20000           # the scalar restatement walks the cases with h * w at most this


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
    assert len(runtime.EXPORTS["accel_boundary_distance"]) == 9 and len(runtime.EXPORTS["accel_labels_band_hist"]) == 15
    assert len(runtime.EXPORTS["accel_model_band_hist_add"]) == 12 and len(runtime.EXPORTS["accel_model_scores_band_hist_add"]) == 12
    assert len(runtime.EXPORTS["accel_model_band_hist_read"]) == 5
    for name in ("boundary_distance", "labels_band_hist"):
        assert hasattr(runtime.Context, name), name
    for name in ("band_hist_add", "band_hist_add_device", "scores_band_hist_add", "band_hist_read"):
        assert hasattr(runtime.Model, name), name
    for name in ("boundary_distance", "TrimapEvaluator", "Evaluator"):
        assert hasattr(results, name), name
    for name in ("boundary_distance_host", "band_hist_host"):
        assert hasattr(image, name), name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


# ---- the table fills every bucket: asserted from the specification alone, before anything else trusts the table -----------------------------------------
@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s not in ref.TINY], ids=lambda s: "x".join(str(v) for v in s[:8]))
@pytest.mark.parametrize("values", ["blocks", "blocks+ignored"])
def test_the_block_maps_put_counted_pixels_into_every_bucket(shape, values):
    d = ref.distance(shape, values)
    cap = shape.widths[-1]
    assert sorted(np.unique(d).tolist()) == list(range(cap + 1)), "not every distance 0 .. cap occurs"
    for pred in ref.PREDS:
        want = ref.expected(ref.Case(shape, values, pred))
        assert want.shape == (len(shape.widths) + 1, shape.ncls, shape.ncls) and want.dtype == np.uint64
        assert (want.sum(axis=(1, 2)) > 0).all(), (pred, want.sum(axis=(1, 2)).tolist())


def test_flat_noise_and_lattice_are_what_they_are_for():
    for s in ref.SHAPES:
        assert (ref.distance(s, "flat") == s.widths[-1]).all()                          # no edge at all: everything in the rest bucket
        assert not ref.expected(ref.Case(s, "flat", "independent"))[:-1].any()
        if s.ncls > 3:
            assert (ref.distance(s, "noise") == 0).mean() > 0.95                        # (nearly) every pixel is an edge
    d = ref.distance(ref.LATTICE, "lattice")[0]
    assert d[0, 0] == 0 and d[37, 41] == 0 and d[74, 287] == 0 and d[1, 1] == 1 and d[0, 1] == 0 and d[37 + 16, 41 + 16] == 16
    assert sorted(np.unique(d).tolist()) == list(range(17))
    # the squares around the lone pixels meet tile borders of 8, 16, 32 and 64 pixels at several phases
    ys, xs = np.arange(0, 96, 37), np.arange(0, 300, 41)
    for tile in (8, 16, 32, 64):
        assert len(set((xs % tile).tolist())) >= min(tile, 6) and len(set((ys % tile).tolist())) >= 2


# ---- the specification against scalar restatements -----------------------------------------------------------------------------------------------------------
def _edges_scalar(g, h, w):
    e = [[False] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            c = g[y][x]
            e[y][x] = ((y > 0 and g[y - 1][x] != c) or (y < h - 1 and g[y + 1][x] != c) or (x > 0 and g[y][x - 1] != c)
                       or (x < w - 1 and g[y][x + 1] != c))
    return e


def _distance_scalar(g, h, w, cap):
    """d of one map, every pixel in turn, in Python integers: the smallest r < cap whose (2 r + 1)-square around the pixel, cut at the frame, holds an
    edge pixel -- the squares are counted with a summed-area table of the edge flags -- and cap where there is none"""
    e = _edges_scalar(g, h, w)
    area = [[0] * (w + 1) for _ in range(h + 1)]
    for y in range(h):
        run, above, row = 0, area[y], area[y + 1]
        for x in range(w):
            run += 1 if e[y][x] else 0
            row[x + 1] = above[x + 1] + run
    d = [[cap] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            for r in range(cap):
                y0, y1, x0, x1 = max(y - r, 0), min(y + r, h - 1) + 1, max(x - r, 0), min(x + r, w - 1) + 1
                if area[y1][x1] - area[y0][x1] - area[y1][x0] + area[y0][x0]:
                    d[y][x] = r
                    break
    return d


def _distance_brute(g, h, w, cap):
    """the definition itself: the minimum over ALL edge pixels, for the two tiny shapes"""
    e = _edges_scalar(g, h, w)
    at = [(y, x) for y in range(h) for x in range(w) if e[y][x]]
    return [[min([cap] + [max(abs(y - ey), abs(x - ex)) for ey, ex in at]) for x in range(w)] for y in range(h)]


def _distance_separable(g, cap):
    """the form the kernel takes, in numpy: a row pass hd = min |dx| to an edge within cap - 1, then d = min over dy of max(|dy|, hd(y + dy, x))"""
    e = image.boundary_edges_host(g)
    n, h, w = e.shape
    hd = np.full((n, h, w), cap, np.int64)
    for dx in range(-(cap - 1), cap):
        if abs(dx) >= w:
            continue
        src = e[:, :, max(dx, 0):w + min(dx, 0)]
        view = hd[:, :, max(-dx, 0):w + min(-dx, 0)]
        np.minimum(view, np.where(src, abs(dx), cap), out=view)
    d = np.full((n, h, w), cap, np.int64)
    for dy in range(-(cap - 1), cap):
        if abs(dy) >= h:
            continue
        src = hd[:, max(dy, 0):h + min(dy, 0), :]
        view = d[:, max(-dy, 0):h + min(-dy, 0), :]
        np.minimum(view, np.maximum(src, abs(dy)), out=view)
    return d.astype(np.uint8)


@pytest.mark.parametrize("shape", ref.ALL_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:8]))
def test_the_distance_equals_its_restatements(shape):
    s = shape
    cap = s.widths[-1]
    for values in ref.maps_of(s):
        g, d = ref.ground_truth(s, values), ref.distance(s, values)
        assert d.dtype == np.uint8 and d.shape == (s.n, s.h, s.w)
        assert np.array_equal(d, _distance_separable(g, cap)), values
        if s.h * s.w <= SCALAR_PIXELS:
            for f in range(s.n):
                assert d[f].tolist() == _distance_scalar(g[f].tolist(), s.h, s.w, cap), (values, f)
        if s in ref.TINY:
            assert d[0].tolist() == _distance_brute(g[0].tolist(), s.h, s.w, cap), values
        # the pitched form holds the same maps
        assert np.array_equal(ref.ground_truth_pitched(s, values)[:, :, :s.w], g)


def _hist_scalar(case):
    """every source pixel in turn, in Python integers, from the specification's distance"""
    s = case.shape
    K = len(s.widths)
    hist = [[0] * (s.ncls * s.ncls) for _ in range(K + 1)]
    cols = [min(x * s.out_w // s.w, s.out_w - 1) for x in range(s.w)]
    maps, gt, dist = ref.labels(case).tolist(), ref.ground_truth(s, case.values).tolist(), ref.distance(s, case.values).tolist()
    for f in range(s.n):
        for y in range(s.h):
            row = maps[f][min(y * s.out_h // s.h, s.out_h - 1)]
            g, d = gt[f][y], dist[f][y]
            for x in range(s.w):
                p = row[cols[x]]
                if g[x] < s.ncls and p < s.ncls:
                    k = 0
                    while k < K and d[x] >= s.widths[k]:
                        k += 1
                    hist[k][g[x] * s.ncls + p] += 1
    return hist


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_the_buckets_equal_a_scalar_restatement_and_sum_to_the_confusion_matrix(case):
    from accel_amd import demo
    s = case.shape
    want = ref.expected(case)
    assert want.dtype == np.uint64 and want.shape == (len(s.widths) + 1, s.ncls, s.ncls)
    if s.h * s.w <= SCALAR_PIXELS:
        assert want.reshape(len(s.widths) + 1, -1).tolist() == _hist_scalar(case)
    pred, gt = image.labels_to_source_host(ref.labels(case), s.out_h, s.out_w, s.h, s.w).reshape(-1), ref.ground_truth(s, case.values).reshape(-1)
    k = pred < s.ncls                   # (fast_hist assumes pred < ncls: the argmax of ncls channels)
    assert np.array_equal(want.sum(axis=0).astype(np.int64), demo.fast_hist(pred[k], gt[k], s.ncls))
    assert np.array_equal(image.band_cumulative(want)[-1], want.sum(axis=0).astype(np.int64))


# ---- wrong kernels: the table tells each of them from the right one ----------------------------------------------------------------------------------
FLAWS = ("edges8", "frame_edges", "class_edges", "pred_edges", "manhattan", "le_width", "short_halo", "next_frame", "pitch_w", "gap_neighbours", "no_cap",
         "bucket_off", "identity_pred", "drop_last")


def _edges(g, diagonal=False):
    e = image.boundary_edges_host(g)
    if diagonal:
        down = g[:, 1:, 1:] != g[:, :-1, :-1]
        e[:, 1:, 1:] |= down
        e[:, :-1, :-1] |= down
        up = g[:, 1:, :-1] != g[:, :-1, 1:]
        e[:, 1:, :-1] |= up
        e[:, :-1, 1:] |= up
    return e


def _grow(edges, rounds, none, manhattan=False):
    """the distance to the nearest flag by `rounds` rounds of dilation (3 x 3, or the 4-neighbourhood), `none` where none was reached; n x h x w int64"""
    reached = edges.copy()
    d = np.where(reached, 0, none).astype(np.int64)
    for r in range(1, rounds + 1):
        up = reached.copy()
        up[:, 1:, :] |= reached[:, :-1, :]
        up[:, :-1, :] |= reached[:, 1:, :]
        src = reached if manhattan else up
        nxt = up.copy()
        nxt[:, :, 1:] |= src[:, :, :-1]
        nxt[:, :, :-1] |= src[:, :, 1:]
        d[nxt & ~reached] = r
        reached = nxt
    return d


def _variant(case, flaw=None):
    """the buckets of the case as a kernel with one flaw would compute them, in numpy; flaw=None: the right kernel.  The ground truth is taken in its
    pitched form, as a kernel gets it"""
    s = case.shape
    ws, cap, K = s.widths, s.widths[-1], len(s.widths)
    gp = ref.ground_truth_pitched(s, case.values)
    g = gp[:, :, :s.w]
    if flaw == "pitch_w":
        g = gp.reshape(s.n, -1)[:, :s.h * s.w].reshape(s.n, s.h, s.w)
    lab = ref.labels(case)
    if flaw == "identity_pred":
        pred = lab[:, np.minimum(np.arange(s.h), s.H - 1), :][:, :, np.minimum(np.arange(s.w), s.W - 1)]
    else:
        pred = image.labels_to_source_host(lab, s.out_h, s.out_w, s.h, s.w)
    if flaw == "gap_neighbours":
        e = _edges(gp)[:, :, :s.w]
    elif flaw == "pred_edges":
        e = _edges(pred)
    elif flaw == "class_edges":
        valid = g.astype(np.int64)                                     # a border to an ignored id does not count, from either side
        valid[g >= s.ncls] = -1
        e = np.zeros(g.shape, bool)
        dy = (valid[:, 1:, :] != valid[:, :-1, :]) & (valid[:, 1:, :] >= 0) & (valid[:, :-1, :] >= 0)
        dx = (valid[:, :, 1:] != valid[:, :, :-1]) & (valid[:, :, 1:] >= 0) & (valid[:, :, :-1] >= 0)
        e[:, 1:, :] |= dy
        e[:, :-1, :] |= dy
        e[:, :, 1:] |= dx
        e[:, :, :-1] |= dx
    else:
        e = _edges(g, diagonal=flaw == "edges8")
    if flaw == "frame_edges":
        e = e.copy()
        e[:, 0, :] = e[:, -1, :] = True
        e[:, :, 0] = e[:, :, -1] = True
    if flaw == "next_frame":
        d = _grow(e.reshape(1, s.n * s.h, s.w), cap - 1, cap).reshape(s.n, s.h, s.w)
    elif flaw == "short_halo":
        d = _grow(e, max(cap - 2, 0), cap)
        if cap == 1:
            d[...] = cap
    elif flaw == "no_cap":
        d = _grow(e, 40, 255) & 15
    else:
        d = _grow(e, cap - 1, cap, manhattan=flaw == "manhattan")
    bucket = np.searchsorted(np.asarray(ws, np.int64), d, side="left" if flaw == "le_width" else "right")
    ok = (g < s.ncls) & (pred < s.ncls)
    at = (bucket[ok] * s.ncls + g[ok].astype(np.int64)) * s.ncls + pred[ok].astype(np.int64)
    hist = np.bincount(at, minlength=(K + 1) * s.ncls * s.ncls).astype(np.uint64).reshape(K + 1, s.ncls, s.ncls)
    if flaw == "bucket_off":
        hist = np.roll(hist, 1, axis=0)
    if flaw == "drop_last":
        hist[K] = 0
    return hist


def _differs(case, flaw):
    return not np.array_equal(_variant(case, flaw), ref.expected(case))


def test_the_variant_without_a_flaw_is_the_specification():
    assert not any(_differs(case, None) for case in ref.CASES)


@pytest.mark.parametrize("flaw", FLAWS)
def test_the_table_tells_a_wrong_kernel_from_the_right_one(flaw):
    caught = [ref.case_id(case) for case in ref.CASES if _differs(case, flaw)]
    assert caught, "no case of the table notices a kernel with the flaw '%s'" % flaw


# ---- the host arithmetic of TrimapEvaluator --------------------------------------------------------------------------------------------------------------
def test_trimap_evaluator_host_arithmetic():
    from accel_amd.core import results
    ev = results.TrimapEvaluator(2, widths=(1, 4))
    assert ev.widths == (1, 4) and ev.num_classes == 2
    assert ev.hist().shape == (3, 2, 2) and ev.hist().dtype == np.int64 and not ev.hist().any()
    assert all(math.isnan(v) for v in ev.miou())
    buckets = np.array([[[0, 0], [0, 0]],              # nothing on the edge pixels themselves
                        [[3, 1], [2, 2]],              # 1 <= d < 4
                        [[10, 0], [0, 30]]], np.uint64)
    hist = results.TrimapEvaluator.cumulative(buckets)
    assert hist.dtype == np.int64 and hist.tolist() == [[[0, 0], [0, 0]], [[3, 1], [2, 2]], [[13, 1], [2, 32]]]
    iu = results.TrimapEvaluator.iu_of(hist)
    assert iu.shape == (3, 2) and np.isnan(iu[0]).all()
    assert iu[1].tolist() == [3 / 6.0, 2 / 5.0] and iu[2].tolist() == [13 / 16.0, 32 / 35.0]
    miou = results.TrimapEvaluator.miou_of(hist)
    assert miou.shape == (3,) and math.isnan(miou[0])                  # an empty band
    assert miou[1] == pytest.approx((3 / 6.0 + 2 / 5.0) / 2) and miou[2] == pytest.approx((13 / 16.0 + 32 / 35.0) / 2)
    # a class that is absent from a band does not count in its mean
    one = results.TrimapEvaluator.miou_of(np.array([[[4, 0], [0, 0]]]))
    assert one.tolist() == [1.0]
    assert results.TrimapEvaluator(19).widths == (1, 2, 4, 8)
    for bad in ((), (1, 2, 3, 4, 5), (0, 1), (1, 17), (2, 2), (4, 2), "ab"):
        with pytest.raises(ValueError, match="width"):
            results.TrimapEvaluator(19, widths=bad)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="num_classes"):
            results.TrimapEvaluator(bad)


def test_argument_errors_of_the_specification():
    g = np.zeros((1, 8, 8), np.uint8)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="cap"):
            image.boundary_distance_host(g, bad)
    with pytest.raises(ValueError, match="maps"):
        image.boundary_distance_host(np.zeros((1, 1, 8, 8), np.uint8), 4)
    with pytest.raises(ValueError, match="ncls"):
        image.band_hist_host(g, 8, 8, g, 33, (1,))
    with pytest.raises(ValueError, match="ascending"):
        image.band_hist_host(g, 8, 8, g, 19, (2, 1))
    with pytest.raises(ValueError, match="ground-truth"):
        image.band_hist_host(g, 8, 8, np.zeros((2, 8, 8), np.uint8), 19, (1,))
    one = image.band_hist_host(g[0], 8, 8, g[0], 2, (1, 2))                  # a single map is a batch of one; no edge: the rest bucket
    assert one.tolist() == [[[0, 0], [0, 0]], [[0, 0], [0, 0]], [[64, 0], [0, 0]]]
    assert image.boundary_distance_host(g[0], 3).shape == (1, 8, 8)
    assert image.band_buckets_host([0, 1, 2, 3, 4, 8], (1, 2, 4)).tolist() == [0, 1, 2, 2, 3, 3]
