"""Summary of finished frames, host side: utils.image.labels_summary_host -- the integer specification the GPU kernel is tested against -- equals a
scalar, loop-per-pixel restatement; the case table of summary_ref.py tells each of a list of plausible wrong kernels from the right one; the churn and
centroid helpers do what they say; and the C ABI declares and exports the entry points.  (GPU side: test_labels_summary_gpu.py.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

import summary_ref as ref

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("accel_labels_summary", "accel_model_labels_summary", "accel_model_scores_summary", "accel_model_labels_forget")


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
    assert len(runtime.EXPORTS["accel_labels_summary"]) == 17
    assert len(runtime.EXPORTS["accel_model_labels_summary"]) == 13 and len(runtime.EXPORTS["accel_model_scores_summary"]) == 13
    assert hasattr(runtime.Context, "labels_summary")
    for name in ("labels_summary", "scores_summary", "labels_forget"):
        assert hasattr(runtime.Model, name), name
    for name in ("summary", "forget", "Summary", "summary_churn", "summary_centroids", "per_class_iu"):
        assert hasattr(results, name), name
    assert results.Summary._fields == ("stats", "box", "trans")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


# ---- the specification against a scalar restatement --------------------------------------------------------------------------------------------
def _summary_scalar(labels, prev, s):
    """every source pixel in turn, in Python integers"""
    stats = [[[0, 0, 0] for _ in range(s.ncls)] for _ in range(s.n)]
    box = [[[s.w, s.h, -1, -1] for _ in range(s.ncls)] for _ in range(s.n)]
    trans = [[0] * (s.ncls * s.ncls) for _ in range(s.n)]
    kept = []
    cols = [min(x * s.out_w // s.w, s.out_w - 1) for x in range(s.w)]
    maps, before = labels.tolist(), prev.tolist()
    for f in range(s.n):
        st, bx, tr, frame = stats[f], box[f], trans[f], []
        for y in range(s.h):
            row = maps[f][min(y * s.out_h // s.h, s.out_h - 1)]
            line = [row[c] for c in cols]
            frame.append(line)
            was = before[f][y]
            for x, k in enumerate(line):
                if k >= s.ncls:
                    continue
                e, b = st[k], bx[k]
                e[0] += 1
                e[1] += x
                e[2] += y
                if x < b[0]:
                    b[0] = x
                if y < b[1]:
                    b[1] = y
                if x > b[2]:
                    b[2] = x
                if y > b[3]:
                    b[3] = y
                if was[x] < s.ncls:
                    tr[was[x] * s.ncls + k] += 1
        kept.append(frame)
    return stats, box, trans, kept


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_the_specification_equals_a_scalar_restatement(case):
    s = case.shape
    want = ref.expected(case)
    assert want.stats.dtype == np.uint64 and want.stats.shape == (s.n, s.ncls, 3)
    assert want.box.dtype == np.int32 and want.box.shape == (s.n, s.ncls, 4)
    assert want.trans.dtype == np.uint64 and want.trans.shape == (s.n, s.ncls * s.ncls)
    assert want.kept.dtype == np.uint8 and want.kept.shape == (s.n, s.h, s.w)
    stats, box, trans, kept = _summary_scalar(ref.labels(s, case.values), ref.previous(case), s)
    assert want.stats.tolist() == stats
    assert want.box.tolist() == box
    assert want.trans.tolist() == trans
    assert want.kept.tolist() == kept
    assert np.array_equal(want.kept, image.labels_to_source_host(ref.labels(s, case.values), s.out_h, s.out_w, s.h, s.w))
    # without a previous frame: the same, and no transitions
    if case.prev == ref.PREVS[0]:
        alone = image.labels_summary_host(ref.labels(s, case.values), s.out_h, s.out_w, s.h, s.w, s.ncls)
        assert alone[2] is None and all(np.array_equal(a, b) for a, b in zip((alone[0], alone[1], alone[3]), (want.stats, want.box, want.kept)))


def test_the_overflow_cases_exceed_32_bits():
    wide = ref.expected(ref.Case(ref.WIDE, "one", "equal"))
    assert wide.stats[0, 1].tolist() == [16 * 32768, 8589672448, 16 * 32768 * 15 // 2] and wide.stats[0, 1, 1] > 1 << 32
    assert not wide.stats[0, 0].any() and wide.box[0].tolist() == [[32768, 16, -1, -1], [0, 0, 32767, 15]]
    assert wide.trans[0].tolist() == [0, 0, 0, 16 * 32768]
    tall = ref.expected(ref.Case(ref.TALL, "one", "equal"))
    assert tall.stats[0, 0].tolist() == [32768 * 16, 32768 * 16 * 15 // 2, 8589672448] and tall.stats[0, 0, 2] > 1 << 32
    assert tall.box[0].tolist() == [[0, 0, 15, 32767]]


def test_single_has_empty_classes_with_the_identity_box():
    for s in ref.SHAPES:
        want = ref.expected(ref.Case(s, "single", "independent"))
        area = want.stats[..., 0]
        assert (area[:, 1::2] == 0).all() and (area[:, 0::2] > 0).all(), s
        assert (want.box[:, 1::2] == np.array([s.w, s.h, -1, -1])).all()
        assert (want.box[:, 0, :2] == 0).all()                                         # class 0 holds the corner (0, 0)
        last = (s.ncls - 1) // 2 * 2
        assert (want.box[:, last, 2] == s.w - 1).all() and (want.box[:, last, 3] == s.h - 1).all()      # and the largest even class (h - 1, w - 1)
        assert int(area.sum()) < s.n * s.h * s.w                                        # everything else is ignored


def test_rows_and_columns_of_the_transitions_are_the_areas_where_nothing_is_ignored():
    seen = 0
    for case in ref.CASES:
        if case.values not in ("runs", "one") or case.prev == "ignored":
            continue
        s, want = case.shape, ref.expected(case)
        t = want.trans.reshape(s.n, s.ncls, s.ncls)
        before = image.labels_summary_host(ref.previous(case), s.h, s.w, s.h, s.w, s.ncls)[0][..., 0]
        assert np.array_equal(t.sum(axis=2), before) and np.array_equal(t.sum(axis=1), want.stats[..., 0]), ref.case_id(case)
        assert int(t.sum()) == s.n * s.h * s.w
        if case.prev == "equal":
            assert not (t * (1 - np.eye(s.ncls, dtype=np.uint64))).any()                  # the diagonal only
        seen += 1
    assert seen >= 2 * 2 * len(ref.SHAPES)


# ---- wrong kernels: the table tells each of them from the right one ----------------------------------------------------------------------------------
FLAWS = ("exclusive_box", "swap_xy", "round", "padded", "clamp_ids", "trans_transposed", "frames_summed", "sum_x32", "sum_y32", "box_zero",
         "last_column", "kept_stale")


def _variant(case, flaw=None):
    """(stats, box, trans, kept) of the case as a kernel with one flaw would compute them, in numpy; flaw=None: the right kernel"""
    s = case.shape
    lab, prev = ref.labels(s, case.values), ref.previous(case)
    out_h, out_w = (s.H, s.W) if flaw == "padded" else (s.out_h, s.out_w)
    if flaw == "round":
        ys = np.minimum((np.arange(s.h, dtype=np.int64) * out_h + s.h // 2) // s.h, out_h - 1)
        xs = np.minimum((np.arange(s.w, dtype=np.int64) * out_w + s.w // 2) // s.w, out_w - 1)
    else:
        ys, xs = image.nearest_index(s.h, out_h), image.nearest_index(s.w, out_w)
    L = lab[:, ys, :][:, :, xs]
    cls = L.astype(np.int64)
    counted = cls < s.ncls
    if flaw == "clamp_ids":
        cls, counted = np.minimum(cls, s.ncls - 1), np.ones_like(counted)
    if flaw == "last_column":
        counted = counted & (np.arange(s.w) != s.w - 1)[None, None, :]
    F, Y, X = np.meshgrid(np.arange(s.n), np.arange(s.h), np.arange(s.w), indexing="ij")
    at = (F * s.ncls + cls)[counted]
    x, y = X[counted], Y[counted]
    cells = s.n * s.ncls
    a, b = (y, x) if flaw == "swap_xy" else (x, y)
    stats = np.stack([np.bincount(at, minlength=cells), np.bincount(at, weights=a, minlength=cells), np.bincount(at, weights=b, minlength=cells)],
                     axis=1).astype(np.uint64).reshape(s.n, s.ncls, 3)           # (float64 weights: every sum is below 2^53)
    x0, y0 = np.full(cells, s.w, np.int64), np.full(cells, s.h, np.int64)
    x1, y1 = np.full(cells, -1, np.int64), np.full(cells, -1, np.int64)
    np.minimum.at(x0, at, x)
    np.minimum.at(y0, at, y)
    np.maximum.at(x1, at, x)
    np.maximum.at(y1, at, y)
    box = np.stack([x0, y0, x1, y1], axis=1).reshape(s.n, s.ncls, 4)
    both = counted & (prev < s.ncls)
    pair = (F * s.ncls * s.ncls + prev.astype(np.int64) * s.ncls + cls)[both]
    trans = np.bincount(pair, minlength=cells * s.ncls).astype(np.uint64).reshape(s.n, s.ncls, s.ncls)
    empty = stats[..., 0] == 0
    if flaw == "exclusive_box":
        box[~empty, 2:] += 1
    if flaw == "box_zero":
        box[empty] = 0
    if flaw == "trans_transposed":
        trans = trans.transpose(0, 2, 1)
    if flaw == "frames_summed":
        stats = np.broadcast_to(stats.sum(axis=0, keepdims=True), stats.shape)
        trans = np.broadcast_to(trans.sum(axis=0, keepdims=True), trans.shape)
        box = np.broadcast_to(np.concatenate([box[..., :2].min(axis=0), box[..., 2:].max(axis=0)], axis=-1)[None], box.shape)
    if flaw == "sum_x32":
        stats = stats.copy()
        stats[..., 1] &= np.uint64(0xffffffff)
    if flaw == "sum_y32":
        stats = stats.copy()
        stats[..., 2] &= np.uint64(0xffffffff)
    kept = prev if flaw == "kept_stale" else L
    return stats.astype(np.uint64), box.astype(np.int32), np.ascontiguousarray(trans).reshape(s.n, -1).astype(np.uint64), kept


def _differs(case, flaw):
    return not all(np.array_equal(a, b) for a, b in zip(_variant(case, flaw), ref.expected(case)))


def test_the_variant_without_a_flaw_is_the_specification():
    assert not any(_differs(case, None) for case in ref.CASES)


@pytest.mark.parametrize("flaw", FLAWS)
def test_the_table_tells_a_wrong_kernel_from_the_right_one(flaw):
    caught = [ref.case_id(case) for case in ref.CASES if _differs(case, flaw)]
    assert caught, "no case of the table notices a kernel with the flaw '%s'" % flaw


# ---- the host helpers --------------------------------------------------------------------------------------------------------------------------------
def test_churn_and_centroids_on_hand_made_inputs():
    churn = image.summary_churn(np.array([[5, 1, 2, 2], [0, 0, 0, 0], [0, 3, 0, 0], [4, 0, 0, 4]], np.uint64))
    assert churn.dtype == np.float64 and churn.shape == (4,)
    assert churn[0] == pytest.approx(0.3) and math.isnan(churn[1]) and churn[2] == 1.0 and churn[3] == 0.0
    assert image.summary_churn(np.arange(9, dtype=np.uint64)) == pytest.approx(1 - (0 + 4 + 8) / 36.0)
    with pytest.raises(ValueError, match="ncls"):
        image.summary_churn(np.zeros((2, 5), np.uint64))
    c = image.summary_centroids(np.array([[[4, 10, 2], [0, 0, 0], [1 << 20, 8589672448, 3 << 20]]], np.uint64))
    assert c.dtype == np.float64 and c.shape == (1, 3, 2)
    assert c[0, 0].tolist() == [2.5, 0.5] and np.isnan(c[0, 1]).all() and c[0, 2].tolist() == [8589672448 / float(1 << 20), 3.0]
    # the temporal IoU is per_class_iu of the square matrix, as it stands
    from accel_amd.core import results
    assert results.summary_churn is image.summary_churn and results.summary_centroids is image.summary_centroids
    iu = results.per_class_iu(np.array([5, 1, 2, 2], np.uint64).reshape(2, 2))
    assert iu.tolist() == [5 / 8.0, 2 / 5.0]


def test_argument_errors_of_the_specification():
    a = np.zeros((1, 16, 16), np.uint8)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="ncls"):
            image.labels_summary_host(a, 16, 16, 16, 16, bad)
    with pytest.raises(ValueError, match="out_h"):
        image.labels_summary_host(a, 17, 16, 16, 16, 19)
    with pytest.raises(ValueError, match="out_h"):
        image.labels_summary_host(a, 16, 0, 16, 16, 19)
    with pytest.raises(ValueError, match="h x w"):
        image.labels_summary_host(a, 16, 16, 0, 16, 19)
    with pytest.raises(ValueError, match="h x w"):
        image.labels_summary_host(a, 16, 16, 16, 32769, 19)
    with pytest.raises(ValueError, match="prev"):
        image.labels_summary_host(a, 16, 16, 20, 20, 19, prev=np.zeros((1, 16, 16), np.uint8))
    with pytest.raises(ValueError, match="labels"):
        image.labels_summary_host(np.zeros((1, 1, 16, 16), np.uint8), 16, 16, 16, 16, 19)
    one = image.labels_summary_host(a[0], 16, 16, 16, 16, 2)                  # a single map is a batch of one
    assert one[0].tolist() == [[[256, 120 * 16, 120 * 16], [0, 0, 0]]] and one[1].tolist() == [[[0, 0, 15, 15], [16, 16, -1, -1]]]
