"""Frame change, host side: utils.image.frame_signature_host / frame_change_host -- the integer specification the GPU kernel is tested against --
equal a scalar, loop-per-pixel restatement; the case table of frame_change_ref.py tells each of a list of plausible wrong kernels from the right one;
the key-frame schedules decide as documented; and the C ABI declares and exports the entry points.  (GPU side: test_frame_change_gpu.py.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

import frame_change_ref as ref

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("accel_frame_change", "accel_model_frame_change", "accel_model_frame_keep")


def test_header_declares_and_library_exports_the_entry_points():
    from accel_amd import runtime
    hdr = open(os.path.join(ROOT, "include", "accel_hip.h")).read()
    declared = set(re.findall(r"\b(accel_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, "include/accel_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libaccel_hip.so does not export %s" % name
    runtime.lib()
    assert set(ENTRY_POINTS) <= set(runtime.EXPORTS)
    assert len(runtime.EXPORTS["accel_frame_change"]) == 15 and len(runtime.EXPORTS["accel_model_frame_change"]) == 13
    assert hasattr(runtime.Context, "frame_change")
    assert hasattr(runtime.Model, "frame_change") and hasattr(runtime.Model, "frame_keep")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


# ---- the specification against a scalar restatement --------------------------------------------------------------------------------------------
def _q_scalar(x):
    """one value, in Python floats: an fp32 is exact as a double, so is its product with 8, and round() rounds half to even"""
    if x != x:
        return -4096                       # fmax(NaN, -512) = -512
    return int(round(min(max(x, -512.0), 512.0) * 8.0))


def _signature_scalar(x, out_h, out_w, cell):
    n = x.shape[0]
    gh, gw = -(-out_h // cell), -(-out_w // cell)
    sig = [[[0] * gw for _ in range(gh)] for _ in range(n)]
    planes = x.astype(np.float64).tolist()
    for f in range(n):
        r, g, b = planes[f]
        for y in range(out_h):
            row, rr, gr, br = sig[f][y // cell], r[y], g[y], b[y]
            for c in range(out_w):
                row[c // cell] += 2 * _q_scalar(rr[c]) + 5 * _q_scalar(gr[c]) + _q_scalar(br[c])
    return sig


def _change_scalar(sig, key, out_h, out_w, cell, level_q):
    n, gh, gw = len(sig), len(sig[0]), len(sig[0][0])
    changed, sad, mask = [0] * n, [0] * n, np.zeros((n, gh, gw), np.uint8)
    for f in range(n):
        for cy in range(gh):
            for cx in range(gw):
                d = abs(sig[f][cy][cx] - key[f][cy][cx])
                area = min(cell, out_h - cy * cell) * min(cell, out_w - cx * cell)
                sad[f] += d
                if d > level_q * area:
                    changed[f] += 1
                    mask[f, cy, cx] = 1
    return changed, sad, mask


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_the_specification_equals_a_scalar_restatement(case):
    s = case.shape
    cur, key = ref.frames(case)
    want = ref.expected(case)
    a, b = _signature_scalar(cur, s.out_h, s.out_w, s.cell), _signature_scalar(key, s.out_h, s.out_w, s.cell)
    assert want.sig.dtype == np.int32 and want.sig.tolist() == a and want.sig_key.tolist() == b
    changed, sad, mask = _change_scalar(a, b, s.out_h, s.out_w, s.cell, case.level_q)
    assert want.changed.dtype == np.uint32 and want.sad.dtype == np.uint64 and want.mask.dtype == np.uint8
    assert want.changed.tolist() == changed and want.sad.tolist() == sad and np.array_equal(want.mask, mask)
    assert int(np.abs(want.sig.astype(np.int64)).max()) <= 1 << 27


def test_the_largest_signature_is_reached_and_fits():
    case = next(c for c in ref.CASES if c.values == "max")
    want = ref.expected(case)
    assert int(want.sig.max()) == 8 * 4096 * 64 * 64 == 1 << 27 and int(want.sig_key.min()) == -(1 << 27)
    assert int(want.sad.max()) == (1 << 29) + (1 << 22)        # two whole cells and one a pixel wide: 64-bit sums
    assert want.mask.all()


def test_the_table_sits_on_the_threshold():
    """the dyadic pairs: cells at exactly d == level_q * area (not changed) beside cells one unit above (changed), edge cells among them"""
    for case in (c for c in ref.CASES if c.values == "dyadic"):
        s, want = case.shape, ref.expected(case)
        d = np.abs(want.sig.astype(np.int64) - want.sig_key.astype(np.int64))
        limit = case.level_q * image.frame_cell_areas(s.out_h, s.out_w, s.cell)[None]
        assert (d == limit).any() and (d == limit + 1).any(), ref.case_id(case)
        assert not want.mask[d == limit].any() and want.mask[d == limit + 1].all()
    for case in ref.CASES:                                   # and every random pair has cells of both outcomes somewhere in the table
        want = ref.expected(case)
        assert want.sad.min() > 0, ref.case_id(case)
    mixed = [c for c in ref.CASES if 0 < ref.expected(c).mask.sum() < ref.expected(c).mask.size]
    assert len(mixed) >= len(ref.SHAPES)


def test_nan_and_infinities_follow_c_fmax_and_fmin():
    x = np.zeros((1, 3, 8, 8), np.float32)
    for value, q in ((np.nan, -4096), (np.inf, 4096), (-np.inf, -4096), (3e38, 4096), (600.0, 4096), (-600.0, -4096), (0.0625, 0), (0.1875, 2), (-0.0625, 0)):
        x[0, 2, 3, 3] = value                               # the B plane: weight 1
        assert image.frame_signature_host(x, 8, 8, 8)[0, 0, 0] == q, value


def test_level_and_argument_errors_of_the_specification():
    assert image.frame_level_q(16.0) == 1024 and image.frame_level_q(0) == 0 and image.frame_level_q(512) == 32768
    for bad in (-0.01, 512.01):
        with pytest.raises(ValueError, match="level"):
            image.frame_level_q(bad)
    x = np.zeros((1, 3, 16, 16), np.float32)
    with pytest.raises(ValueError, match="cell"):
        image.frame_signature_host(x, 16, 16, 12)
    with pytest.raises(ValueError, match="out_h"):
        image.frame_signature_host(x, 17, 16, 8)
    sig = image.frame_signature_host(x, 16, 16, 8)
    with pytest.raises(ValueError, match="level_q"):
        image.frame_change_host(sig, sig, 16, 16, 8, 32769)
    with pytest.raises(ValueError, match="signatures"):
        image.frame_change_host(sig, sig[:, :1], 16, 16, 8, 0)
    assert image.frame_cells(37, 70, 16) == (3, 5)
    assert image.frame_cell_areas(37, 70, 16).tolist() == [[256] * 4 + [96], [256] * 4 + [96], [80] * 4 + [30]]


# ---- wrong kernels: the table tells each of them from the right one ----------------------------------------------------------------------------------
def _variant(case, flaw=None):
    """(sig, changed, sad, mask) of the case as a kernel with one flaw would compute them, in numpy; flaw=None: the right kernel"""
    s = case.shape
    out = []
    for x in ref.frames(case):
        h, w = (s.H, s.W) if flaw == "padded" else (s.out_h, s.out_w)
        v = x[:, :, :h, :w].astype(np.float64)
        if flaw == "no_clamp":                               # finite values go through as they are (non-finite ones as the right kernel has them)
            v = np.where(np.isfinite(v) & (np.abs(v) < 1e6), v, np.fmin(np.fmax(v, -512.0), 512.0))
        else:
            v = np.fmin(np.fmax(v, -512.0), 512.0)
        v = v * 8.0
        if flaw == "truncate":
            q = np.trunc(v)
        elif flaw == "half_away":
            q = np.sign(v) * np.floor(np.abs(v) + 0.5)
        else:
            q = np.rint(v)
        q = q.astype(np.int64)
        wr, wb = (1, 2) if flaw == "swap_rb" else (2, 1)
        px = wr * q[:, 0] + 5 * q[:, 1] + wb * q[:, 2]
        gh, gw = -(-h // s.cell), -(-w // s.cell)
        full = np.zeros((s.n, gh * s.cell, gw * s.cell), np.int64)
        full[:, :h, :w] = px
        sums = full.reshape(s.n, gh, s.cell, gw, s.cell).sum(axis=(2, 4))
        g = image.frame_cells(s.out_h, s.out_w, s.cell)
        out.append(sums[:, :g[0], :g[1]])
    sig, key = out
    if flaw == "kept_frame_0":
        key = np.broadcast_to(key[:1], key.shape)
    d = np.abs(sig - key)
    area = np.full(sig.shape[1:], s.cell * s.cell, np.int64) if flaw == "full_area" else image.frame_cell_areas(s.out_h, s.out_w, s.cell)
    mask = d >= case.level_q * area if flaw == "greater_equal" else d > case.level_q * area
    changed, sad = mask.sum(axis=(1, 2)), d.sum(axis=(1, 2))
    if flaw == "mask_transposed":
        mask = np.ascontiguousarray(mask.transpose(0, 2, 1)).reshape(mask.shape)
    return sig.astype(np.int32), changed.astype(np.uint32), sad.astype(np.uint64), mask.astype(np.uint8)


def _differs(case, flaw):
    want = ref.expected(case)
    got = _variant(case, flaw)
    return not all(np.array_equal(a, b) for a, b in zip(got, (want.sig, want.changed, want.sad, want.mask)))


def test_the_variant_without_a_flaw_is_the_specification():
    assert not any(_differs(case, None) for case in ref.CASES)


@pytest.mark.parametrize("flaw", ["truncate", "half_away", "no_clamp", "swap_rb", "full_area", "greater_equal", "padded", "kept_frame_0", "mask_transposed"])
def test_the_table_tells_a_wrong_kernel_from_the_right_one(flaw):
    caught = [ref.case_id(case) for case in ref.CASES if _differs(case, flaw)]
    assert caught, "no case of the table notices a kernel with the flaw '%s'" % flaw


# ---- the schedules -------------------------------------------------------------------------------------------------------------------------------
def _keys(schedule, measures):
    """the key frames a schedule takes over frames 0 .. len(measures) - 1, fed the measure of each frame: None, or a list of changed counts of
    100 cells per frame of the call; as ClipRunner does, a schedule that does not look at frames is not given any"""
    out = []
    for idx, m in enumerate(measures):
        change = None if m is None or not schedule.needs_change else [(c, 100, 0) for c in m]
        if schedule.decide(idx, change):
            out.append(idx)
    return out


def test_fixed_and_explicit_schedules():
    from accel_amd.core.schedule import KeySchedule
    for interval in (1, 2, 3, 5):
        s = KeySchedule.fixed(interval)
        assert not s.needs_change
        assert _keys(s, [None] * 12) == [i for i in range(12) if i % interval == 0]
    s = KeySchedule.explicit([0, 3, 4, 9])
    assert not s.needs_change and _keys(s, [None] * 12) == [0, 3, 4, 9]
    with pytest.raises(ValueError, match="interval"):
        KeySchedule.fixed(0)
    with pytest.raises(ValueError, match="frame 0"):
        KeySchedule.explicit([2, 4])


def test_adaptive_schedule():
    from accel_amd.core.schedule import KeySchedule
    quiet = [None] + [[0]] * 11
    s = KeySchedule.adaptive(0.25, max_interval=5)
    assert s.needs_change and s.level_q == 1024 and s.cell == 32
    assert _keys(s, quiet) == [0, 5, 10]                                            # the longest distance
    busy = [None, [0], [26], [0], [0], [25], [0], [0], [30], [30], [0], [0]]
    assert _keys(KeySchedule.adaptive(0.25, max_interval=5), busy) == [0, 2, 7, 8, 9]        # 25 of 100 is not MORE than a quarter; 26 is
    assert _keys(KeySchedule.adaptive(0.25, max_interval=5, min_interval=3), busy) == [0, 5, 8]      # 26 at distance 2 and 30 at distance 1 wait
    assert _keys(KeySchedule.adaptive(1.0, max_interval=4), [None] + [[100]] * 8) == [0, 4, 8]      # a share of 1 can never be exceeded
    assert _keys(KeySchedule.adaptive(0.0, max_interval=4), [None, [0], [1], [0], [0], [0], [0]]) == [0, 2, 6]      # a share of 0: any changed cell
    # a batch: ANY frame of the call
    batch = [None, [0, 0, 0], [0, 26, 0], [0, 0, 0], [25, 25, 25], [0, 0, 27]]
    assert _keys(KeySchedule.adaptive(0.25, max_interval=9), batch) == [0, 2, 5]
    # nothing to compare with (no kept signature of this geometry): a key frame
    assert _keys(KeySchedule.adaptive(0.25, max_interval=9), [None, [0], None, [0]]) == [0, 2]
    # indices that start over: a new clip starts with a key frame
    s = KeySchedule.adaptive(0.25, max_interval=9)
    assert [s.decide(i, c) for i, c in ((0, None), (1, [(0, 100, 0)]), (0, [(0, 100, 0)]), (1, [(0, 100, 0)]))] == [True, False, True, False]
    for bad in (dict(share=1.5), dict(share=-0.1), dict(share=0.5, cell=12), dict(share=0.5, level=600), dict(share=0.5, max_interval=0),
                dict(share=0.5, max_interval=3, min_interval=4)):
        with pytest.raises(ValueError):
            KeySchedule.adaptive(**bad)


def test_inputs_without_identity_are_refused_by_the_adaptive_schedule(demo_cfg):
    """plain numpy inputs carry no uid: they could not be recognised as staged, and the runner says so before anything touches the GPU"""
    from accel_amd import demo
    from accel_amd.core.schedule import KeySchedule

    class Staged(Exception):
        pass

    class NoPredictor(object):
        def stage(self, batch):
            raise Staged()

    runner = demo.ClipRunner.__new__(demo.ClipRunner)        # the decision needs no bound predictor
    runner.cur_predictor = runner.key_predictor = NoPredictor()
    runner.last_key = runner.last_change = runner.feat = None
    x = np.zeros((1, 3, 32, 64), np.float32)
    zero = np.zeros((1, 2048, 1, 1), np.float32)
    with pytest.raises(ValueError, match="without identity"):
        runner.step(0, [x, x, zero], 5, schedule=KeySchedule.adaptive(0.25))
    from accel_amd import mx
    a = mx.nd.array(x)
    with pytest.raises(ValueError, match="data_key"):
        runner.step(0, [a, x, zero], 5, schedule=KeySchedule.adaptive(0.25))
    with pytest.raises(Staged):                                # arrays with identity get as far as the staging
        runner.step(0, [a, a, zero], 5, schedule=KeySchedule.adaptive(0.25))
