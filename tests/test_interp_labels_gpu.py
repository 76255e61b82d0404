"""Labels from interpolated scores on the GPU (csrc/scores_labels.hip behind accel_scores_labels and the accel_model_scores_* forms): every label is
what utils.image.labels_interpolated_host gives -- EXACTLY.  The blend is float64 on both sides with every operation rounded on its own, the inputs
come from interp_ref.py, whose guard condition (test_interp_labels_cpu.py::test_guard_condition_of_the_gpu_inputs) says that no label of them can
depend on the last bits of a sum, and the dyadic cases are exact, ties included.  So every comparison is np.array_equal: no tolerance.
(Host side, and the mutants these cases tell apart: test_interp_labels_cpu.py.)"""
import ctypes

import numpy as np
import pytest

from accel_amd.utils import image, synth

import interp_ref as ref
from test_frames_u8_gpu import SMALL
from test_results_gpu import PALETTE, STRIDE, _check_rows, _fast_hist, _geo, _pitched, _pitches, _steps

pytestmark = pytest.mark.gpu


def _run(ctx, case, **kw):
    return ctx.scores_labels(ref.scores(case), case.out_h, case.out_w, case.h, case.w, **kw)


def _check(got, case):
    want = ref.reference(case)
    assert got.dtype == np.uint8 and got.shape == (case.n, case.h, case.w)
    assert np.array_equal(got, want), (ref.ident(case), int(np.count_nonzero(got != want)))


# ---- 1. operator level: every case of the table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ncls", ref.NCLS)
@pytest.mark.parametrize("rows,cols,target,max_size", SMALL)
def test_labels_equal_the_host_restatement(ctx, rows, cols, target, max_size, ncls, n):
    for case in ref.operator_cases(rows, cols, target, max_size, ncls, n):
        _check(_run(ctx, case), case)


@pytest.mark.parametrize("case", ref.near_tie_cases(), ids=ref.ident)
def test_near_ties_are_decided_in_float64(ctx, case):
    got = _run(ctx, case)
    assert (got[0] == 11).all() and (got[1] == 5).all(), (int(np.count_nonzero(got[0] != 11)), int(np.count_nonzero(got[1] != 5)))
    _check(got, case)


@pytest.mark.parametrize("case", ref.dyadic_cases(), ids=ref.ident)
def test_dyadic_known_answers(ctx, case):
    got = _run(ctx, case)
    assert np.array_equal(got, ref.integer_labels(case)), ref.ident(case)
    if case.kind == "step" and case.h == 16:
        assert got[0, 3, 10] == 0 and got[0, 3, 11] == 1          # the pixel at value 1 ties and takes class 0
    _check(got, case)


@pytest.mark.parametrize("case", ref.crop_cases(), ids=ref.ident)
def test_crops_of_widths_not_divisible_by_four(ctx, case):
    _check(_run(ctx, case), case)


@pytest.mark.parametrize("case", ref.multiblock_cases(), ids=ref.ident)
def test_more_than_one_block_per_frame(ctx, case):
    _check(_run(ctx, case), case)


def test_full_size_720p_from_its_bound_size(ctx):
    case = ref.full_case()
    assert (case.H, case.W, case.out_h, case.out_w) == (1024, 1824, 1024, 1820)
    _check(_run(ctx, case), case)


# ---- 2. pitched destinations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.pitched_cases(), ids=ref.ident)
def test_pitched_destinations_keep_the_bytes_between_rows(ctx, case):
    want = ref.reference(case)
    for pitch in _pitches(case.w)[1:]:
        out = _pitched(np.zeros((case.n, case.h, case.w), np.uint8), pitch, pitch)
        before = out.copy()
        assert _run(ctx, case, out=out) is out
        _check_rows(out, before, want, "pitch %d" % pitch)


# ---- 3. the identity geometry is the nearest rule's -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ref.small_case(*SMALL[0], ncls=k, n=3, scale=1.0) for k in ref.NCLS] + ref.crop_cases()[:2] + [ref.multiblock_cases()[1]],
                         ids=ref.ident)
def test_identity_equals_labels_to_source_of_the_argmax(ctx, case):
    assert (case.h, case.w) == (case.out_h, case.out_w)
    s = ref.scores(case)
    labels = np.concatenate([ctx.argmax_c(s[i:i + 1]) for i in range(case.n)])          # one frame per call
    assert np.array_equal(labels, np.argmax(s, axis=1))
    want = ctx.labels_to_source(labels, case.out_h, case.out_w, case.h, case.w)
    assert np.array_equal(_run(ctx, case), want)


# ---- 4. model level ----------------------------------------------------------------------------------------------------------------------------------------
def test_finishing_calls_on_accel18_with_interpolation(demo_cfg):
    """Accel-18 at 128 x 256 on the synthetic clip, raw frames of 90 x 180 (the map is resampled): the logits of a key and a non-key frame are
    finished on the GPU with interpolate=True; the calls change nothing -- not the generations, not the buffers, not what the captured graphs
    compute next, not the default path"""
    import torch
    from accel_amd import demo, runtime
    from accel_amd.core import results, tester
    H, W, rows, cols = 128, 256, 90, 180
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = STRIDE
    out_h, out_w = _geo(rows, cols, H, W)[:2]
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    frames = synth.make_clip(rows, cols, 3)
    rng = np.random.default_rng(rows)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        raw = demo.build_batches(frames, demo_cfg, raw=True)
        base = _steps(r, raw, 3, 3)                      # frames 0 (key), 1, 2 (non-key) without any finishing call
        ev = results.Evaluator(19)
        total = np.zeros((19, 19), np.int64)
        kept = None
        for i in (0, 1):
            lg, lab = r.step(i, raw[i], 3)
            m = lg.device_ref[0]
            gen = m.generation("labels"), m.generation("logits")
            logits0, labels0 = m.read("logits", (1, 19, H, W)), m.read("labels", (1, H, W), np.uint8)
            assert np.array_equal(logits0, base[i][0]) and np.array_equal(labels0, base[i][1])
            want = image.labels_interpolated_host(lg.asnumpy(), out_h, out_w, rows, cols)
            nearest = image.labels_to_source_host(labels0, out_h, out_w, rows, cols)
            # a fresh result, through the handle; a dict names the same geometry
            got = results.labels_at_source(lg, raw[i][0], interpolate=True)
            assert got.dtype == np.uint8 and got.shape == (1, rows, cols)
            assert np.array_equal(got, want), int(np.count_nonzero(got != want))
            assert np.array_equal(results.labels_at_source(lg, dict(raw[i][0].geometry, h=rows, w=cols), interpolate=True), want)
            # pitched host rows and pitched rows in HBM
            for pitch in _pitches(cols)[1:]:
                out = _pitched(np.zeros((1, rows, cols), np.uint8), pitch, pitch)
                before = out.copy()
                assert m.scores_labels(1, out_h, out_w, rows, cols, out=out) is out
                _check_rows(out, before, want, "host pitch %d" % pitch)
            dp = cols + 7
            dev = torch.full((1, rows, dp), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            m.scores_labels_device(dev.data_ptr(), 1, out_h, out_w, rows, cols, dp)
            m.ctx.sync()
            host = dev.cpu().numpy()
            assert np.array_equal(host[:, :, :cols], want) and (host[:, :, cols:] == 7).all()
            # the confusion matrix and the colour image of those labels
            gt = rng.integers(0, 19, (rows, cols), dtype=np.uint8)
            gt[rng.integers(0, 4, gt.shape) == 0] = 255
            ev.add(lg, gt, like=raw[i][0], interpolate=True)
            total += _fast_hist(want, gt, 19)
            assert np.array_equal(ev.hist(), total)
            col = results.colour(lg, raw[i][0], PALETTE, frames=True, alpha=128, interpolate=True)
            assert np.array_equal(col, image.colour_host(want, PALETTE, frames=frames[i][None], alpha=128))
            assert np.array_equal(results.colour(lg, raw[i][0], PALETTE, rgb=False, interpolate=True), image.colour_host(want, PALETTE, rgb=False))
            # a label handle is not a logits handle, and the other way round on the default path
            for call in (lambda: results.labels_at_source(lab, raw[i][0], interpolate=True), lambda: ev.add(lab, gt, like=raw[i][0], interpolate=True),
                         lambda: results.colour(lab, raw[i][0], PALETTE, interpolate=True)):
                with pytest.raises(runtime.AccelError, match="logits"):
                    call()
            assert np.array_equal(ev.hist(), total)
            # nothing was written: generations, labels and logits are what they were
            assert (m.generation("labels"), m.generation("logits")) == gen
            assert np.array_equal(m.read("logits", (1, 19, H, W)), logits0) and np.array_equal(m.read("labels", (1, H, W), np.uint8), labels0)
            # the default path is untouched, and adds into the same accumulator
            assert np.array_equal(results.labels_at_source(lab, raw[i][0]), nearest)
            assert np.array_equal(results.colour(lab, raw[i][0], PALETTE), image.colour_host(nearest, PALETTE))
            ev.add(lab, gt, like=raw[i][0])
            total += _fast_hist(nearest, gt, 19)
            assert np.array_equal(ev.hist(), total)
            kept = lg
        # the captured graphs are undisturbed: the next step gives what the run without finishing calls gave
        lg, lab = r.step(2, raw[2], 3)
        assert np.array_equal(lg.asnumpy(), base[2][0]) and np.array_equal(lab.asnumpy(), base[2][1])
        # a logits handle kept across that step names a buffer that has been rewritten: never read
        for call in (lambda: results.labels_at_source(kept, raw[1][0], interpolate=True),
                     lambda: ev.add(kept, np.zeros((rows, cols), np.uint8), like=raw[1][0], interpolate=True),
                     lambda: results.colour(kept, raw[1][0], PALETTE, interpolate=True)):
            with pytest.raises(runtime.AccelError, match="stale"):
                call()
        assert np.array_equal(ev.hist(), total)
    finally:
        tester.release_models()


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------------------------
def _logits_model(ctx, n, ncls, H, W):
    """a model that owns a `logits` buffer of n x ncls x H x W and says so (no op: nothing is ever run)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=logits bytes=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d\n"
                     % (n * ncls * H * W * 4, n, ncls, H, W))
    return m


def test_argument_errors_return_err_arg(ctx):
    """every call the kernel could not honour is refused on the host, with a message that names the argument; nothing is launched and the model is
    what it was"""
    from accel_amd import runtime
    lib = runtime.lib()
    n, ncls, H, W, rows, cols = 2, 19, 32, 64, 29, 50
    out_h, out_w = 31, 54
    case = ref.Case("normal", n, ncls, H, W, out_h, out_w, rows, cols, 1.0, 9)
    scores = ref.scores(case)
    rng = np.random.default_rng(3)
    gt = rng.integers(0, 19, (n, rows, cols), dtype=np.uint8)
    frame = rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)
    pal = np.ascontiguousarray(PALETTE.reshape(-1))
    dst, dst3 = np.zeros((n, rows, cols), np.uint8), np.zeros((n, rows, cols, 3), np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(scores=vp(scores), n=n, ncls=ncls, H=H, W=W, out_h=out_h, out_w=out_w, h=rows, w=cols, dst=vp(dst), dst_pitch=cols, gt=vp(gt),
                gt_pitch=cols, hncls=19, pal=vp(pal), frame=vp(frame), frame_pitch=3 * cols, alpha=128, dst3=vp(dst3), dst3_pitch=3 * cols)
    m = _logits_model(ctx, n, ncls, H, W)
    odd = _logits_model(ctx, 1, 7, 16, 16)                     # a class count the kernel is not built for
    try:
        m.write("logits", scores)
        m.scores_hist_add(gt, out_h, out_w, 19)
        state = m.generation("logits"), m.hist_read(19)
        calls = {
            "op": lambda a: lib.accel_scores_labels(ctx.handle, a["scores"], a["n"], a["ncls"], a["H"], a["W"], a["out_h"], a["out_w"], a["h"], a["w"],
                                                    a["dst"], a["dst_pitch"]),
            "labels": lambda a: lib.accel_model_scores_labels(m.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], a["dst"], a["dst_pitch"], 0),
            "hist": lambda a: lib.accel_model_scores_hist_add(m.handle, a["gt"], a["n"], a["h"], a["w"], a["gt_pitch"], a["out_h"], a["out_w"], a["hncls"], 0),
            "colour": lambda a: lib.accel_model_scores_colour(m.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], a["pal"], 1, a["frame"],
                                                              a["frame_pitch"], a["alpha"], 0, a["dst3"], a["dst3_pitch"], 0),
        }
        every, model = tuple(calls), ("labels", "hist", "colour")
        cases = [(dict(scores=None), "scores", ("op",)), (dict(dst=None), "dst", ("op", "labels")), (dict(dst3=None), "dst", ("colour",)),
                 (dict(gt=None), "gt", ("hist",)), (dict(pal=None), "palette_rgb", ("colour",)),
                 (dict(n=0), "n =", every), (dict(n=-1), "n =", every), (dict(h=0), "h =", every), (dict(w=0), "w =", every), (dict(h=32769), "h =", every),
                 (dict(w=32769), "w =", every), (dict(H=0), "H x W", ("op",)), (dict(W=32769), "H x W", ("op",)),
                 (dict(out_h=0), "out_h", every), (dict(out_w=0), "out_w", every), (dict(out_h=H + 1), "out_h", every), (dict(out_w=W + 1), "out_w", every),
                 (dict(dst_pitch=cols - 1), "dst_pitch", ("op", "labels")), (dict(gt_pitch=cols - 1), "gt_pitch", ("hist",)),
                 (dict(dst3_pitch=3 * cols - 1), "dst_pitch", ("colour",)), (dict(frame_pitch=3 * cols - 1), "frame_pitch", ("colour",)),
                 (dict(ncls=0), "ncls", ("op",)), (dict(ncls=3), "ncls", ("op",)), (dict(ncls=20), "ncls", ("op",)), (dict(ncls=32), "ncls", ("op",)),
                 (dict(hncls=0), "ncls", ("hist",)), (dict(hncls=33), "ncls", ("hist",)),
                 (dict(hncls=21), "ncls", ("hist",)),                                  # the accumulator holds 19 classes since its last clear
                 (dict(alpha=-1), "alpha", ("colour",)), (dict(alpha=257), "alpha", ("colour",)),
                 (dict(n=n + 1), "n =", model)]                                        # larger than the bound batch
        for change, word, names in cases:
            for name in names:
                rc = calls[name](dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (name, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg, (name, change, msg)
        assert lib.accel_scores_labels(None, vp(scores), n, ncls, H, W, out_h, out_w, rows, cols, vp(dst), cols) == -1
        assert lib.accel_model_scores_labels(None, n, out_h, out_w, rows, cols, vp(dst), cols, 0) == -1
        assert lib.accel_model_scores_hist_add(None, vp(gt), n, rows, cols, cols, out_h, out_w, 19, 0) == -1
        assert lib.accel_model_scores_colour(None, n, out_h, out_w, rows, cols, vp(pal), 1, None, 0, 256, 0, vp(dst3), 3 * cols, 0) == -1
        assert lib.accel_model_scores_labels(odd.handle, 1, 16, 16, 16, 16, vp(dst), 16, 0) == -1 and "ncls" in lib.accel_last_error().decode()
        bare = runtime.Model(ctx)                               # a model without logits
        for call in (lambda: lib.accel_model_scores_labels(bare.handle, 1, 8, 8, 8, 8, vp(dst), 8, 0),
                     lambda: lib.accel_model_scores_hist_add(bare.handle, vp(gt), 1, 8, 8, 8, 8, 8, 19, 0),
                     lambda: lib.accel_model_scores_colour(bare.handle, 1, 8, 8, 8, 8, vp(pal), 1, None, 0, 256, 0, vp(dst3), 24, 0)):
            assert call() == -1 and "logits" in lib.accel_last_error().decode()
        bare.close()
        # none of the refused calls reached the model or the destinations
        assert m.generation("logits") == state[0] and np.array_equal(m.read("logits", (n, ncls, H, W)), scores)
        assert np.array_equal(m.hist_read(19), state[1])
        assert not dst.any() and not dst3.any()
        want = ref.reference(case)
        assert np.array_equal(state[1].astype(np.int64), _fast_hist(want, gt, 19))
        for name in every:                                      # and every call is accepted as it stands
            dst[...] = 0
            assert calls[name](good) == 0, (name, lib.accel_last_error().decode())
            if name in ("op", "labels"):
                assert np.array_equal(dst, want), name
        assert np.array_equal(dst3, image.colour_host(want, PALETTE, frames=frame, alpha=128))
        assert np.array_equal(m.hist_read(19), 2 * state[1])
        assert m.generation("logits") == state[0]
    finally:
        ctx.sync()
        m.close()
        odd.close()


def test_demo_interpolates_the_labels_of_raw_frames(demo_cfg, capsys, tmp_path):
    """90 x 180 frames bound at 128 x 256 with --interpolate: the loop fetches source-size labels and writes them as PNGs"""
    from PIL import Image
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "3", "--num_ex", "1", "--synthetic", "90x180", "--scales", "128x256", "--raw-frames",
                   "--finish-on-gpu", "--interpolate", "--out", str(tmp_path)])
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    assert out.rstrip().endswith("done") and out.count("testing synthetic_") == 3, out[-1500:]
    pngs = sorted(tmp_path.glob("seg_*.png"))
    assert len(pngs) == 3 and Image.open(str(pngs[0])).size == (180, 90)
