"""Per-pixel confidence on the GPU (csrc/confidence.hip behind accel_scores_confidence / accel_model_confidence): conf, second and hist are
what utils.image.confidence_host gives -- EXACTLY -- and margin is bit for bit.  conf is float64 arithmetic on both sides; the inputs come from
confidence_ref.py, whose guard condition (test_confidence_cpu.py::test_guard_condition_of_the_gpu_inputs) says that no byte of them can depend on
the last bits of an exp.  So every comparison is np.array_equal: no tolerance.  (Host side: test_confidence_cpu.py.)"""
import ctypes

import numpy as np
import pytest

from accel_amd.utils import image, synth

import confidence_ref as ref
from test_frames_u8_gpu import SMALL
from test_results_gpu import _pitches, _steps

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(ctx, case, **kw):
    return ctx.scores_confidence(ref.scores(case), case.out_h, case.out_w, case.h, case.w, is_prob=ref.is_prob(case), **kw)


def _check(got, case, what=""):
    conf, margin, second, hist = got
    wc, wm, ws, wh = ref.reference(case)
    assert conf.dtype == np.uint8 and conf.shape == (case.n, case.h, case.w)
    assert margin.dtype == np.float32 and second.dtype == np.uint8 and hist.dtype == np.uint64 and hist.shape == (case.n, 256)
    assert np.array_equal(conf, wc), (what, case, "conf", int(np.count_nonzero(conf != wc)))
    assert np.array_equal(second, ws), (what, case, "second", int(np.count_nonzero(second != ws)))
    assert np.array_equal(_bits(margin), _bits(wm)), (what, case, "margin", int(np.count_nonzero(_bits(margin) != _bits(wm))))
    assert np.array_equal(hist, wh), (what, case, "hist")


# ---- 1. operator level over the small geometries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ncls", ref.NCLS)
@pytest.mark.parametrize("rows,cols,target,max_size", SMALL)
def test_confidence_equals_the_host_restatement(ctx, rows, cols, target, max_size, ncls, n):
    for case in ref.operator_cases(rows, cols, target, max_size, ncls, n):
        _check(_run(ctx, case), case, "scale %g" % case.scale)


# ---- 2. tight and pitched destinations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.pitched_cases(), ids=lambda c: "%dx%d" % (c.h, c.w))
def test_pitched_destinations_keep_the_bytes_between_rows(ctx, case):
    wc, wm, ws, wh = ref.reference(case)
    n, h, w = case.n, case.h, case.w
    margin_pitches = [(p + 3) // 4 * 4 for p in _pitches(4 * w)]           # bytes, multiples of 4
    for pitch, mpitch in zip(_pitches(w), margin_pitches):
        rng = np.random.default_rng(pitch)
        conf = rng.integers(1, 256, (n, h, pitch), dtype=np.uint8)
        second = rng.integers(1, 256, (n, h, pitch), dtype=np.uint8)
        margin = rng.integers(1, 1 << 30, (n, h, mpitch // 4), dtype=np.uint32).view(np.float32)
        before = conf.copy(), second.copy(), margin.copy()
        got = ctx.scores_confidence(ref.scores(case), case.out_h, case.out_w, h, w, conf=conf, margin=margin, second=second)
        assert got[0] is conf and got[1] is margin and got[2] is second
        assert np.array_equal(conf[:, :, :w], wc) and np.array_equal(conf[:, :, w:], before[0][:, :, w:]), pitch
        assert np.array_equal(second[:, :, :w], ws) and np.array_equal(second[:, :, w:], before[1][:, :, w:]), pitch
        assert np.array_equal(_bits(margin[:, :, :w]), _bits(wm)) and np.array_equal(_bits(margin[:, :, w:]), _bits(before[2][:, :, w:])), mpitch
        assert np.array_equal(got[3], wh)


# ---- 3. each output alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.pitched_cases(), ids=lambda c: "%dx%d" % (c.h, c.w))
def test_each_output_alone_equals_the_all_together_call(ctx, case):
    together = _run(ctx, case)
    _check(together, case)
    for i, name in enumerate(("conf", "margin", "second", "hist")):
        only = dict(conf=False, margin=False, second=False, hist=False)
        only[name] = True
        got = _run(ctx, case, **only)
        assert [g is not None for g in got] == [j == i for j in range(4)], name
        a, b = got[i], together[i]
        assert a.dtype == b.dtype and np.array_equal(_bits(a) if name == "margin" else a, _bits(b) if name == "margin" else b), name


# ---- 4. widths not divisible by four -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", ref.CROPS)
def test_crops_of_widths_not_divisible_by_four(ctx, rows, cols):
    case = ref.crop_case(rows, cols)
    _check(_run(ctx, case), case)


# ---- 5. known answers --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.known_cases(), ids=lambda c: "%s-ncls%d-%dx%d" % (c.kind, c.ncls, c.h, c.w))
def test_known_answers(ctx, case):
    conf, margin, second, hist = _run(ctx, case)
    pixels = case.h * case.w
    if case.kind == "equal":            # p = 1 / ncls; two equal classes of two: exactly 128
        level = {2: 128, 19: 13, 21: 12}[case.ncls]
        assert (conf == level).all() and (margin == 0).all() and (second == 1).all()
    elif case.kind == "one100":         # p = 1 -> 256, clamped
        level = 255
        assert (conf == 255).all() and (margin == 100).all() and (second == (1 if ref.known_winner(case) == 0 else 0)).all()
    else:                               # a two-way tie at the top: the runner-up is the later index
        a, b = ref.known_tie(case)
        level = int(np.floor(256.0 / (2.0 + (case.ncls - 2) * np.exp(-3.0))))
        assert (conf == level).all() and (margin == 0).all() and (second == b).all()
    want = np.zeros((case.n, 256), np.uint64)
    want[:, level] = pixels
    assert np.array_equal(hist, want)
    _check((conf, margin, second, hist), case)


# ---- 6. more than one block per frame ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.multiblock_cases(), ids=lambda c: "%dx%d" % (c.h, c.w))
def test_histogram_over_many_blocks(ctx, case):
    got = _run(ctx, case)
    _check(got, case)
    conf, hist = got[0], got[3]
    for f in range(case.n):
        assert np.array_equal(hist[f].astype(np.int64), np.bincount(conf[f].reshape(-1), minlength=256))
        assert int(hist[f].sum()) == case.h * case.w


# ---- 7. probabilities ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.prob_cases(), ids=lambda c: "ncls%d-%dx%d-s%g" % (c.ncls, c.h, c.w, c.scale))
def test_probabilities_are_scaled_not_exponentiated(ctx, case):
    assert ref.is_prob(case)
    _check(_run(ctx, case), case)
    # and read as logits the same tensor gives something else: the flag is honoured
    other = ctx.scores_confidence(ref.scores(case), case.out_h, case.out_w, case.h, case.w, is_prob=False, margin=False, second=False, hist=False)[0]
    assert not np.array_equal(other, ref.reference(case)[0])


# ---- 8. model level -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(90, 180), (128, 256), (120, 250)])
def test_confidence_on_accel18(demo_cfg, rows, cols):
    """Accel-18 at 128 x 256 on the synthetic clip, raw frames: the logits of a key and a non-key frame are finished on the GPU; the call changes
    nothing -- not the generation, not the buffers, not what the captured graphs compute next"""
    import torch
    from accel_amd import demo, runtime
    from accel_amd.core import results, tester
    H, W = 128, 256
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = ref.STRIDE
    out_h, out_w = ref.geo(rows, cols, H, W)[:2]
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    frames = synth.make_clip(rows, cols, 3)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        raw = demo.build_batches(frames, demo_cfg, raw=True)
        base = _steps(r, raw, 3, 3)                      # frames 0 (key), 1, 2 (non-key) without any finishing call
        kept = None
        for i in (0, 1):
            lg, lab = r.step(i, raw[i], 3)
            m = lg.device_ref[0]
            assert lg.device_ref[1] == "logits" and lg.probabilities is False
            gen = m.generation("labels"), m.generation("logits")
            logits0, labels0 = m.read("logits", (1, 19, H, W)), m.read("labels", (1, H, W), np.uint8)
            assert np.array_equal(logits0, base[i][0])
            want = image.confidence_host(lg.asnumpy(), out_h, out_w, rows, cols)
            got = results.confidence(lg, raw[i][0], margin=True, second=True, hist=True)
            assert isinstance(got, tuple) and len(got) == 4
            assert np.array_equal(got[0], want[0]), int(np.count_nonzero(got[0] != want[0]))
            assert np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
            # conf alone is an array; a dict names the same geometry
            alone = results.confidence(lg, dict(raw[i][0].geometry, h=rows, w=cols))
            assert isinstance(alone, np.ndarray) and np.array_equal(alone, want[0])
            pair = results.confidence(lg, raw[i][0], hist=True)
            assert len(pair) == 2 and np.array_equal(pair[1], want[3])
            # pixel for pixel with the labels: the argmax of the same scores
            src_scores = image.labels_to_source_host(logits0, out_h, out_w, rows, cols)
            assert np.array_equal(np.argmax(src_scores, axis=1).astype(np.uint8), results.labels_at_source(lab, raw[i][0]))
            # the device-destination form, into pitched rows
            cp, mp = cols + 7, 4 * cols + 12
            dev = {k: torch.full((1, rows, p), 7, dtype=torch.uint8, device="cuda") for k, p in (("conf", cp), ("margin", mp), ("second", cp))}
            dh = torch.full((1, 256), 7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            m.confidence_device(1, out_h, out_w, rows, cols, conf_ptr=dev["conf"].data_ptr(), conf_pitch=cp, margin_ptr=dev["margin"].data_ptr(),
                                margin_pitch=mp, second_ptr=dev["second"].data_ptr(), second_pitch=cp, hist_ptr=dh.data_ptr())
            m.ctx.sync()
            host = {k: v.cpu().numpy() for k, v in dev.items()}
            assert np.array_equal(host["conf"][:, :, :cols], want[0]) and (host["conf"][:, :, cols:] == 7).all()
            assert np.array_equal(host["second"][:, :, :cols], want[2]) and (host["second"][:, :, cols:] == 7).all()
            assert np.array_equal(np.ascontiguousarray(host["margin"][:, :, :4 * cols]).view(np.uint32), _bits(want[1]))
            assert (host["margin"][:, :, 4 * cols:] == 7).all()
            assert np.array_equal(dh.cpu().numpy().astype(np.uint64), want[3])      # overwritten, not added to
            # nothing was written: generations, labels and logits are what they were
            assert (m.generation("labels"), m.generation("logits")) == gen
            assert np.array_equal(m.read("logits", (1, 19, H, W)), logits0) and np.array_equal(m.read("labels", (1, H, W), np.uint8), labels0)
            # a label handle is not a logits handle
            with pytest.raises(runtime.AccelError, match="logits"):
                results.confidence(lab, raw[i][0])
            kept = lg
        # the captured graphs are undisturbed: the next step gives what the run without finishing calls gave
        lg, lab = r.step(2, raw[2], 3)
        assert np.array_equal(lg.asnumpy(), base[2][0]) and np.array_equal(lab.asnumpy(), base[2][1])
        with pytest.raises(runtime.AccelError, match="stale"):
            results.confidence(kept, raw[1][0])
    finally:
        tester.release_models()


# ---- 9. argument errors ----------------------------------------------------------------------------------------------------------------------------
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
    conf, second = np.zeros((n, rows, cols), np.uint8), np.zeros((n, rows, cols), np.uint8)
    margin, hist = np.zeros((n, rows, cols), np.float32), np.zeros((n, 256), np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(scores=vp(scores), n=n, ncls=ncls, H=H, W=W, out_h=out_h, out_w=out_w, h=rows, w=cols, conf=vp(conf), conf_pitch=cols, margin=vp(margin),
                margin_pitch=4 * cols, second=vp(second), second_pitch=cols, hist=vp(hist))
    m = _logits_model(ctx, n, ncls, H, W)
    odd = _logits_model(ctx, 1, 7, 16, 16)                     # a class count the kernel is not built for
    try:
        m.write("logits", scores)
        state = m.generation("logits")
        calls = {
            "op": lambda a: lib.accel_scores_confidence(ctx.handle, a["scores"], a["n"], a["ncls"], a["H"], a["W"], a["out_h"], a["out_w"], a["h"], a["w"], 0,
                                                        a["conf"], a["conf_pitch"], a["margin"], a["margin_pitch"], a["second"], a["second_pitch"], a["hist"]),
            "model": lambda a: lib.accel_model_confidence(m.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], 0, a["conf"], a["conf_pitch"],
                                                          a["margin"], a["margin_pitch"], a["second"], a["second_pitch"], a["hist"], 0),
        }
        both, op, model = ("op", "model"), ("op",), ("model",)
        cases = [(dict(scores=None), "scores", op), (dict(conf=None, margin=None, second=None, hist=None), "all NULL", both),
                 (dict(n=0), "n =", both), (dict(n=-1), "n =", both), (dict(h=0), "h =", both), (dict(w=0), "w =", both), (dict(h=32769), "h =", both),
                 (dict(w=32769), "w =", both), (dict(H=0), "H x W", op), (dict(W=32769), "H x W", op),
                 (dict(out_h=0), "out_h", both), (dict(out_w=0), "out_w", both), (dict(out_h=H + 1), "out_h", both), (dict(out_w=W + 1), "out_w", both),
                 (dict(conf_pitch=cols - 1), "conf_pitch", both), (dict(second_pitch=cols - 1), "second_pitch", both),
                 (dict(margin_pitch=4 * cols - 4), "margin_pitch", both), (dict(margin_pitch=4 * cols + 2), "margin_pitch", both),
                 (dict(ncls=0), "ncls", op), (dict(ncls=3), "ncls", op), (dict(ncls=20), "ncls", op), (dict(ncls=32), "ncls", op),
                 (dict(n=n + 1), "n =", model)]                                      # larger than the bound batch
        for change, word, names in cases:
            for name in names:
                rc = calls[name](dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (name, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg, (name, change, msg)
        assert lib.accel_scores_confidence(None, vp(scores), n, ncls, H, W, out_h, out_w, rows, cols, 0, vp(conf), cols, None, 0, None, 0, None) == -1
        assert lib.accel_model_confidence(None, n, out_h, out_w, rows, cols, 0, vp(conf), cols, None, 0, None, 0, None, 0) == -1
        assert lib.accel_model_confidence(odd.handle, 1, 16, 16, 16, 16, 0, vp(conf), 16, None, 0, None, 0, None, 0) == -1
        assert "ncls" in lib.accel_last_error().decode()
        bare = runtime.Model(ctx)                               # a model without logits
        assert lib.accel_model_confidence(bare.handle, 1, 8, 8, 8, 8, 0, vp(conf), 8, None, 0, None, 0, None, 0) == -1
        assert "logits" in lib.accel_last_error().decode()
        bare.close()
        # a pitch of an output that is left out is not looked at
        assert calls["op"](dict(good, margin=None, margin_pitch=1, second=None, second_pitch=0)) == 0, lib.accel_last_error().decode()
        conf[...] = 0
        hist[...] = 0
        # none of the refused calls reached the model or the destinations
        assert m.generation("logits") == state and np.array_equal(m.read("logits", (n, ncls, H, W)), scores)
        assert not conf.any() and not second.any() and not margin.any() and not hist.any()
        want = ref.reference(case)
        for name in both:                                       # and every call is accepted as it stands
            for a in (conf, second, margin, hist):
                a[...] = 0
            assert calls[name](good) == 0, (name, lib.accel_last_error().decode())
            assert np.array_equal(conf, want[0]) and np.array_equal(_bits(margin), _bits(want[1])) and np.array_equal(second, want[2])
            assert np.array_equal(hist, want[3])
        assert m.generation("logits") == state
    finally:
        ctx.sync()
        m.close()
        odd.close()


def test_demo_reports_the_confidence_of_every_frame(demo_cfg, capsys, tmp_path):
    """90 x 180 frames bound at 128 x 256: one line per frame from the histogram, and the greyscale map at the source size"""
    from PIL import Image
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "3", "--num_ex", "1", "--synthetic", "90x180", "--scales", "128x256", "--raw-frames",
                   "--finish-on-gpu", "--confidence", "--out", str(tmp_path)])
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("confidence mean ")]
    assert out.rstrip().endswith("done") and len(lines) == 3, out[-1500:]
    for ln in lines:
        mean, low = float(ln.split()[2]), float(ln.split()[4])
        assert 1.0 / 19 <= mean <= 1.0 and 0.0 <= low <= 1.0
    pngs = sorted(tmp_path.glob("conf_*.png"))
    assert len(pngs) == 3
    im = Image.open(str(pngs[0]))
    assert im.size == (180, 90) and im.mode == "L"
