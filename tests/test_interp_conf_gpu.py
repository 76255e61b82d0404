"""Confidence of interpolated scores on the GPU (csrc/scores_confidence.hip behind accel_scores_confidence_interp / accel_model_confidence_interp):
labels, conf, second and hist are what utils.image.confidence_interpolated_host gives -- EXACTLY -- and margin is bit for bit.  The blend is
float64 on both sides with every operation rounded on its own, so of the whole computation only the exp can differ; the inputs come from
interp_conf_ref.py, whose guard conditions (test_interp_conf_cpu.py::test_guard_conditions_of_the_gpu_inputs) say that no byte of them can depend
on the last bits of an exp, and the dyadic cases and known answers are exact, ties included.  So every comparison is np.array_equal: no tolerance.
(Host side, and the mutants these cases tell apart: test_interp_conf_cpu.py.)"""
import ctypes

import numpy as np
import pytest

from accel_amd.utils import image, synth

import interp_conf_ref as ref
from test_frames_u8_gpu import SMALL
from test_results_gpu import STRIDE, _geo, _pitches, _steps

pytestmark = pytest.mark.gpu

NAMES = ("labels", "conf", "margin", "second", "hist")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(name, a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a) if name == "margin" else a, _bits(b) if name == "margin" else b)


def _run(ctx, case, **kw):
    return ctx.scores_confidence_interp(ref.scores(case), case.out_h, case.out_w, case.h, case.w, is_prob=ref.is_prob(case), **kw)


def _check(got, case, want=None, what=""):
    want = ref.reference(case) if want is None else want
    assert len(got) == 5
    assert got[0].shape == (case.n, case.h, case.w) and got[4].shape == (case.n, 256)
    for name, g, w in zip(NAMES, got, want):
        assert _same(name, g, w), (what, ref.ident(case), name, g.dtype, g.shape,
                                   int(np.count_nonzero((_bits(g) if name == "margin" else g) != (_bits(w) if name == "margin" else w))))


# ---- 1. operator level: every case of the table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ncls", ref.NCLS)
@pytest.mark.parametrize("rows,cols,target,max_size", SMALL)
def test_all_five_outputs_equal_the_host_restatement(ctx, rows, cols, target, max_size, ncls, n):
    for case in ref.operator_cases(rows, cols, target, max_size, ncls, n):
        _check(_run(ctx, case), case)


@pytest.mark.parametrize("case", ref.near_tie_cases(), ids=ref.ident)
def test_near_ties_are_decided_in_float64(ctx, case):
    got = _run(ctx, case)
    labels, second = got[0], got[3]
    assert (labels[0] == 11).all() and (second[0] == 5).all(), (int(np.count_nonzero(labels[0] != 11)), int(np.count_nonzero(second[0] != 5)))
    assert (labels[1] == 5).all() and (second[1] == 11).all(), (int(np.count_nonzero(labels[1] != 5)), int(np.count_nonzero(second[1] != 11)))
    _check(got, case)


@pytest.mark.parametrize("case", ref.dyadic_cases(), ids=ref.ident)
def test_dyadic_known_answers(ctx, case):
    import interp_ref
    got = _run(ctx, case)
    labels, conf, margin, second, _ = got
    assert np.array_equal(labels, interp_ref.integer_labels(case)), ref.ident(case)
    if case.kind == "step" and case.h == 16:
        assert conf[0, 3, 6:14].tolist() == [243, 243, 243, 225, 128, 187, 187, 187]
        assert margin[0, 3, 10] == 0 and second[0, 3, 10] == 1 and labels[0, 3, 10] == 0          # the tie takes the first class
    _check(got, case)


@pytest.mark.parametrize("case", ref.known_cases(), ids=ref.ident)
def test_known_answers_on_resampled_geometries(ctx, case):
    got = _run(ctx, case)
    labels, conf, margin, second, hist = got
    if case.kind == "equal":            # identical planes: p = 1 / ncls; two equal classes of two: exactly 128
        level = {2: 128, 19: 13, 21: 12}[case.ncls]
        assert (conf == level).all() and (margin == 0).all() and (labels == 0).all() and (second == 1).all()
    elif case.kind == "one100":         # p = 1 -> 256, clamped
        level, w = 255, ref.known_winner(case)
        assert (conf == 255).all() and (margin == 100).all() and (labels == w).all() and (second == (1 if w == 0 else 0)).all()
    else:                               # a two-way tie at the top: the runner-up is the later index
        a, b = ref.known_tie(case)
        level = int(np.floor(256.0 / (2.0 + (case.ncls - 2) * np.exp(-3.0))))
        assert (conf == level).all() and (margin == 0).all() and (labels == a).all() and (second == b).all()
    want = np.zeros((case.n, 256), np.uint64)
    want[:, level] = case.h * case.w
    assert np.array_equal(hist, want)
    _check(got, case)


@pytest.mark.parametrize("case", ref.prob_cases(), ids=ref.ident)
def test_probabilities_are_scaled_not_exponentiated(ctx, case):
    assert ref.is_prob(case)
    _check(_run(ctx, case), case)
    # and read as logits the same tensor gives something else: the flag is honoured
    other = ctx.scores_confidence_interp(ref.scores(case), case.out_h, case.out_w, case.h, case.w, is_prob=False, labels=False, margin=False,
                                         second=False, hist=False)[1]
    assert not np.array_equal(other, ref.reference(case)[1])


@pytest.mark.parametrize("case", ref.crop_cases(), ids=ref.ident)
def test_crops_of_widths_not_divisible_by_four(ctx, case):
    _check(_run(ctx, case), case)


@pytest.mark.parametrize("case", ref.multiblock_cases(), ids=ref.ident)
def test_histogram_over_many_blocks(ctx, case):
    got = _run(ctx, case)
    _check(got, case)
    conf, hist = got[1], got[4]
    for f in range(case.n):
        assert np.array_equal(hist[f].astype(np.int64), np.bincount(conf[f].reshape(-1), minlength=256))
        assert int(hist[f].sum()) == case.h * case.w


def test_full_size_720p_from_its_bound_size(ctx):
    case = ref.full_case()
    assert (case.n, case.H, case.W, case.out_h, case.out_w) == (1, 1024, 1824, 1024, 1820)
    _check(_run(ctx, case), case)


# ---- 2. the identity geometry is the nearest rule's ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ref.small_case(*SMALL[0], ncls=k, n=3, scale=1.0) for k in ref.NCLS] + ref.crop_cases()[:2] + [ref.multiblock_cases()[1]],
                         ids=ref.ident)
def test_identity_equals_the_nearest_confidence_and_the_interpolated_labels(ctx, case):
    assert (case.h, case.w) == (case.out_h, case.out_w)
    s = ref.scores(case)
    got = _run(ctx, case)
    nearest = ctx.scores_confidence(s, case.out_h, case.out_w, case.h, case.w)
    assert np.array_equal(got[0], ctx.scores_labels(s, case.out_h, case.out_w, case.h, case.w))
    for name, g, w in zip(NAMES[1:], got[1:], nearest):
        assert _same(name, g, w), (ref.ident(case), name)


# ---- 3. each output alone, pitched destinations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.pitched_cases(), ids=ref.ident)
def test_each_output_alone_equals_the_all_together_call(ctx, case):
    together = _run(ctx, case)
    _check(together, case)
    for i, name in enumerate(NAMES):
        only = dict.fromkeys(NAMES, False)
        only[name] = True
        got = _run(ctx, case, **only)
        assert [g is not None for g in got] == [j == i for j in range(5)], name
        assert _same(name, got[i], together[i]), name


@pytest.mark.parametrize("case", ref.pitched_cases(), ids=ref.ident)
def test_pitched_destinations_keep_the_bytes_between_rows(ctx, case):
    wl, wc, wm, ws, wh = ref.reference(case)
    n, h, w = case.n, case.h, case.w
    margin_pitches = [(p + 3) // 4 * 4 for p in _pitches(4 * w)]           # bytes, multiples of 4
    for pitch, mpitch in zip(_pitches(w), margin_pitches):
        rng = np.random.default_rng(pitch)
        labels, conf, second = (rng.integers(1, 256, (n, h, pitch), dtype=np.uint8) for _ in range(3))
        margin = rng.integers(1, 1 << 30, (n, h, mpitch // 4), dtype=np.uint32).view(np.float32)
        before = labels.copy(), conf.copy(), margin.copy(), second.copy()
        got = ctx.scores_confidence_interp(ref.scores(case), case.out_h, case.out_w, h, w, labels=labels, conf=conf, margin=margin, second=second)
        assert got[0] is labels and got[1] is conf and got[2] is margin and got[3] is second
        for a, b, want in ((labels, before[0], wl), (conf, before[1], wc), (second, before[3], ws)):
            assert np.array_equal(a[:, :, :w], want) and np.array_equal(a[:, :, w:], b[:, :, w:]), pitch
        assert np.array_equal(_bits(margin[:, :, :w]), _bits(wm)) and np.array_equal(_bits(margin[:, :, w:]), _bits(before[2][:, :, w:])), mpitch
        assert np.array_equal(got[4], wh)


# ---- 4. model level -------------------------------------------------------------------------------------------------------------------------------------
def _logits_model(ctx, n, ncls, H, W):
    """a model that owns a `logits` buffer of n x ncls x H x W and says so (no op: nothing is ever run)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=logits bytes=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d\n"
                     % (n * ncls * H * W * 4, n, ncls, H, W))
    return m


def _device_call(m, case, pitch, mpitch):
    """confidence_interp_device into rows of `pitch` (margin: `mpitch`) bytes filled with 7s: ({name: host copy}, hist)"""
    import torch
    n, h = case.n, case.h
    dev = {k: torch.full((n, h, p), 7, dtype=torch.uint8, device="cuda") for k, p in (("labels", pitch), ("conf", pitch), ("margin", mpitch), ("second", pitch))}
    dh = torch.full((n, 256), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m.confidence_interp_device(n, case.out_h, case.out_w, h, case.w, is_prob=ref.is_prob(case), labels_ptr=dev["labels"].data_ptr(), labels_pitch=pitch,
                               conf_ptr=dev["conf"].data_ptr(), conf_pitch=pitch, margin_ptr=dev["margin"].data_ptr(), margin_pitch=mpitch,
                               second_ptr=dev["second"].data_ptr(), second_pitch=pitch, hist_ptr=dh.data_ptr())
    m.ctx.sync()
    return {k: v.cpu().numpy() for k, v in dev.items()}, dh.cpu().numpy().astype(np.uint64)


def _check_device(host, hist, case, want):
    w = case.w
    for name, at in (("labels", 0), ("conf", 1), ("second", 3)):
        assert np.array_equal(host[name][:, :, :w], want[at]) and (host[name][:, :, w:] == 7).all(), (ref.ident(case), name)
    assert np.array_equal(np.ascontiguousarray(host["margin"][:, :, :4 * w]).view(np.uint32), _bits(want[2])), ref.ident(case)
    assert (host["margin"][:, :, 4 * w:] == 7).all()
    assert np.array_equal(hist, want[4])                        # overwritten, not added to


@pytest.mark.parametrize("case", [ref.pitched_cases()[0], ref.pitched_cases()[2], ref.prob_cases()[4]], ids=ref.ident)
def test_device_destinations_at_pitches_of_both_paths(ctx, case):
    """rows in HBM whose pitches allow 16-byte stores (the identity case takes the vector path) and whose pitches do not"""
    m = _logits_model(ctx, case.n, case.ncls, case.H, case.W)
    try:
        m.write("logits", ref.scores(case))
        gen = m.generation("logits")
        for pitch, mpitch in (((case.w + 15) // 16 * 16 + 16, (4 * case.w + 15) // 16 * 16 + 16), (case.w + 7, 4 * case.w + 12)):
            host, hist = _device_call(m, case, pitch, mpitch)
            _check_device(host, hist, case, ref.reference(case))
        _check(m.confidence_interp(case.n, case.out_h, case.out_w, case.h, case.w, is_prob=ref.is_prob(case)), case)
        assert m.generation("logits") == gen and np.array_equal(m.read("logits", (case.n, case.ncls, case.H, case.W)), ref.scores(case))
    finally:
        ctx.sync()
        m.close()


def test_confidence_of_interpolated_scores_on_accel18(demo_cfg):
    """Accel-18 at 128 x 256 on the synthetic clip, raw frames of 90 x 180 (the map is resampled): the logits of a key and a non-key frame are
    finished on the GPU with interpolate=True; the calls change nothing -- not the generations, not the buffers, not what the captured graphs
    compute next"""
    from accel_amd import demo, runtime
    from accel_amd.core import results, tester
    H, W, rows, cols = 128, 256, 90, 180
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = STRIDE
    out_h, out_w = _geo(rows, cols, H, W)[:2]
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
            gen = m.generation("labels"), m.generation("logits")
            logits0, labels0 = m.read("logits", (1, 19, H, W)), m.read("labels", (1, H, W), np.uint8)
            assert np.array_equal(logits0, base[i][0]) and np.array_equal(labels0, base[i][1])
            case = ref.Case("model", 1, 19, H, W, out_h, out_w, rows, cols, 1.0, i)
            want = image.confidence_interpolated_host(lg.asnumpy(), out_h, out_w, rows, cols)
            # everything through the handle: the model-level call equals the specification on the fetched logits
            got = results.confidence(lg, raw[i][0], margin=True, second=True, hist=True, interpolate=True, labels=True)
            assert isinstance(got, tuple)
            _check(got, case, want=want, what="frame %d" % i)
            # its labels are those of labels_at_source, its other outputs do not depend on asking for them
            assert np.array_equal(got[0], results.labels_at_source(lg, raw[i][0], interpolate=True))
            four = results.confidence(lg, raw[i][0], margin=True, second=True, hist=True, interpolate=True)
            assert len(four) == 4 and all(_same(name, g, w) for name, g, w in zip(NAMES[1:], four, want[1:]))
            alone = results.confidence(lg, dict(raw[i][0].geometry, h=rows, w=cols), interpolate=True)           # a dict names the same geometry
            assert isinstance(alone, np.ndarray) and np.array_equal(alone, want[1])
            trio = results.confidence(lg, raw[i][0], hist=True, interpolate=True, labels=True)
            assert len(trio) == 3 and np.array_equal(trio[0], want[0]) and np.array_equal(trio[1], want[1]) and np.array_equal(trio[2], want[4])
            # it is not the nearest rule's answer: this frame was resampled on the way in
            assert not np.array_equal(results.confidence(lg, raw[i][0]), want[1])
            with pytest.raises(ValueError, match="interpolate=True"):
                results.confidence(lg, raw[i][0], labels=True)
            # the device-destination form, into pitched rows
            host, hist = _device_call(m, case, cols + 7, 4 * cols + 12)
            _check_device(host, hist, case, want)
            # a label handle is not a logits handle
            with pytest.raises(runtime.AccelError, match="logits"):
                results.confidence(lab, raw[i][0], interpolate=True)
            # nothing was written: generations, labels and logits are what they were
            assert (m.generation("labels"), m.generation("logits")) == gen
            assert np.array_equal(m.read("logits", (1, 19, H, W)), logits0) and np.array_equal(m.read("labels", (1, H, W), np.uint8), labels0)
            kept = lg
        # the captured graphs are undisturbed: the next step gives what the run without finishing calls gave
        lg, lab = r.step(2, raw[2], 3)
        assert np.array_equal(lg.asnumpy(), base[2][0]) and np.array_equal(lab.asnumpy(), base[2][1])
        # a logits handle kept across that step names a buffer that has been rewritten: never read
        with pytest.raises(runtime.AccelError, match="stale"):
            results.confidence(kept, raw[1][0], interpolate=True, labels=True)
    finally:
        tester.release_models()


# ---- 5. scratch reuse ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_staging_is_reused_across_repeated_and_growing_calls(ctx, n):
    """one model, its staged output shared with the nearest confidence and the interpolated labels, while the source size goes up and down and
    the set of outputs changes: every call gives what its own specification demands; the operator-level call (fresh device temporaries every
    time) between them"""
    H, W, ncls = 48, 96, 19
    m = _logits_model(ctx, n, ncls, H, W)
    try:
        for rows, cols in ((44, 82), (60, 120), (36, 72), (60, 120)):
            case = ref.small_case(rows, cols, H, W, ncls=ncls, n=n, scale=1.0)
            assert (case.H, case.W) == (H, W)
            v, exact = ref.scaled_float64(case)                  # the conditions of test_interp_conf_cpu.py, for the cases this walk adds
            assert not ((np.abs(v - np.rint(v)) < ref.CONF_GUARD) & ~exact).any(), ref.ident(case)
            first, third, top = ref.smallest_gaps(case)
            assert first >= ref.GUARD * top and third >= ref.GUARD * top, ref.ident(case)
            s, want = ref.scores(case), ref.reference(case)
            m.write("logits", s)
            args = (n, case.out_h, case.out_w, rows, cols)
            for _ in range(2):
                _check(m.confidence_interp(*args), case, what="all five")
            got = m.confidence_interp(*args, conf=False, margin=False, second=False)            # a smaller stage between two full ones
            assert got[1] is None and got[2] is None and got[3] is None and np.array_equal(got[0], want[0]) and np.array_equal(got[4], want[4])
            nearest = m.confidence(*args)
            for name, g, w in zip(NAMES[1:], nearest, image.confidence_host(s, case.out_h, case.out_w, rows, cols)):
                assert _same(name, g, w), (ref.ident(case), name)
            assert np.array_equal(m.scores_labels(*args), want[0])
            _check(m.confidence_interp(*args), case, what="after the others")
            _check(_run(ctx, case), case, what="operator level")
    finally:
        ctx.sync()
        m.close()


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_err_arg(ctx):
    """every call the kernel could not honour is refused on the host, with a message that names the argument; nothing is launched and the model is
    what it was"""
    from accel_amd import runtime
    lib = runtime.lib()
    n, ncls, H, W, rows, cols = 2, 19, 32, 64, 29, 50
    out_h, out_w = 31, 54
    case = ref.Case("normal", n, ncls, H, W, out_h, out_w, rows, cols, 1.0, 9)
    scores = ref.scores(case)
    labels, conf, second = (np.zeros((n, rows, cols), np.uint8) for _ in range(3))
    margin, hist = np.zeros((n, rows, cols), np.float32), np.zeros((n, 256), np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(scores=vp(scores), n=n, ncls=ncls, H=H, W=W, out_h=out_h, out_w=out_w, h=rows, w=cols, labels=vp(labels), labels_pitch=cols, conf=vp(conf),
                conf_pitch=cols, margin=vp(margin), margin_pitch=4 * cols, second=vp(second), second_pitch=cols, hist=vp(hist))
    m = _logits_model(ctx, n, ncls, H, W)
    odd = _logits_model(ctx, 1, 7, 16, 16)                     # a class count the kernel is not built for
    try:
        m.write("logits", scores)
        state = m.generation("logits")
        outs = lambda a: (a["labels"], a["labels_pitch"], a["conf"], a["conf_pitch"], a["margin"], a["margin_pitch"], a["second"], a["second_pitch"], a["hist"])
        calls = {
            "op": lambda a: lib.accel_scores_confidence_interp(ctx.handle, a["scores"], a["n"], a["ncls"], a["H"], a["W"], a["out_h"], a["out_w"], a["h"],
                                                               a["w"], 0, *outs(a)),
            "model": lambda a: lib.accel_model_confidence_interp(m.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], 0, *(outs(a) + (0,))),
        }
        both, op, model = ("op", "model"), ("op",), ("model",)
        cases = [(dict(scores=None), "scores", op), (dict(labels=None, conf=None, margin=None, second=None, hist=None), "labels, conf", both),
                 (dict(n=0), "n =", both), (dict(n=-1), "n =", both), (dict(h=0), "h =", both), (dict(w=0), "w =", both), (dict(h=32769), "h =", both),
                 (dict(w=32769), "w =", both), (dict(H=0), "H x W", op), (dict(W=32769), "H x W", op),
                 (dict(out_h=0), "out_h", both), (dict(out_w=0), "out_w", both), (dict(out_h=H + 1), "out_h", both), (dict(out_w=W + 1), "out_w", both),
                 (dict(labels_pitch=cols - 1), "labels_pitch", both), (dict(conf_pitch=cols - 1), "conf_pitch", both),
                 (dict(second_pitch=cols - 1), "second_pitch", both),
                 (dict(margin_pitch=4 * cols - 4), "margin_pitch", both), (dict(margin_pitch=4 * cols + 2), "margin_pitch", both),
                 (dict(ncls=0), "ncls", op), (dict(ncls=3), "ncls", op), (dict(ncls=20), "ncls", op), (dict(ncls=32), "ncls", op),
                 (dict(n=n + 1), "n =", model)]                                      # larger than the bound batch
        for change, word, names in cases:
            for name in names:
                rc = calls[name](dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (name, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg and "_confidence_interp" in msg, (name, change, msg)
        nothing = (None, 0, vp(conf), cols, None, 0, None, 0, None)
        assert lib.accel_scores_confidence_interp(None, vp(scores), n, ncls, H, W, out_h, out_w, rows, cols, 0, *nothing) == -1
        assert lib.accel_model_confidence_interp(None, n, out_h, out_w, rows, cols, 0, *(nothing + (0,))) == -1
        assert lib.accel_model_confidence_interp(odd.handle, 1, 16, 16, 16, 16, 0, None, 0, vp(conf), 16, None, 0, None, 0, None, 0) == -1
        assert "ncls" in lib.accel_last_error().decode()
        bare = runtime.Model(ctx)                               # a model without logits
        assert lib.accel_model_confidence_interp(bare.handle, 1, 8, 8, 8, 8, 0, None, 0, vp(conf), 8, None, 0, None, 0, None, 0) == -1
        assert "logits" in lib.accel_last_error().decode()
        bare.close()
        # misaligned device destinations of the model-level call
        for change, word in ((dict(margin=ctypes.c_void_p(margin.ctypes.data + 2)), "margin"), (dict(hist=ctypes.c_void_p(hist.ctypes.data + 4)), "hist")):
            assert lib.accel_model_confidence_interp(m.handle, n, out_h, out_w, rows, cols, 0, *(outs(dict(good, **change)) + (1,))) == -1
            assert word in lib.accel_last_error().decode() and "aligned" in lib.accel_last_error().decode()
        # a pitch of an output that is left out is not looked at; labels alone is a call
        assert calls["op"](dict(good, labels=None, labels_pitch=0, margin=None, margin_pitch=1, second=None, second_pitch=0)) == 0, lib.accel_last_error().decode()
        assert calls["model"](dict(good, conf=None, margin=None, second=None, hist=None)) == 0, lib.accel_last_error().decode()
        want = ref.reference(case)
        assert np.array_equal(labels, want[0])
        for a in (labels, conf, hist):
            a[...] = 0
        # none of the refused calls reached the model or the destinations
        assert m.generation("logits") == state and np.array_equal(m.read("logits", (n, ncls, H, W)), scores)
        assert not second.any() and not margin.any()
        for name in both:                                       # and every call is accepted as it stands
            for a in (labels, conf, second, margin, hist):
                a[...] = 0
            assert calls[name](good) == 0, (name, lib.accel_last_error().decode())
            _check((labels, conf, margin, second, hist), case, what=name)
        assert m.generation("logits") == state
    finally:
        ctx.sync()
        m.close()
        odd.close()


# ---- 7. the demo ---------------------------------------------------------------------------------------------------------------------------------------------
def test_demo_reports_the_confidence_of_the_interpolated_labels(demo_cfg, capsys, tmp_path):
    """90 x 180 frames bound at 128 x 256 with --interpolate --confidence: one confidence line per frame, the greyscale map and the labels at
    the source size, all from one call per frame"""
    from PIL import Image
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "3", "--num_ex", "1", "--synthetic", "90x180", "--scales", "128x256", "--raw-frames",
                   "--finish-on-gpu", "--interpolate", "--confidence", "--out", str(tmp_path)])
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("confidence mean ")]
    assert out.rstrip().endswith("done") and out.count("testing synthetic_") == 3 and len(lines) == 3, out[-1500:]
    for ln in lines:
        mean, low = float(ln.split()[2]), float(ln.split()[4])
        assert 1.0 / 19 <= mean <= 1.0 and 0.0 <= low <= 1.0
    confs, segs = sorted(tmp_path.glob("conf_*.png")), sorted(tmp_path.glob("seg_*.png"))
    assert len(confs) == 3 and len(segs) == 3
    im = Image.open(str(confs[0]))
    assert im.size == (180, 90) and im.mode == "L" and Image.open(str(segs[0])).size == (180, 90)
