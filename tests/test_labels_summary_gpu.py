"""Summary of finished frames on the GPU (csrc/labels_summary.hip behind accel_labels_summary and the accel_model_* forms): per-class areas, coordinate
sums, boxes, class transitions and the kept map are what utils.image.labels_summary_host gives -- EXACTLY.  Everything is integer arithmetic, so every
comparison is np.array_equal: no tolerance.  (Host side, and the wrong kernels the cases tell apart: test_labels_summary_cpu.py.)"""
import ctypes
import re

import numpy as np
import pytest

from accel_amd.utils import image, synth

import interp_ref
import summary_ref as ref
from test_interp_labels_gpu import _logits_model
from test_results_gpu import STRIDE, _check_rows, _fast_hist, _geo, _labels_model, _pitched, _pitches, _steps

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    for name, a, b in zip(("stats", "box", "trans", "kept"), got, want):
        if b is None:
            assert a is None, (what, name)
            continue
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape, (what, name, None if a is None else (a.dtype, a.shape))
        assert np.array_equal(a, b), (what, name, int(np.count_nonzero(a != b)))


# ---- operator level ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_the_kernel_equals_the_specification(ctx, case):
    s = case.shape
    labels, prev, want = ref.labels(s, case.values), ref.previous(case), ref.expected(case)
    got = ctx.labels_summary(labels, s.out_h, s.out_w, s.h, s.w, s.ncls, prev=prev, kept=True)
    _same(got, want, "with prev")
    got = ctx.labels_summary(labels, s.out_h, s.out_w, s.h, s.w, s.ncls, kept=True)
    _same(got, (want.stats, want.box, None, want.kept), "without prev")


@pytest.mark.parametrize("case", [c for c in ref.CASES if c.prev == "independent" and c.values in ("uniform", "runs")], ids=ref.case_id)
def test_each_output_alone_equals_the_call_for_all_of_them(ctx, case):
    s = case.shape
    labels, prev, want = ref.labels(s, case.values), ref.previous(case), ref.expected(case)
    run = lambda **kw: ctx.labels_summary(labels, s.out_h, s.out_w, s.h, s.w, s.ncls, **kw)
    _same(run(box=False), (want.stats, None, None, None), "stats alone")
    _same(run(stats=False), (None, want.box, None, None), "box alone")
    _same(run(prev=prev, stats=False, box=False), (None, None, want.trans, None), "trans alone")
    _same(run(stats=False, box=False, kept=True), (None, None, None, want.kept), "kept alone")
    _same(run(prev=prev, trans=False), (want.stats, want.box, None, None), "a previous frame that is not asked about")


@pytest.mark.parametrize("si", [1, 2, 3])
def test_pitched_maps_keep_or_ignore_the_bytes_between_rows(ctx, si):
    case = ref.Case(ref.SHAPES[si], "runs", "ignored")
    s = case.shape
    labels, prev, want = ref.labels(s, case.values), ref.previous(case), ref.expected(case)
    for pitch in _pitches(s.w)[1:]:
        out = _pitched(np.zeros((s.n, s.h, s.w), np.uint8), pitch, pitch)
        before = out.copy()
        p = _pitched(prev, pitch, pitch + 1)
        got = ctx.labels_summary(labels, s.out_h, s.out_w, s.h, s.w, s.ncls, prev=p, prev_width=s.w, kept=out)
        assert got[3] is out
        _check_rows(out, before, want.kept, "kept pitch %d" % pitch)
        _same(got[:3], want[:3], "prev pitch %d" % pitch)


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------------
def _maps(seed, n, H, W, ncls):
    """label maps in runs, a few ignored ids among them"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 200, n * H * W // 16 + 8)
    a = np.repeat(rng.integers(0, ncls + 2, lengths.size, dtype=np.uint8), lengths)[:n * H * W].reshape(n, H, W).copy()
    a[a >= ncls] = 255
    return a


def test_the_model_keeps_the_previous_map(ctx):
    import torch
    n, H, W, out_h, out_w, h, w, ncls = 2, 48, 80, 37, 70, 50, 93, 19
    A, B, C = (_maps(seed, n, H, W, ncls) for seed in (1, 2, 3))
    spec = lambda cur, prev=None, **kw: image.labels_summary_host(cur, kw.get("out_h", out_h), kw.get("out_w", out_w), kw.get("h", h), kw.get("w", w),
                                                                  kw.get("ncls", ncls), prev=prev)
    m, other = _labels_model(ctx, n, H, W), _labels_model(ctx, n, H, W)
    try:
        run = lambda **kw: m.labels_summary(kw.pop("n", n), out_h, out_w, kw.pop("h", h), kw.pop("w", w), kw.pop("ncls", ncls), **kw)
        m.write("labels", A)
        other.write("labels", B)
        a = spec(A)
        _same(run(track=True), (a[0], a[1], None), "the first tracked call compares with nothing")
        _same(other.labels_summary(n, out_h, out_w, h, w, ncls, track=True), spec(B)[:2] + (None,), "the other model's first call")
        m.write("labels", B)
        _same(run(), spec(B)[:2] + (None,), "an untracked call")
        m.write("labels", C)
        gen = m.generation("labels")
        c = spec(C, prev=a[3])
        _same(run(track=True), c[:3], "the second tracked call: against the first map, not the untracked one")
        _same(run(track=True), spec(C, prev=c[3])[:3], "the same map again: the diagonal")
        _same(run(track=True, stats=False, box=False), (None, None, spec(C, prev=c[3])[2]), "transitions alone")
        # the other model kept its own map
        other.write("labels", A)
        _same(other.labels_summary(n, out_h, out_w, h, w, ncls, track=True), spec(A, prev=spec(B)[3])[:3], "the other model's second call")
        # forgetting, and every change of what the kept map was made under
        m.labels_forget()
        _same(run(track=True), c[:2] + (None,), "after labels_forget")
        _same(run(track=True), spec(C, prev=c[3])[:3], "and the call after that")
        _same(run(track=True, ncls=21), spec(C, ncls=21)[:2] + (None,), "another ncls")
        _same(run(track=True, n=1), spec(C[:1])[:2] + (None,), "another n")
        _same(run(track=True), c[:2] + (None,), "n again")
        _same(run(track=True, h=h + 1), spec(C, h=h + 1)[:2] + (None,), "another h")
        _same(run(track=True, h=h + 1, w=w - 1), spec(C, h=h + 1, w=w - 1)[:2] + (None,), "another w")
        m.labels_forget()
        m.labels_forget()                                        # not an error when there is none
        # device destinations equal host destinations: the first call compares with nothing and leaves trans alone
        dev = [torch.full((size,), 7, dtype=dtype, device="cuda") for size, dtype in ((n * ncls * 3, torch.int64), (n * ncls * 4, torch.int32),
                                                                                     (n * ncls * ncls, torch.int64))]
        torch.cuda.synchronize()                                 # torch's stream and the library's compute stream are not ordered by themselves
        ptrs = dict(stats_ptr=dev[0].data_ptr(), box_ptr=dev[1].data_ptr(), trans_ptr=dev[2].data_ptr())
        assert m.labels_summary_device(n, out_h, out_w, h, w, ncls, track=True, **ptrs) is False
        ctx.sync()
        assert np.array_equal(dev[0].cpu().numpy().view(np.uint64).reshape(n, ncls, 3), c[0])
        assert np.array_equal(dev[1].cpu().numpy().reshape(n, ncls, 4), c[1]) and (dev[2].cpu().numpy() == 7).all()
        m.write("labels", A)
        assert m.labels_summary_device(n, out_h, out_w, h, w, ncls, track=True, **ptrs) is True
        ctx.sync()
        d = spec(A, prev=c[3])
        assert np.array_equal(dev[0].cpu().numpy().view(np.uint64).reshape(n, ncls, 3), d[0])
        assert np.array_equal(dev[1].cpu().numpy().reshape(n, ncls, 4), d[1])
        assert np.array_equal(dev[2].cpu().numpy().view(np.uint64).reshape(n, ncls * ncls), d[2])
        # nothing but `write` moved the generation, and the maps are what was written
        m.write("labels", C)
        gen2 = m.generation("labels")
        run(track=True)
        run()
        assert gen2 == gen + 2 and m.generation("labels") == gen2
        assert np.array_equal(m.read("labels", (n, H, W), np.uint8), C)
        del dev
    finally:
        ctx.sync()
        m.close()
        other.close()


@pytest.mark.parametrize("case", interp_ref.pitched_cases() + [c for c in interp_ref.dyadic_cases() if c.kind == "ints" and c.ncls == 19],
                         ids=interp_ref.ident)
def test_the_scores_form_summarises_the_interpolated_labels(ctx, case):
    """the inputs of the interpolated-label tests, whose guard condition (test_interp_labels_cpu.py) makes equality of every label a fair demand"""
    labels = interp_ref.reference(case)
    spec = lambda prev=None: image.labels_summary_host(labels, case.h, case.w, case.h, case.w, 19, prev=prev)
    m = _logits_model(ctx, case.n, case.ncls, case.H, case.W)
    try:
        m.write("logits", interp_ref.scores(case))
        gen = m.generation("logits")
        run = lambda **kw: m.scores_summary(case.n, case.out_h, case.out_w, case.h, case.w, 19, **kw)
        _same(run(), spec()[:2] + (None,), "untracked")
        _same(run(track=True), spec()[:2] + (None,), "the first tracked call")
        _same(run(track=True), spec(prev=labels)[:3], "the second: the diagonal")
        assert np.array_equal(m.scores_labels(case.n, case.out_h, case.out_w, case.h, case.w), labels)
        assert m.generation("logits") == gen
    finally:
        ctx.sync()
        m.close()


def test_one_kept_map_serves_both_forms(ctx):
    """a model with `labels` and `logits`: the labels form compares with what the scores form kept"""
    from accel_amd import runtime
    case = interp_ref.pitched_cases()[2]
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=logits bytes=%d\npbuf name=labels bytes=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d\n"
                     "meta labels_n=%d labels_h=%d labels_w=%d\n" % (case.n * case.ncls * case.H * case.W * 4, (case.n * case.H * case.W + 255) // 256 * 256,
                                                                      case.n, case.ncls, case.H, case.W, case.n, case.H, case.W))
    try:
        maps = _maps(9, case.n, case.H, case.W, 19)
        m.write("logits", interp_ref.scores(case))
        m.write("labels", maps)
        assert m.scores_summary(case.n, case.out_h, case.out_w, case.h, case.w, 19, track=True)[2] is None
        want = image.labels_summary_host(maps, case.out_h, case.out_w, case.h, case.w, 19, prev=interp_ref.reference(case))
        _same(m.labels_summary(case.n, case.out_h, case.out_w, case.h, case.w, 19, track=True), want[:3], "labels after scores")
    finally:
        ctx.sync()
        m.close()


# ---- argument errors --------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_err_arg(ctx):
    """every call the kernel could not honour is refused on the host, with a message that names the argument; nothing is launched, nothing is written
    and the kept map is what it was"""
    from accel_amd import runtime
    lib = runtime.lib()
    n, H, W, out_h, out_w, h, w, ncls = 2, 32, 64, 31, 54, 29, 50, 19
    labels = _maps(4, n, H, W, ncls)
    prev = _maps(5, n, h, w, ncls)
    stats, box, trans = np.zeros((n, ncls, 3), np.uint64), np.zeros((n, ncls, 4), np.int32), np.zeros((n, ncls * ncls), np.uint64)
    kept = np.zeros((n, h, w), np.uint8)
    compared = ctypes.c_int(5)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    good = dict(labels=labels, n=n, H=H, W=W, out_h=out_h, out_w=out_w, h=h, w=w, ncls=ncls, prev=prev, prev_pitch=w, stats=stats, box=box, trans=trans,
                kept=kept, kept_pitch=w, track=1, compared=ctypes.byref(compared))
    m, lm = _labels_model(ctx, n, H, W), _logits_model(ctx, n, 19, H, W)
    try:
        m.write("labels", labels)
        lm.write("logits", np.random.default_rng(6).standard_normal((n, 19, H, W)).astype(np.float32))
        assert m.labels_summary(n, out_h, out_w, h, w, ncls, track=True)[2] is None
        assert lm.scores_summary(n, out_h, out_w, h, w, ncls, track=True)[2] is None
        gen = m.generation("labels"), lm.generation("logits")
        calls = {
            "op": lambda a: lib.accel_labels_summary(ctx.handle, vp(a["labels"]), a["n"], a["H"], a["W"], a["out_h"], a["out_w"], a["h"], a["w"], a["ncls"],
                                                     vp(a["prev"]), a["prev_pitch"], vp(a["stats"]), vp(a["box"]), vp(a["trans"]), vp(a["kept"]), a["kept_pitch"]),
            "labels": lambda a: lib.accel_model_labels_summary(m.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], a["ncls"], a["track"], vp(a["stats"]),
                                                               vp(a["box"]), vp(a["trans"]), 0, a["compared"]),
            "scores": lambda a: lib.accel_model_scores_summary(lm.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], a["ncls"], a["track"], vp(a["stats"]),
                                                               vp(a["box"]), vp(a["trans"]), 0, a["compared"]),
        }
        every, models = tuple(calls), ("labels", "scores")
        cases = [(dict(n=0), "n =", every), (dict(n=-1), "n =", every), (dict(n=32769), "n =", every), (dict(h=0), "h =", every), (dict(w=0), "w =", every),
                 (dict(h=32769), "h =", every), (dict(w=32769), "w =", every), (dict(out_h=H + 1), "out_h", every), (dict(out_w=W + 1), "out_w", every),
                 (dict(out_h=0), "out_h", every), (dict(out_w=0), "out_w", every), (dict(H=0), "H x W", ("op",)), (dict(W=32769), "H x W", ("op",)),
                 (dict(ncls=0), "ncls", every), (dict(ncls=33), "ncls", every), (dict(labels=None), "labels", ("op",)),
                 (dict(prev_pitch=w - 1), "prev_pitch", ("op",)), (dict(kept_pitch=w - 1), "kept_pitch", ("op",)),
                 (dict(stats=None, box=None, trans=None, kept=None), "all NULL", every), (dict(prev=None), "prev", ("op",)),
                 (dict(track=0), "track", models), (dict(n=n + 1), "n =", models), (dict(compared=None), "compared", models)]
        for change, word, names in cases:
            for name in names:
                rc = calls[name](dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (name, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg, (name, change, msg)
        assert lib.accel_labels_summary(None, vp(labels), n, H, W, out_h, out_w, h, w, ncls, None, 0, vp(stats), None, None, None, 0) == -1
        assert lib.accel_model_labels_summary(None, n, out_h, out_w, h, w, ncls, 0, vp(stats), None, None, 0, ctypes.byref(compared)) == -1
        assert lib.accel_model_labels_forget(None) == -1
        assert lib.accel_model_labels_summary(lm.handle, n, out_h, out_w, h, w, ncls, 0, vp(stats), None, None, 0, ctypes.byref(compared)) == -1
        assert "labels" in lib.accel_last_error().decode()       # a model without label maps
        assert lib.accel_model_scores_summary(m.handle, n, out_h, out_w, h, w, ncls, 0, vp(stats), None, None, 0, ctypes.byref(compared)) == -1
        assert "logits" in lib.accel_last_error().decode()       # and one without scores
        # none of the refused calls wrote anything or reached the models: destinations, generations, kept maps
        assert not stats.any() and not box.any() and not trans.any() and not kept.any() and compared.value == 5
        assert (m.generation("labels"), lm.generation("logits")) == gen
        # and every call is accepted as it stands; the kept maps are still there to compare with
        want = image.labels_summary_host(labels, out_h, out_w, h, w, ncls, prev=prev)
        assert calls["op"](good) == 0, lib.accel_last_error().decode()
        _same((stats, box, trans, kept), want, "the operator call")
        assert calls["labels"](good) == 0, lib.accel_last_error().decode()
        assert compared.value == 1
        _same((stats, box, trans), image.labels_summary_host(labels, out_h, out_w, h, w, ncls, prev=want[3])[:3], "the labels form")
        compared.value = 5
        assert calls["scores"](good) == 0, lib.accel_last_error().decode()
        assert compared.value == 1
        interpolated = lm.scores_labels(n, out_h, out_w, h, w)
        _same((stats, box, trans), image.labels_summary_host(interpolated, h, w, h, w, ncls, prev=interpolated)[:3], "the scores form")
    finally:
        ctx.sync()
        m.close()
        lm.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def test_summary_on_accel18(demo_cfg):
    """Accel-18 at 128 x 256 on the synthetic clip, raw frames of 90 x 180: a key frame and two non-key frames are summarised and tracked on the GPU; the
    calls change nothing -- not the generations, not what the captured graphs compute next"""
    from accel_amd import demo, runtime
    from accel_amd.core import results, tester
    H, W, rows, cols = 128, 256, 90, 180
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = STRIDE
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    frames = synth.make_clip(rows, cols, 4)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        raw = demo.build_batches(frames, demo_cfg, raw=True)
        base = _steps(r, raw, 3, 4)                      # frames 0 (key), 1, 2 (non-key) and 3 (key) without any finishing call
        before, kept = None, None
        for i in (0, 1, 2):
            lg, lab = r.step(i, raw[i], 3)
            assert np.array_equal(lg.asnumpy(), base[i][0]) and np.array_equal(lab.asnumpy(), base[i][1])      # undisturbed by the calls before
            m = lab.device_ref[0]
            gen = m.generation("labels"), m.generation("logits")
            if i == 0:
                results.forget(lab)
            s = results.summary(lab, raw[i][0], track=True)
            assert isinstance(s, results.Summary)
            src = results.labels_at_source(lab, raw[i][0])
            want = image.labels_summary_host(src, rows, cols, rows, cols, 19, prev=before)
            _same(tuple(s), want[:3], "frame %d" % i)
            assert int(s.stats[0, :, 0].sum()) == rows * cols
            if before is not None:
                assert np.array_equal(s.trans.reshape(19, 19).astype(np.int64), _fast_hist(src, before, 19))      # rows the previous frame
                assert 0.0 <= float(results.summary_churn(s.trans)[0]) <= 1.0
            # the labels of the interpolated scores, untracked: the kept map is not touched
            si = results.summary(lg, raw[i][0], interpolate=True, box=False)
            wi = image.labels_summary_host(results.labels_at_source(lg, raw[i][0], interpolate=True), rows, cols, rows, cols, 19)
            _same(tuple(si), (wi[0], None, None), "frame %d, interpolated" % i)
            assert (m.generation("labels"), m.generation("logits")) == gen
            before, kept = src, lab
        lg, lab = r.step(3, raw[3], 3)
        assert np.array_equal(lg.asnumpy(), base[3][0]) and np.array_equal(lab.asnumpy(), base[3][1])
        with pytest.raises(runtime.AccelError, match="stale"):
            results.summary(kept, raw[2][0], track=True)
        with pytest.raises(runtime.AccelError, match="logits"):
            results.summary(lab, raw[3][0], interpolate=True)
        # the refused call did not touch the kept map: frame 3 is compared with frame 2
        s = results.summary(lab, raw[3][0], track=True)
        assert np.array_equal(s.trans.reshape(19, 19).astype(np.int64), _fast_hist(results.labels_at_source(lab, raw[3][0]), before, 19))
    finally:
        tester.release_models()


TIMES = re.compile(r"\d+\.\d+s|\d+\.\d+ frames/s")


def test_demo_prints_shares_and_churn(demo_cfg, capsys):
    """--summary adds one line per frame -- the largest classes with share and box, the churn from the second frame of a clip on -- and changes no
    other line: without the flag the output is what it is without this feature"""
    from accel_amd import demo
    from accel_amd.core import tester
    argv = ["--version", "18", "--interval", "3", "--num_ex", "2", "--synthetic", "90x180", "--scales", "128x256", "--raw-frames", "--finish-on-gpu"]
    outs = []
    for extra in ([], ["--summary"]):
        try:
            demo.main(argv + extra)
        finally:
            tester.release_models()
        outs.append(capsys.readouterr().out)
    plain, with_summary = (TIMES.sub("T", o).splitlines() for o in outs)
    assert not any("summary" in line or "churn" in line for line in plain)
    lines = [line for line in with_summary if line.startswith("summary ")]
    assert [line for line in with_summary if not line.startswith("summary ")] == plain
    assert len(lines) == 6 and plain[-1] == "done"
    share_box = r"\d+:[01]\.\d{3}\[\d+,\d+,\d+,\d+\]"
    for i, line in enumerate(lines):
        churn = r" churn [01]\.\d{3}" if i % 3 else ""           # a clip is three frames: its first frame is compared with nothing
        assert re.fullmatch(r"summary %s( %s){0,2}%s" % (share_box, share_box, churn), line), (i, line)
    with pytest.raises(ValueError, match="finish-on-gpu"):
        demo.main(["--summary"])
