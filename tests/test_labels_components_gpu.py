"""Connected components of finished frames on the GPU (csrc/labels_components.hip behind accel_labels_components and the accel_model_* forms): the
count, the records, the coordinate sums and the per-pixel object index are what utils.image.labels_components_host gives -- EXACTLY.  Everything is
integer arithmetic, so every comparison is np.array_equal: no tolerance.  (Host side, and the wrong kernels the cases tell apart:
test_labels_components_cpu.py.)"""
import ctypes
import re

import numpy as np
import pytest

from accel_amd.utils import image, synth

import components_ref as ref
import interp_ref
from test_interp_labels_gpu import _logits_model
from test_results_gpu import STRIDE, _labels_model, _steps

pytestmark = pytest.mark.gpu

NAMES = ("count", "comp", "sums", "ids")


def _same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        if b is None:
            assert a is None, (what, name)
            continue
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape, (what, name, None if a is None else (a.dtype, a.shape))
        assert np.array_equal(a, b), (what, name, int(np.count_nonzero(a != b)))


def _spec(labels, out_h, out_w, h, w, ncls, **kw):
    return image.labels_components_host(labels, out_h, out_w, h, w, ncls, ids=True, **kw)


# ---- operator level ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_the_kernels_equal_the_specification(ctx, case):
    s = case.shape
    got = ctx.labels_components(ref.labels(s, case.pattern), s.out_h, s.out_w, s.h, s.w, s.ncls, connectivity=case.connectivity,
                                min_area=case.min_area, max_components=case.max_components, ids=True)
    _same(got, ref.expected(case), ref.case_id(case))


@pytest.mark.parametrize("case", [c for c in ref.CASES if c.shape in (ref.CROP, ref.LARGER) and c.pattern in ("uniform", "runs")], ids=ref.case_id)
def test_each_output_alone_equals_the_call_for_all_of_them(ctx, case):
    s = case.shape
    want = ref.expected(case)
    run = lambda **kw: ctx.labels_components(ref.labels(s, case.pattern), s.out_h, s.out_w, s.h, s.w, s.ncls, connectivity=case.connectivity,
                                             min_area=case.min_area, max_components=case.max_components, **kw)
    _same(run(comp=False, sums=False), (want.count, None, None, None), "count alone")
    _same(run(sums=False), (want.count, want.comp, None, None), "comp alone")
    _same(run(comp=False), (want.count, None, want.sums, None), "sums alone")
    _same(run(comp=False, sums=False, ids=True), (want.count, None, None, want.ids), "ids alone")


@pytest.mark.parametrize("case", ref.PITCHED, ids=ref.case_id)
def test_pitched_ids_leave_the_words_between_rows_alone(ctx, case):
    s = case.shape
    want = ref.expected(case)
    for extra in (1, 4, 7):
        out = np.random.default_rng(extra).integers(1, 1 << 30, (s.n, s.h, s.w + extra), dtype=np.int32)
        before = out.copy()
        got = ctx.labels_components(ref.labels(s, case.pattern), s.out_h, s.out_w, s.h, s.w, s.ncls, connectivity=case.connectivity,
                                    min_area=case.min_area, max_components=case.max_components, ids=out, width=s.w)
        assert got[3] is out
        assert np.array_equal(out[:, :, :s.w], want.ids), ("ids at a pitch of %d words" % (s.w + extra), int(np.count_nonzero(out[:, :, :s.w] != want.ids)))
        assert np.array_equal(out[:, :, s.w:], before[:, :, s.w:]), "words between the rows were written"
        _same(got[:3], want[:3], "pitch %d" % (s.w + extra))


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_model_forms_and_their_scratch(ctx):
    """host and device destinations of the labels form; two calls of different sizes in a row reuse (and regrow) the model's scratch"""
    import torch
    case = next(c for c in ref.CASES if c.shape is ref.CROP and c.pattern == "runs" and c.connectivity == 8 and c.min_area == 1)
    s = case.shape
    labels, want = ref.labels(s, case.pattern), ref.expected(case)
    m = _labels_model(ctx, s.n, s.H, s.W)
    try:
        m.write("labels", labels)
        gen = m.generation("labels")
        kw = dict(connectivity=8, min_area=1, max_components=case.max_components)
        small = _spec(labels[:1], 40, 70, 33, 61, s.ncls, connectivity=4, min_area=2, max_components=64)
        _same(m.labels_components(1, 40, 70, 33, 61, s.ncls, connectivity=4, min_area=2, max_components=64, ids=True), small, "a small call first")
        _same(m.labels_components(s.n, s.out_h, s.out_w, s.h, s.w, s.ncls, ids=True, **kw), want, "then a larger one")
        _same(m.labels_components(1, 40, 70, 33, 61, s.ncls, connectivity=4, min_area=2, max_components=64, ids=True), small, "and the small one again")
        _same(m.labels_components(s.n, s.out_h, s.out_w, s.h, s.w, s.ncls, comp=False, sums=False, **kw), (want.count, None, None, None), "count alone")
        # device destinations, ids at a padded pitch
        mc, pitch = case.max_components, s.w + 3
        dev = [torch.full((size,), 7, dtype=dtype, device="cuda") for size, dtype in ((s.n, torch.int32), (s.n * mc * 8, torch.int32),
                                                                                     (s.n * mc * 2, torch.int64), (s.n * s.h * pitch, torch.int32))]
        torch.cuda.synchronize()                                 # torch's stream and the library's compute stream are not ordered by themselves
        m.labels_components_device(s.n, s.out_h, s.out_w, s.h, s.w, s.ncls, count_ptr=dev[0].data_ptr(), comp_ptr=dev[1].data_ptr(),
                                   sums_ptr=dev[2].data_ptr(), ids_ptr=dev[3].data_ptr(), ids_pitch=4 * pitch, **kw)
        ctx.sync()
        assert np.array_equal(dev[0].cpu().numpy(), want.count)
        assert np.array_equal(dev[1].cpu().numpy().reshape(s.n, mc, 8), want.comp)
        assert np.array_equal(dev[2].cpu().numpy().view(np.uint64).reshape(s.n, mc, 2), want.sums)
        ids = dev[3].cpu().numpy().reshape(s.n, s.h, pitch)
        assert np.array_equal(ids[:, :, :s.w], want.ids) and (ids[:, :, s.w:] == 7).all()
        assert m.generation("labels") == gen and np.array_equal(m.read("labels", (s.n, s.H, s.W), np.uint8), labels)
        del dev
    finally:
        ctx.sync()
        m.close()


@pytest.mark.parametrize("case", interp_ref.pitched_cases() + [c for c in interp_ref.dyadic_cases() if c.kind == "ints" and c.ncls == 19],
                         ids=interp_ref.ident)
def test_the_scores_form_finds_the_components_of_the_interpolated_labels(ctx, case):
    """the inputs of the interpolated-label tests, whose guard condition (test_interp_labels_cpu.py) makes equality of every label a fair demand"""
    import torch
    labels = interp_ref.reference(case)
    m = _logits_model(ctx, case.n, case.ncls, case.H, case.W)
    try:
        m.write("logits", interp_ref.scores(case))
        gen = m.generation("logits")
        for conn, area in ((8, 1), (4, 2)):
            want = _spec(labels, case.h, case.w, case.h, case.w, 19, connectivity=conn, min_area=area, max_components=4096)
            assert int(want[0].max()) <= 4096
            _same(m.scores_components(case.n, case.out_h, case.out_w, case.h, case.w, 19, connectivity=conn, min_area=area, max_components=4096, ids=True),
                  want, "connectivity %d, min_area %d" % (conn, area))
        want = _spec(labels, case.h, case.w, case.h, case.w, 19, max_components=4096)
        dev = [torch.full((size,), 7, dtype=dtype, device="cuda") for size, dtype in ((case.n, torch.int32), (case.n * 4096 * 8, torch.int32))]
        torch.cuda.synchronize()
        m.scores_components_device(case.n, case.out_h, case.out_w, case.h, case.w, 19, max_components=4096, count_ptr=dev[0].data_ptr(),
                                   comp_ptr=dev[1].data_ptr())
        ctx.sync()
        assert np.array_equal(dev[0].cpu().numpy(), want[0]) and np.array_equal(dev[1].cpu().numpy().reshape(case.n, 4096, 8), want[1])
        assert m.generation("logits") == gen
        del dev
    finally:
        ctx.sync()
        m.close()


# ---- argument errors --------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_err_arg(ctx):
    """every call the kernels could not honour is refused on the host, with a message that names the argument; nothing is launched, nothing is
    written, and the next accepted call is right"""
    import torch
    from accel_amd import runtime
    lib = runtime.lib()
    n, H, W, out_h, out_w, h, w, ncls, mc = 2, 32, 64, 31, 54, 29, 50, 19, 256
    rng = np.random.default_rng(4)
    labels = np.repeat(rng.integers(0, ncls + 2, n * H * W // 8, dtype=np.uint8), 8).reshape(n, H, W)
    count, comp, sums = np.zeros(n, np.int32), np.zeros((n, mc, 8), np.int32), np.zeros((n, mc, 2), np.uint64)
    ids = np.zeros((n, h, w), np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    good = dict(labels=labels, n=n, H=H, W=W, out_h=out_h, out_w=out_w, h=h, w=w, ncls=ncls, connectivity=8, min_area=1, max_components=mc,
                count=count, comp=comp, sums=sums, ids=ids, ids_pitch=4 * w)
    m, lm = _labels_model(ctx, n, H, W), _logits_model(ctx, n, 19, H, W)
    try:
        m.write("labels", labels)
        lm.write("logits", rng.standard_normal((n, 19, H, W)).astype(np.float32))
        gen = m.generation("labels"), lm.generation("logits")
        tail = lambda a: (a["connectivity"], a["min_area"], a["max_components"])
        outs = lambda a: (vp(a["count"]), vp(a["comp"]), vp(a["sums"]), vp(a["ids"]), a["ids_pitch"])
        calls = {
            "op": lambda a: lib.accel_labels_components(ctx.handle, vp(a["labels"]), a["n"], a["H"], a["W"], a["out_h"], a["out_w"], a["h"], a["w"],
                                                        a["ncls"], *(tail(a) + outs(a))),
            "labels": lambda a: lib.accel_model_labels_components(m.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], a["ncls"],
                                                                  *(tail(a) + (0,) + outs(a))),
            "scores": lambda a: lib.accel_model_scores_components(lm.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], a["ncls"],
                                                                  *(tail(a) + (0,) + outs(a))),
        }
        every, models = tuple(calls), ("labels", "scores")
        cases = [(dict(n=0), "n =", every), (dict(n=-1), "n =", every), (dict(n=32769), "n =", every), (dict(h=0), "h =", every), (dict(w=0), "w =", every),
                 (dict(h=32769), "h =", every), (dict(w=32769), "w =", every), (dict(out_h=H + 1), "out_h", every), (dict(out_w=W + 1), "out_w", every),
                 (dict(out_h=0), "out_h", every), (dict(out_w=0), "out_w", every), (dict(H=0), "H x W", ("op",)), (dict(W=32769), "H x W", ("op",)),
                 (dict(ncls=0), "ncls", every), (dict(ncls=33), "ncls", every), (dict(labels=None), "labels", ("op",)),
                 (dict(connectivity=6), "connectivity", every), (dict(connectivity=0), "connectivity", every),
                 (dict(min_area=0), "min_area", every), (dict(min_area=-3), "min_area", every),
                 (dict(max_components=0), "max_components", every), (dict(max_components=65537), "max_components", every),
                 (dict(count=None), "count", every), (dict(count=None, comp=None, sums=None, ids=None), "count", every),
                 (dict(ids_pitch=4 * w - 4), "ids_pitch", every), (dict(ids_pitch=4 * w + 2), "ids_pitch", every),
                 (dict(n=n + 1), "n =", models), (dict(ncls=21), "ncls", ("scores",))]
        for change, word, names in cases:
            for name in names:
                rc = calls[name](dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (name, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg, (name, change, msg)
        assert lib.accel_labels_components(None, vp(labels), n, H, W, out_h, out_w, h, w, ncls, 8, 1, mc, vp(count), None, None, None, 0) == -1
        assert lib.accel_model_labels_components(None, n, out_h, out_w, h, w, ncls, 8, 1, mc, 0, vp(count), None, None, None, 0) == -1
        assert lib.accel_model_scores_components(None, n, out_h, out_w, h, w, ncls, 8, 1, mc, 0, vp(count), None, None, None, 0) == -1
        assert lib.accel_model_labels_components(lm.handle, n, out_h, out_w, h, w, ncls, 8, 1, mc, 0, vp(count), None, None, None, 0) == -1
        assert "labels" in lib.accel_last_error().decode()       # a model without label maps
        assert lib.accel_model_scores_components(m.handle, n, out_h, out_w, h, w, ncls, 8, 1, mc, 0, vp(count), None, None, None, 0) == -1
        assert "logits" in lib.accel_last_error().decode()       # and one without scores
        # misaligned device destinations: 4 bytes for the int32 words, 8 for the sums
        dev = torch.full((n * mc * 8 + n * h * w + 64,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        base = dev.data_ptr()
        dp = lambda v: ctypes.c_void_p(v) if v else None
        for word, ptrs in (("count", (base + 2, 0, 0, 0)), ("comp", (base, base + 65, 0, 0)), ("sums", (base, 0, base + 68, 0)), ("ids", (base, 0, 0, base + 67))):
            for fn, handle in ((lib.accel_model_labels_components, m.handle), (lib.accel_model_scores_components, lm.handle)):
                rc = fn(handle, n, out_h, out_w, h, w, ncls, 8, 1, mc, 1, dp(ptrs[0]), dp(ptrs[1]), dp(ptrs[2]), dp(ptrs[3]), 4 * w)
                msg = lib.accel_last_error().decode()
                assert rc == -1 and word in msg and "aligned" in msg, (word, rc, msg)
        ctx.sync()
        assert (dev.cpu().numpy() == 7).all()
        # none of the refused calls wrote anything or reached the models
        assert not count.any() and not comp.any() and not sums.any() and not ids.any()
        assert (m.generation("labels"), lm.generation("logits")) == gen
        # and every call is accepted as it stands, and right
        want = _spec(labels, out_h, out_w, h, w, ncls, max_components=mc)
        assert int(want[0].max()) <= mc
        assert calls["op"](good) == 0, lib.accel_last_error().decode()
        _same((count, comp, sums, ids), want, "the operator call")
        for a in (count, comp, sums, ids):
            a[...] = 0
        assert calls["labels"](good) == 0, lib.accel_last_error().decode()
        _same((count, comp, sums, ids), want, "the labels form")
        assert calls["scores"](good) == 0, lib.accel_last_error().decode()
        interpolated = lm.scores_labels(n, out_h, out_w, h, w)
        _same((count, comp, sums, ids), _spec(interpolated, h, w, h, w, ncls, max_components=mc), "the scores form")
        del dev
    finally:
        ctx.sync()
        m.close()
        lm.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def test_components_on_accel18(demo_cfg):
    """Accel-18 at 128 x 256 on the synthetic clip, raw frames of 90 x 180: the objects of a key frame and a non-key frame are found on the GPU and
    equal the specification applied to the fetched labels; the calls change nothing"""
    from accel_amd import demo, runtime
    from accel_amd.core import results, tester
    H, W, rows, cols = 128, 256, 90, 180
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = STRIDE
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    frames = synth.make_clip(rows, cols, 3)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        raw = demo.build_batches(frames, demo_cfg, raw=True)
        base = _steps(r, raw, 3, 3)
        kept = None
        for i in (0, 1):
            lg, lab = r.step(i, raw[i], 3)
            assert np.array_equal(lg.asnumpy(), base[i][0]) and np.array_equal(lab.asnumpy(), base[i][1])      # undisturbed by the calls before
            m = lab.device_ref[0]
            gen = m.generation("labels"), m.generation("logits")
            src = results.labels_at_source(lab, raw[i][0])
            for kw in (dict(), dict(connectivity=4, min_area=16, max_components=8)):
                c = results.components(lab, raw[i][0], ids=True, **kw)
                assert isinstance(c, results.Components)
                _same(tuple(c), _spec(src, rows, cols, rows, cols, 19, **kw), "frame %d %s" % (i, kw))
            c = results.components(lab, raw[i][0])
            assert c.ids is None
            rec, sums = results.components_of(c, 0)
            assert int(rec[:, 1].sum()) == int((src[0] < 19).sum()) and len(rec) == min(int(c.count[0]), 1024)
            ci = results.components(lg, raw[i][0], interpolate=True, ids=True)
            si = results.labels_at_source(lg, raw[i][0], interpolate=True)
            _same(tuple(ci), _spec(si, rows, cols, rows, cols, 19), "frame %d, interpolated" % i)
            assert (m.generation("labels"), m.generation("logits")) == gen
            kept = lab
        lg, lab = r.step(2, raw[2], 3)
        assert np.array_equal(lg.asnumpy(), base[2][0]) and np.array_equal(lab.asnumpy(), base[2][1])
        with pytest.raises(runtime.AccelError, match="stale"):
            results.components(kept, raw[1][0])
        with pytest.raises(runtime.AccelError, match="logits"):
            results.components(lab, raw[2][0], interpolate=True)
    finally:
        tester.release_models()


TIMES = re.compile(r"\d+\.\d+s|\d+\.\d+ frames/s")


def test_demo_prints_objects_per_class(demo_cfg, capsys):
    """--components adds one line per frame -- the objects per class and the largest one -- and changes no other line: without the flag the output
    is what it is without this feature"""
    from accel_amd import demo
    from accel_amd.core import tester
    argv = ["--version", "18", "--interval", "3", "--num_ex", "1", "--synthetic", "90x180", "--scales", "128x256", "--raw-frames", "--finish-on-gpu"]
    outs = []
    for extra in ([], ["--components"]):
        try:
            demo.main(argv + extra)
        finally:
            tester.release_models()
        outs.append(capsys.readouterr().out)
    plain, with_flag = (TIMES.sub("T", o).splitlines() for o in outs)
    assert not any(line.startswith("components") for line in plain)
    lines = [line for line in with_flag if line.startswith("components ")]
    assert [line for line in with_flag if not line.startswith("components ")] == plain
    assert len(lines) == 3 and plain[-1] == "done"
    for line in lines:
        assert re.fullmatch(r"components( \d+:\d+)*( largest \d+\[\d+,\d+,\d+,\d+\]=\d+)?( \(truncated\))?", line.rstrip()), line
    with pytest.raises(ValueError, match="finish-on-gpu"):
        demo.main(["--components"])
