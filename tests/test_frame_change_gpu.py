"""Frame change on the GPU (csrc/frame_change.hip behind accel_frame_change / accel_model_frame_change / accel_model_frame_keep): the signature, the
changed-cell count, the sum of differences and the mask the kernel writes are those of accel_amd/utils/image.py frame_signature_host /
frame_change_host BIT FOR BIT -- the arithmetic is integer, so every comparison is np.array_equal: no tolerance -- on the smallest shapes at which the
kernel can go wrong (frame_change_ref.py), through every input route at the model level, and end to end: the adaptive schedule takes the key frames
the specification predicts and the frames come out as under the explicit schedule that names them.  (Host side: test_frame_change_cpu.py.)"""
import ctypes

import numpy as np
import pytest

from accel_amd.utils import image, synth

import frame_change_ref as ref

pytestmark = pytest.mark.gpu

MEANS = (103.06, 115.9, 123.15)


def _check(got, want, what):
    """(sig, changed, sad, mask) against the specification"""
    names = ("sig", "changed", "sad", "mask")
    for name, g, w in zip(names, got, (want.sig, want.changed, want.sad, want.mask)):
        assert g is not None and g.dtype == w.dtype and g.shape == w.shape, (what, name, None if g is None else (g.dtype, g.shape), w.dtype, w.shape)
        assert np.array_equal(g, w), "%s: %s differs in %d of %d places" % (what, name, int(np.count_nonzero(g != w)), w.size)


# ---- operator level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_kernel_equals_the_specification(ctx, case):
    s = case.shape
    cur, key = ref.frames(case)
    want = ref.expected(case)
    _check(ctx.frame_change(cur, s.out_h, s.out_w, s.cell, case.level_q, sig_key=want.sig_key), want, ref.case_id(case))
    # sig_key=None: the signature only
    alone = ctx.frame_change(key, s.out_h, s.out_w, s.cell)
    assert alone[1] is None and alone[2] is None and alone[3] is None
    assert alone[0].dtype == np.int32 and np.array_equal(alone[0], want.sig_key)


@pytest.mark.parametrize("case", [c for c in ref.CASES if c.values == "dyadic" and c.shape.n in (2, 3)], ids=ref.case_id)
def test_each_output_alone_equals_the_call_for_all_of_them(ctx, case):
    s, want = case.shape, ref.expected(case)
    cur, _ = ref.frames(case)
    args = (cur, s.out_h, s.out_w, s.cell, case.level_q)
    off = dict(sig=False, changed=False, sad=False, mask=False)
    for i, name in enumerate(("sig", "changed", "sad", "mask")):
        got = ctx.frame_change(*args, sig_key=want.sig_key, **dict(off, **{name: True}))
        assert [g is not None for g in got] == [j == i for j in range(4)], name
        assert np.array_equal(got[i], (want.sig, want.changed, want.sad, want.mask)[i]), name


def test_a_pitched_mask_keeps_the_bytes_between_its_rows(ctx):
    case = next(c for c in ref.CASES if c.shape.W == 80 and c.values == "dyadic")
    s, want = case.shape, ref.expected(case)
    cur, _ = ref.frames(case)
    gh, gw = image.frame_cells(s.out_h, s.out_w, s.cell)
    for pitch in (gw + 1, gw + 11):
        out = np.full((s.n, gh, pitch), 7, np.uint8)
        got = ctx.frame_change(cur, s.out_h, s.out_w, s.cell, case.level_q, sig_key=want.sig_key, mask=out)
        assert got[3] is out and np.array_equal(out[:, :, :gw], want.mask) and (out[:, :, gw:] == 7).all()
        assert np.array_equal(got[1], want.changed)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_err_arg(ctx):
    """every call the kernel could not honour is refused on the host, with a message that names the argument; nothing is written"""
    from accel_amd import runtime
    from test_frames_u8_gpu import _input_model
    lib = runtime.lib()
    n, H, W, out_h, out_w, cell = 1, 32, 64, 30, 50, 16
    gh, gw = image.frame_cells(out_h, out_w, cell)
    x = np.random.default_rng(5).uniform(-100, 100, (n, 3, H, W)).astype(np.float32)
    key = image.frame_signature_host(x[:, ::-1].copy(), out_h, out_w, cell)
    sig, changed, sad = np.zeros((n, gh, gw), np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    mask = np.zeros((n, gh, gw), np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    good = dict(img=x, key=key, n=n, H=H, W=W, out_h=out_h, out_w=out_w, cell=cell, level_q=64, sig=sig, changed=changed, sad=sad, mask=mask, mask_pitch=gw)
    m = _input_model(ctx, H, W)
    compared = ctypes.c_int(-5)
    try:
        with pytest.raises(runtime.AccelError, match="not an image input"):
            m.frame_change("data", n, out_h, out_w, cell, 64)
        m.plans["op"].finalize()                                # the image inputs are known as such once their plan is finalized
        m.write("data", x)
        m.frame_change("data", n, out_h, out_w, cell, 64)
        m.frame_keep()
        state = m.generation("data")
        calls = {
            "op": lambda a: lib.accel_frame_change(ctx.handle, vp(a["img"]), vp(a["key"]), a["n"], a["H"], a["W"], a["out_h"], a["out_w"], a["cell"],
                                                   a["level_q"], vp(a["sig"]), vp(a["changed"]), vp(a["sad"]), vp(a["mask"]), a["mask_pitch"]),
            "model": lambda a: lib.accel_model_frame_change(m.handle, b"data", a["n"], a["out_h"], a["out_w"], a["cell"], a["level_q"], vp(a["changed"]),
                                                            vp(a["sad"]), vp(a["mask"]), a["mask_pitch"], 0, ctypes.byref(compared)),
        }
        both, op, model = ("op", "model"), ("op",), ("model",)
        cases = [(dict(cell=12), "cell", both), (dict(cell=0), "cell", both), (dict(cell=128), "cell", both),
                 (dict(out_w=W + 1), "out_w", both), (dict(out_h=H + 1), "out_h", both), (dict(out_h=0), "out_h", both), (dict(out_w=0), "out_w", both),
                 (dict(level_q=32769), "level_q", both), (dict(level_q=-1), "level_q", both),
                 (dict(sig=None, changed=None, sad=None, mask=None), "all NULL", op),
                 (dict(key=None), "sig_key", op), (dict(key=None, changed=None, sad=None), "sig_key", op), (dict(key=None, changed=None, mask=None), "sig_key", op),
                 (dict(img=None), "img", op), (dict(n=0), "n =", both), (dict(n=32769), "n =", both), (dict(H=0), "H x W", op), (dict(W=32769), "H x W", op),
                 (dict(mask_pitch=gw - 1), "mask_pitch", both),
                 (dict(n=2), "n =", model)]                               # larger than the bound batch
        for change, word, names in cases:
            for name in names:
                rc = calls[name](dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (name, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg, (name, change, msg)
        assert lib.accel_frame_change(None, vp(x), None, n, H, W, out_h, out_w, cell, 0, vp(sig), None, None, None, 0) == -1
        assert lib.accel_model_frame_change(None, b"data", n, out_h, out_w, cell, 0, None, None, None, 0, 0, ctypes.byref(compared)) == -1
        assert lib.accel_model_frame_change(m.handle, b"data", n, out_h, out_w, cell, 0, None, None, None, 0, 0, None) == -1
        assert "compared" in lib.accel_last_error().decode()
        assert lib.accel_model_frame_change(m.handle, b"nothing", n, out_h, out_w, cell, 0, None, None, None, 0, 0, ctypes.byref(compared)) == -1
        assert "unknown buffer" in lib.accel_last_error().decode()
        assert lib.accel_model_frame_change(m.handle, b"y", n, out_h, out_w, cell, 0, None, None, None, 0, 0, ctypes.byref(compared)) == -1
        assert "not an image input" in lib.accel_last_error().decode()
        assert lib.accel_model_frame_keep(None) == -1
        bare = runtime.Model(ctx)                               # no signature has been made
        assert lib.accel_model_frame_keep(bare.handle) == -1
        assert "no signature" in lib.accel_last_error().decode()
        bare.close()
        # a pitch of a mask that is left out is not looked at
        assert calls["op"](dict(good, mask=None, mask_pitch=0)) == 0, lib.accel_last_error().decode()
        # none of the refused calls reached the model or the destinations
        assert compared.value == -5 and m.generation("data") == state
        for a in (sig, changed, sad, mask):
            a[...] = 0
        want = image.frame_change_host(image.frame_signature_host(x, out_h, out_w, cell), key, out_h, out_w, cell, 64)
        assert calls["op"](good) == 0, lib.accel_last_error().decode()
        assert np.array_equal(sig, image.frame_signature_host(x, out_h, out_w, cell))
        assert np.array_equal(changed, want[0]) and np.array_equal(sad, want[1]) and np.array_equal(mask, want[2]) and want[0][0] > 0
        assert calls["model"](good) == 0 and compared.value == 1, lib.accel_last_error().decode()
        assert changed[0] == 0 and sad[0] == 0 and not mask.any()      # the kept frame is the frame itself
    finally:
        ctx.sync()
        m.close()


# ---- model level ------------------------------------------------------------------------------------------------------------------
def _spec(x, kept, out_h, out_w, cell, level_q):
    sig = image.frame_signature_host(x, out_h, out_w, cell)
    return sig, image.frame_change_host(sig, kept, out_h, out_w, cell, level_q)


def _same_change(got, want, what):
    assert got is not None, "%s: nothing was compared" % what
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, g, w)


def _frames_model(ctx, N, H, W):
    """a model with the image inputs `data` / `data_key` of N frames of H x W (the one-op plan of test_frames_u8_gpu._input_model with room for N
    frames, finalized so that the inputs are known as such; never run)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    ib, h2, w2 = N * 3 * H * W * 4, H // 2, W // 2
    arena = (h2 * w2 * 32 + 255) // 256 * 256
    m.add_plan("op", "option graph=0 tune=0\narena bytes=%d\npbuf name=data bytes=%d\npbuf name=data_key bytes=%d\npbuf name=y bytes=%d\n"
                     "prep_flow cur=data:0:3:4:%d:%d prev=data_key:0:3:4:%d:%d dst=A:0:6:8:%d:%d H=%d W=%d\n"
                     "export_nchw src=A:0:6:8:%d:%d dst=y:0:6:8:%d:%d\n"
               % (arena, ib, ib, 6 * h2 * w2 * 4, H, W, H, W, h2, w2, H, W, h2, w2, h2, w2)).finalize()
    return m


def test_model_frame_change_through_every_input_route(ctx):
    """a model bound for 2 frames of 128 x 256; frames of 120 x 250 land in a valid region of 123 x 256 (scale 1.024)"""
    import torch
    from accel_amd import runtime
    from test_frames_nv12_gpu import _host as _nv12_host
    from test_frames_u8_gpu import _geometry, _host as _u8_host
    N, H, W, rows, cols, cell, level_q = 2, 128, 256, 120, 250, 16, 640
    g = _geometry(rows, cols, H, W)
    out_h, out_w = g["out_h"], g["out_w"]
    assert (out_h, out_w, g["H"], g["W"]) == (123, 256, H, W)
    rng = np.random.default_rng(77)
    a = rng.uniform(-120, 130, (N, 3, H, W)).astype(np.float32)
    b = a.copy()
    b[0, :, 16:64, 32:200] += 40.0                    # frame 0 changes in a patch, frame 1 by less than the level everywhere
    b[1] += 5.0
    a[:, :, out_h:, :] = np.nan                        # the padding is never looked at
    b[:, :, out_h:, :] = 3e38
    m = _frames_model(ctx, N, H, W)
    try:
        with pytest.raises(runtime.AccelError, match="no signature"):
            m.frame_keep()
        m.write("data", a)
        gen = m.generation("data"), m.generation("data_key")
        # nothing is kept yet: nothing is compared
        assert m.frame_change("data", N, out_h, out_w, cell, level_q) is None
        m.frame_keep()
        kept = image.frame_signature_host(a, out_h, out_w, cell)
        # the same frame: no cell changed, no difference at all
        same = m.frame_change("data", N, out_h, out_w, cell, level_q, mask=True)
        assert same is not None and not same[0].any() and not same[1].any() and not same[2].any()
        assert (m.generation("data"), m.generation("data_key")) == gen, "frame_change / frame_keep must not count as writes"
        # another frame, written as fp32
        m.write("data", b)
        gen = m.generation("data")
        _, want = _spec(b, kept, out_h, out_w, cell, level_q)
        assert want[0][0] > 0 and want[0][1] == 0 and want[1][1] > 0
        _same_change(m.frame_change("data", N, out_h, out_w, cell, level_q, mask=True), want, "write")
        _same_change(m.frame_change("data", N, out_h, out_w, cell, level_q), want[:2], "write, no mask")
        # the other image input
        m.write("data_key", b)
        _same_change(m.frame_change("data_key", N, out_h, out_w, cell, level_q, mask=True), want, "data_key")
        # BGR bytes and NV12 bytes, converted by the GPU on the way in
        f8 = rng.integers(0, 256, (N, rows, cols, 3), dtype=np.uint8)
        m.write_u8("data", f8, MEANS, **g)
        _same_change(m.frame_change("data", N, out_h, out_w, cell, level_q, mask=True),
                     _spec(_u8_host(f8, H, W), kept, out_h, out_w, cell, level_q)[1], "write_u8")
        nv = image.bgr_to_nv12_host(f8, 2)
        m.write_nv12("data", nv, rows, cols, MEANS, colour=2, **g)
        _same_change(m.frame_change("data", N, out_h, out_w, cell, level_q, mask=True),
                     _spec(_nv12_host(nv, rows, cols, H, W, colour=2), kept, out_h, out_w, cell, level_q)[1], "write_nv12")
        # a zero-copy binding, 4-byte but not 16-byte aligned: what is read is what the plans would read, not the model's own copy
        dev = torch.zeros(b.size + 1, dtype=torch.float32, device="cuda")
        dev[1:] = torch.from_numpy(b.reshape(-1))
        torch.cuda.synchronize()                     # torch's stream and the library's compute stream are not ordered by themselves
        ptr = dev.data_ptr() + 4
        assert ptr % 16 == 4
        m.bind_device("data", ptr, b.nbytes)
        gen = m.generation("data")
        _same_change(m.frame_change("data", N, out_h, out_w, cell, level_q, mask=True), want, "bound device pointer")
        # ... and into caller-owned HBM, a pitched mask among the destinations
        gh, gw = image.frame_cells(out_h, out_w, cell)
        dc = torch.full((N,), 7, dtype=torch.int32, device="cuda")
        ds = torch.full((N,), 7, dtype=torch.int64, device="cuda")
        dm = torch.full((N, gh, gw + 5), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert m.frame_change_device("data", N, out_h, out_w, cell, level_q, dc.data_ptr(), ds.data_ptr(), dm.data_ptr(), gw + 5) is True
        m.ctx.sync()
        hm = dm.cpu().numpy()
        assert np.array_equal(dc.cpu().numpy().astype(np.uint32), want[0]) and np.array_equal(ds.cpu().numpy().astype(np.uint64), want[1])
        assert np.array_equal(hm[:, :, :gw], want[2]) and (hm[:, :, gw:] == 7).all()
        assert m.generation("data") == gen
        # fewer frames than the model is bound for: another geometry, so nothing to compare with until it is kept
        assert m.frame_change("data", 1, out_h, out_w, cell, level_q) is None
        m.frame_keep()
        assert m.frame_change("data", N, out_h, out_w, cell, level_q) is None
        m.write("data", a)                             # (ends the binding)
        _same_change(m.frame_change("data", 1, out_h, out_w, cell, level_q, mask=True),
                     _spec(a[:1], image.frame_signature_host(b[:1], out_h, out_w, cell), out_h, out_w, cell, level_q)[1], "n = 1")
        with pytest.raises(runtime.AccelError, match="n = 3"):
            m.frame_change("data", 3, out_h, out_w, cell, level_q)
        # kept under cell 16, asked under cell 32: not compared; nor under another valid region
        m.frame_change("data", N, out_h, out_w, 16, level_q)
        m.frame_keep()
        assert m.frame_change("data", N, out_h, out_w, 32, level_q) is None
        assert m.frame_change("data", N, out_h - 1, out_w, 16, level_q) is None
        assert m.frame_change("data", N, out_h, out_w, 16, level_q) is not None
        with pytest.raises(runtime.AccelError, match="not an image input"):
            m.frame_change("y", N, out_h, out_w, cell, level_q)
        del dev, dc, ds, dm
    finally:
        ctx.sync()
        m.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _run(runner, batches, interval, schedule):
    outs, keys, changes = [], [], []
    for i, arrays in enumerate(batches):
        lg, lab = runner.step(i, arrays, interval, schedule=schedule)
        outs.append((lg.asnumpy().copy(), lab.asnumpy().copy()))
        if runner.last_key:
            keys.append(i)
        changes.append(runner.last_change)
    return outs, keys, changes


def _identical(got, want, what):
    assert len(got) == len(want)
    for t, ((lg, lab), (rlg, rlab)) in enumerate(zip(got, want)):
        assert np.array_equal(lg, rlg), "%s, frame %d: logits differ by %g" % (what, t, float(np.abs(lg - rlg).max()))
        assert np.array_equal(lab, rlab), "%s, frame %d: labels differ" % (what, t)


def test_adaptive_schedule_takes_the_key_frames_the_specification_predicts(demo_cfg):
    """Accel-18 at 128 x 256 with seeded weights, six raw BGR frames with a cut at frame 3"""
    from accel_amd import demo
    from accel_amd.core import tester
    from accel_amd.core.schedule import KeySchedule
    H, W = 128, 256
    demo_cfg.SCALES[0] = (H, W)
    frames = synth.make_clip(H, W, 6, seed=1)[0:3] + synth.make_clip(H, W, 6, seed=2)[3:6]
    adaptive = lambda: KeySchedule.adaptive(share=0.25, level=16, cell=32, max_interval=5)
    # the oracle: the specification on the tensors the host would build
    tensors = [image.transform(f, demo_cfg.network.PIXEL_MEANS).astype(np.float32) for f in frames]
    s, kept, want_keys, want_changes = adaptive(), None, [], []
    for t, x in enumerate(tensors):
        sig = image.frame_signature_host(x, H, W, s.cell)
        change = None
        if kept is not None:
            c, d, _ = image.frame_change_host(sig, kept, H, W, s.cell, s.level_q)
            change = [(int(c[0]), sig[0].size, int(d[0]))]
        want_changes.append(change)
        if s.decide(t, change):
            want_keys.append(t)
            kept = sig
    assert want_keys == [0, 3], (want_keys, want_changes)
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        batches = demo.build_batches(frames, demo_cfg, raw=True)
        got, keys, changes = _run(r, batches, 5, adaptive())
        assert keys == want_keys and changes == want_changes, (keys, changes, want_changes)
        explicit, keys, changes = _run(r, demo.build_batches(frames, demo_cfg, raw=True), 5, KeySchedule.explicit([0, 3]))
        assert keys == [0, 3] and changes == [None] * 6
        _identical(got, explicit, "adaptive against explicit([0, 3])")
        assert not np.array_equal(got[2][0], got[3][0])
        # and the pinned prefetch loop finds the staged frame as the plain loop does
        pinned = demo.build_batches(frames, demo_cfg, pinned=True, raw=True)
        s, outs = adaptive(), []
        for i, arrays in enumerate(pinned):
            lg, lab = r.step(i, arrays, 5, schedule=s)
            if i + 1 < len(pinned):
                assert r.prefetch(pinned[i + 1])
            outs.append((lg.asnumpy().copy(), lab.asnumpy().copy()))
        _identical(outs, explicit, "adaptive, pinned prefetch loop")
        # schedule=None is the fixed rule
        for interval in (3,):
            plain, _, _ = _run(r, demo.build_batches(frames, demo_cfg, raw=True), interval, None)
            fixed, keys, _ = _run(r, demo.build_batches(frames, demo_cfg, raw=True), interval, KeySchedule.fixed(interval))
            assert keys == [0, 3]
            _identical(plain, fixed, "schedule=None against fixed(%d)" % interval)
            _identical(fixed, explicit, "fixed(3) takes the same key frames here")
    finally:
        tester.release_models()


def test_demo_marks_its_key_frames(demo_cfg, capsys):
    """two synthetic clips of three frames: the second starts with a cut, which the adaptive schedule takes as a key frame"""
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "3", "--num_ex", "2", "--synthetic", "128x256", "--raw-frames", "--adaptive-key", "0.25"])
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("testing ")]
    assert out.rstrip().endswith("done") and len(lines) == 6, out[-1500:]
    assert lines[0].endswith(" key") and " share " not in lines[0]
    keys = [i for i, ln in enumerate(lines) if " key" in ln]
    assert keys == [0, 3], lines
    for i, ln in enumerate(lines[1:], 1):
        share = float(ln.split(" share ")[1])
        assert (share > 0.25) == (i in keys) and 0.0 <= share <= 1.0, ln
