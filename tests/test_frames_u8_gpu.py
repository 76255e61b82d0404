"""uint8 video frames on the GPU (csrc/frames_u8.hip behind accel_frame_u8 / accel_model_write_u8 / _prefetch_u8 / _commit_u8): the tensor the
kernel writes is the one accel_amd/utils/image.py builds on the host -- transform(resize(frame)) as fp32 -- BIT FOR BIT.  These are fp32 values
with one defined rounding (float64 arithmetic in numpy's order, one conversion to fp32), so every comparison is np.array_equal: no tolerance.
(Host side: test_frames_u8_cpu.py.)"""
import ctypes

import numpy as np
import pytest

from accel_amd.utils import image, synth

pytestmark = pytest.mark.gpu

MEANS = (103.06, 115.9, 123.15)
STRIDE = 16

# (rows, cols, target, max): scale 1 without padding (landscape, portrait) / up with padded columns / up with padded rows / up / down / down /
# portrait down with padded rows / portrait with both padded / down to a 16-row image
SMALL = [(48, 96, 48, 96), (96, 48, 48, 96), (45, 83, 48, 96), (37, 91, 64, 128), (33, 57, 48, 96), (60, 120, 48, 96),
         (50, 100, 64, 96), (100, 75, 48, 96), (61, 47, 48, 80), (23, 150, 48, 96)]
FULL = [(1024, 2048, 1024, 2048),      # the BASELINE frame: scale 1
        (720, 1280, 1024, 2048)]       # a full-size resample


def _host(frames, target, max_size, stride=STRIDE, means=MEANS):
    return np.concatenate([image.transform(image.resize(f, target, max_size, stride=stride)[0], means) for f in frames]).astype(np.float32)


def _geometry(rows, cols, target, max_size, stride=STRIDE):
    scale, out_h, out_w, H, W = image.resize_geometry(rows, cols, target, max_size, stride)
    return dict(out_h=out_h, out_w=out_w, step=image.resample_step(rows, cols, scale, out_h, out_w), H=H, W=W)


def _frames(n, rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)


def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ from the host path, first at %s: %r != %r"
                             % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- operator level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,target,max_size", SMALL + FULL)
def test_frame_u8_equals_the_host_path(ctx, rows, cols, target, max_size):
    f = _frames(1, rows, cols, rows * 4096 + cols)
    g = _geometry(rows, cols, target, max_size)
    _same(ctx.frame_u8(f, MEANS, **g), _host(f, target, max_size), (rows, cols, target, max_size, g))


@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (45, 83, 48, 96), (100, 75, 48, 96)])
def test_frame_u8_batch_of_three(ctx, rows, cols, target, max_size):
    f = _frames(3, rows, cols, 77 + rows)
    got = ctx.frame_u8(f, MEANS, **_geometry(rows, cols, target, max_size))
    assert got.shape[0] == 3 and not np.array_equal(got[0], got[1])
    _same(got, _host(f, target, max_size), "batch of 3")


@pytest.mark.parametrize("rows,cols,target,max_size,pitch", [(48, 96, 48, 96, 3 * 96 + 32),      # multiple of 4: the three-dword path
                                                             (48, 96, 48, 96, 3 * 96 + 7),       # odd pitch: scalar loads
                                                             (60, 120, 48, 96, 3 * 120 + 13)])   # resampled
def test_frame_u8_row_pitch_larger_than_a_row(ctx, rows, cols, target, max_size, pitch):
    f = _frames(2, rows, cols, pitch)
    padded = np.random.default_rng(pitch + 1).integers(0, 256, (2, rows, pitch), dtype=np.uint8)      # the bytes between rows are not zero
    padded[:, :, :3 * cols] = f.reshape(2, rows, 3 * cols)
    got = ctx.frame_u8(padded, MEANS, width=cols, **_geometry(rows, cols, target, max_size))
    _same(got, _host(f, target, max_size), "pitch %d" % pitch)


@pytest.mark.parametrize("rows,cols,stride", [(48, 90, 16),      # w % 4 != 0: scalar loads, the last quad of a row is half frame, half padding
                                              (48, 93, 16),
                                              (31, 50, 0),       # no padding at all, W % 4 != 0: scalar stores with a tail
                                              (17, 33, 0)])
def test_frame_u8_width_not_divisible_by_four_at_scale_one(ctx, rows, cols, stride):
    f = _frames(2, rows, cols, cols)
    target, max_size = min(rows, cols), max(rows, cols)
    g = _geometry(rows, cols, target, max_size, stride)
    assert g["step"] == 1.0 and (g["out_h"], g["out_w"]) == (rows, cols)
    _same(ctx.frame_u8(f, MEANS, **g), _host(f, target, max_size, stride), (rows, cols, stride))


@pytest.mark.parametrize("level", [0, 255])
@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (45, 83, 48, 96), (60, 120, 48, 96)])
def test_frame_u8_constant_frames(ctx, level, rows, cols, target, max_size):
    f = np.full((1, rows, cols, 3), level, np.uint8)
    g = _geometry(rows, cols, target, max_size)
    got = ctx.frame_u8(f, MEANS, **g)
    _same(got, _host(f, target, max_size), "constant %d" % level)
    for c in range(3):      # a resample of a constant frame is the constant; the padding is fp32(0 - mean), not 0
        assert np.all(got[0, 2 - c, :g["out_h"], :g["out_w"]] == np.float32(float(level) - MEANS[c]))
        assert np.all(got[0, 2 - c, g["out_h"]:, :] == np.float32(0.0 - MEANS[c]))
        assert np.all(got[0, 2 - c, :, g["out_w"]:] == np.float32(0.0 - MEANS[c]))


def test_frame_u8_other_means(ctx):
    means = (0.0, 127.5, 254.999)
    f = _frames(1, 45, 83, 5)
    _same(ctx.frame_u8(f, means, **_geometry(45, 83, 48, 96)), _host(f, 48, 96, means=means), "other means")


# ---- model level ------------------------------------------------------------------------------------------------------------------
def _input_model(ctx, H, W):
    """a model with the image inputs `data` / `data_key` of one H x W frame (the one-op plan of accel_flow_input; never run here)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    ib, h2, w2 = 3 * H * W * 4, H // 2, W // 2
    arena = (h2 * w2 * 32 + 255) // 256 * 256
    m.add_plan("op", "option graph=0 tune=0\narena bytes=%d\npbuf name=data bytes=%d\npbuf name=data_key bytes=%d\npbuf name=y bytes=%d\n"
                     "prep_flow cur=data:0:3:4:%d:%d prev=data_key:0:3:4:%d:%d dst=A:0:6:8:%d:%d H=%d W=%d\n"
                     "export_nchw src=A:0:6:8:%d:%d dst=y:0:6:8:%d:%d\n"
               % (arena, ib, ib, 6 * h2 * w2 * 4, H, W, H, W, h2, w2, H, W, h2, w2, h2, w2))
    return m


@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (45, 83, 48, 96), (100, 75, 48, 96)])
def test_model_write_u8_prefetch_commit_and_device_source(ctx, rows, cols, target, max_size):
    import torch
    from accel_amd import runtime
    g = _geometry(rows, cols, target, max_size)
    H, W = g["H"], g["W"]
    fa, fb, fc = (_frames(1, rows, cols, 300 + i) for i in range(3))
    ha, hb, hc = (_host(f, target, max_size) for f in (fa, fb, fc))
    m = _input_model(ctx, H, W)
    pin = runtime.PinnedBuffer(fb.shape, np.uint8)
    pin32 = runtime.PinnedBuffer(hc.shape, np.float32)
    try:
        m.write_u8("data", fa, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), ha, "write_u8")
        gen = m.generation("data")
        # an accel_model_write after a write_u8 replaces the content, and the other way round
        m.write("data", hb)
        _same(m.read("data", (1, 3, H, W)), hb, "write after write_u8")
        m.write_u8("data", fc, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), hc, "write_u8 after write")
        assert m.generation("data") == gen + 2
        # the overlapped upload: uint8 bytes on the copy stream into a uint8 shadow, converted at commit
        pin.array[...] = fb
        m.prefetch_u8("data", pin)
        m.commit_u8("data", 1, rows, cols, 3 * cols, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), hb, "prefetch_u8 + commit_u8")
        pin.array[...] = fa                          # a second round through the same shadow (waits for the first kernel)
        m.prefetch_u8("data", pin)
        m.commit_u8("data", 1, rows, cols, 3 * cols, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), ha, "second prefetch_u8 + commit_u8")
        with pytest.raises(runtime.AccelError, match="no uint8 frames were prefetched"):
            m.commit_u8("data", 1, rows, cols, 3 * cols, MEANS, **g)
        # the fp32 shadow and the uint8 shadow of one buffer are two things: each commit takes its own
        pin32.array[...] = hc
        m.prefetch("data", pin32)
        with pytest.raises(runtime.AccelError, match="no uint8 frames were prefetched"):
            m.commit_u8("data", 1, rows, cols, 3 * cols, MEANS, **g)
        pin.array[...] = fb
        m.prefetch_u8("data", pin)
        m.commit("data")
        _same(m.read("data", (1, 3, H, W)), hc, "fp32 commit beside a uint8 prefetch")
        m.commit_u8("data", 1, rows, cols, 3 * cols, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), hb, "uint8 commit after the fp32 one")
        with pytest.raises(runtime.AccelError, match="nothing was prefetched"):
            m.commit("data")
        # a device-resident source (a frame a GPU decoder left in HBM) is read in place, into the other input
        dev = torch.from_numpy(fc).cuda()
        torch.cuda.synchronize()                     # torch's stream and the library's compute stream are not ordered by themselves
        m.write_u8_device("data_key", dev.data_ptr(), 1, rows, cols, 3 * cols, MEANS, **g)
        _same(m.read("data_key", (1, 3, H, W)), hc, "device source")
        _same(m.read("data", (1, 3, H, W)), hb, "the other input is untouched")
        del dev
    finally:
        ctx.sync()
        pin.close()
        pin32.close()
        m.close()


def test_argument_errors_return_err_arg(ctx):
    """every geometry the kernel could not honour is refused before anything is enqueued, with a message that names the argument"""
    from accel_amd import runtime
    lib = runtime.lib()
    rows, cols = 45, 83
    g = _geometry(rows, cols, 48, 96)
    H, W = g["H"], g["W"]
    f = _frames(1, rows, cols, 9)
    want = _host(f, 48, 96)
    means = (ctypes.c_double * 3)(*MEANS)
    src = f.ctypes.data_as(ctypes.c_void_p)
    out = np.empty((1, 3, H, W), np.float32)
    good = dict(n=1, h=rows, w=cols, pitch=3 * cols, out_h=g["out_h"], out_w=g["out_w"], step=g["step"], H=H, W=W)
    cases = [(dict(out_h=H + 1), "out_h"), (dict(out_w=W + 1), "out_w"), (dict(h=0), "h ="), (dict(w=0), "w ="), (dict(h=-3), "h ="),
             (dict(pitch=3 * cols - 1), "pitch"), (dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=float("nan")), "step"),
             (dict(n=0), "n ="), (dict(step=1.0), "step")]
    m = _input_model(ctx, H, W)
    pin = runtime.PinnedBuffer(f.shape, np.uint8)
    try:
        m.write_u8("data", f, MEANS, **g)

        def op(a):
            return lib.accel_frame_u8(ctx.handle, src, a["n"], a["h"], a["w"], a["pitch"], means, a["out_h"], a["out_w"], a["step"], a["H"], a["W"],
                                      out.ctypes.data_as(ctypes.c_void_p))

        def write(a, buf=b"data"):
            return lib.accel_model_write_u8(m.handle, buf, src, a["n"], a["h"], a["w"], a["pitch"], means, a["out_h"], a["out_w"], a["step"],
                                            a["H"], a["W"], 0)

        def commit(a, buf=b"data"):
            return lib.accel_model_commit_u8(m.handle, buf, a["n"], a["h"], a["w"], a["pitch"], means, a["out_h"], a["out_w"], a["step"], a["H"], a["W"])

        pin.array[...] = f
        m.prefetch_u8("data", pin)
        for change, word in cases:
            for call in (op, write, commit):
                rc = call(dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (call.__name__, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg, (call.__name__, change, msg)
        # n * 3 * H * W * 4 must be the size of the buffer: another batch, another padded size
        for change in (dict(n=2), dict(H=H + 16), dict(W=W - 16, out_w=W - 16, w=W - 16, pitch=3 * (W - 16), step=1.0, out_h=rows)):
            for call in (write, commit):
                rc = call(dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1 and "buffer 'data' has" in msg, (call.__name__, change, rc, msg)
        for call in (write, commit):
            rc = call(good, b"no_such_buffer")
            assert rc == -1 and "unknown buffer 'no_such_buffer'" in lib.accel_last_error().decode()
        assert lib.accel_model_prefetch_u8(m.handle, b"no_such_buffer", pin.ptr, pin.nbytes) == -1
        assert "unknown buffer" in lib.accel_last_error().decode()
        rc = commit(dict(good, n=1, h=rows + 1, out_h=g["out_h"]))       # more bytes than were prefetched
        assert rc == -1 and "were prefetched" in lib.accel_last_error().decode()
        # none of the refused calls touched the buffer or consumed the prefetch
        _same(m.read("data", (1, 3, H, W)), want, "after the refused calls")
        assert commit(good) == 0
        _same(m.read("data", (1, 3, H, W)), want, "commit after the refused calls")
    finally:
        ctx.sync()
        pin.close()
        m.close()


# ---- whole path ---------------------------------------------------------------------------------------------------------------------
def _run(runner, batches, interval, prefetch=False):
    outs = []
    for i, arrays in enumerate(batches):
        lg, lab = runner.step(i, arrays, interval)
        if prefetch and i + 1 < len(batches):
            assert runner.prefetch(batches[i + 1])
        outs.append((lg.asnumpy().copy(), lab.asnumpy().copy()))
    return outs


def _identical(got, ref, what):
    assert len(got) == len(ref)
    for t, ((lg, lab), (rlg, rlab)) in enumerate(zip(got, ref)):
        assert np.array_equal(lg, rlg), "%s, frame %d: logits differ by %g" % (what, t, float(np.abs(lg - rlg).max()))
        assert np.array_equal(lab, rlab), "%s, frame %d: labels differ" % (what, t)


@pytest.mark.parametrize("rows,cols,stride", [(128, 256, 0),        # scale 1: the bytes themselves
                                              (120, 250, 16)])      # scale 1.024: a 123 x 256 interior padded to 128 x 256
def test_raw_frames_give_the_logits_of_fp32_frames(demo_cfg, rows, cols, stride):
    """Accel-18, 5 frames, interval 3: the plans are the same and a run is a pure function of its inputs (test_stateless_gpu.py), so raw uint8
    frames must give BIT-IDENTICAL logits and labels -- through the plain loop and through the pinned prefetch loop."""
    from accel_amd import demo, mx
    from accel_amd.core import tester
    H, W = 128, 256
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = stride
    g = image.resize_geometry(rows, cols, H, W, stride)
    assert g[3:] == (H, W) and (rows != 120 or g == (1.024, 123, 256, 128, 256))
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    frames = synth.make_clip(rows, cols, 5)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        ref = _run(r, demo.build_batches(frames, demo_cfg), 3)
        assert not np.array_equal(ref[0][0], ref[1][0])
        raw = demo.build_batches(frames, demo_cfg, raw=True)
        assert isinstance(raw[0][0], mx.nd.RawFrames) and raw[0][0].shape == (1, 3, H, W)
        _identical(_run(r, raw, 3), ref, "raw frames, plain loop")
        assert raw[0][0]._host is None, "the uint8 route must not build the fp32 image on the host"
        pinned = demo.build_batches(frames, demo_cfg, pinned=True, raw=True)
        assert pinned[0][0].pinned is not None and pinned[0][0].pinned.dtype == np.uint8
        _identical(_run(r, pinned, 3, prefetch=True), ref, "raw frames, pinned prefetch loop")
        assert pinned[1][0]._host is None
        # a prefetched frame that is NOT the one fed next must not be used
        r.step(0, pinned[0], 3)
        assert r.prefetch(pinned[3])
        lg = r.step(1, pinned[1], 3)[0].asnumpy()
        assert np.array_equal(lg, ref[1][0])
        # fp32 and raw arrays may alternate on one runner: each route replaces what the other left in the inputs
        mixed = demo.build_batches(frames, demo_cfg, pinned=True)
        r.step(0, mixed[0], 3)
        assert r.prefetch(pinned[1])
        assert np.array_equal(r.step(1, [pinned[1][0], mixed[0][0], pinned[1][2]], 3)[0].asnumpy(), ref[1][0])
        assert r.prefetch(mixed[2])
        assert np.array_equal(r.step(2, [mixed[2][0], pinned[1][0], mixed[2][2]], 3)[0].asnumpy(), ref[2][0])
        # a raw array given as data_key without being resident goes the uint8 route into data_key
        r.step(0, raw[0], 3)
        other = mx.nd.raw_frames(frames[0], demo_cfg)
        assert np.array_equal(r.step(1, [raw[1][0], other, raw[1][2]], 3)[0].asnumpy(), ref[1][0])
        assert other._host is None
    finally:
        tester.release_models()


def test_raw_frames_at_batch_two(demo_cfg):
    from accel_amd import demo, mx
    from accel_amd.core import tester
    H, W, rows, cols = 128, 256, 120, 250
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = 16
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    clips = [synth.make_clip(rows, cols, 3, seed=s) for s in (11, 12)]
    zero = mx.nd.array(np.zeros((2, 2048, 1, 1), np.float32))
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W), batch=2)
        plain, raw = [], []
        for t in range(3):
            pair = np.stack([clips[0][t], clips[1][t]])
            plain.append(mx.nd.array(_host(pair, H, W, 16, demo_cfg.network.PIXEL_MEANS)))
            raw.append(mx.nd.raw_frames(pair, demo_cfg, ctx=mx.cpu_pinned()))
            assert raw[-1].shape == plain[-1].shape == (2, 3, H, W)
        ref = _run(r, [[plain[t], plain[t - 1] if t else plain[0], zero] for t in range(3)], 3)
        assert ref[0][0].shape == (2, 19, H, W) and not np.array_equal(ref[0][0][0], ref[0][0][1])
        batches = [[raw[t], raw[t - 1] if t else raw[0], zero] for t in range(3)]
        _identical(_run(r, batches, 3), ref, "batch 2, plain loop")
        _identical(_run(r, batches, 3, prefetch=True), ref, "batch 2, prefetch loop")
    finally:
        tester.release_models()


def test_demo_runs_on_raw_frames(demo_cfg, capsys):
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "3", "--num_ex", "2", "--synthetic", "128x256", "--raw-frames"])
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    assert out.rstrip().endswith("done") and out.count("testing synthetic_") == 6, out[-1500:]
