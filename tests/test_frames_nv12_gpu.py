"""NV12 video frames on the GPU (csrc/frames_yuv.hip behind accel_frame_nv12 / accel_nv12_to_bgr / accel_model_write_nv12 / _commit_nv12): the
tensor the kernel writes is the one accel_amd/utils/image.py builds on the host -- transform(resize(nv12_to_bgr_host(frame))) as fp32 -- BIT FOR
BIT.  The colour conversion is integer arithmetic and what follows it is the float64 arithmetic of the uint8 route with one defined rounding, so
every comparison is np.array_equal: no tolerance.  Random frames draw luma and both chroma bytes independently, so a wrong chroma row, column or
byte order cannot cancel.  (Host side: test_frames_nv12_cpu.py.)"""
import ctypes

import numpy as np
import pytest

from accel_amd.utils import image, synth

from test_frames_nv12_cpu import _spread, _tight
from test_frames_u8_gpu import _geometry, _identical, _input_model, _run, _same

pytestmark = pytest.mark.gpu

MEANS = (103.06, 115.9, 123.15)
STRIDE = 16

# step 1 (rows, cols, stride): the dword form / portrait / the smallest frame, all padding but one patch / w % 4 == 2, the last patch of a row is half
# frame, half padding / W % 4 != 0, scalar stores with a tail
COPIES = [(48, 96, 16), (96, 48, 16), (2, 2, 16), (16, 18, 16), (30, 50, 0)]
# resampled (rows, cols, target, max): up with padded columns / up with padded rows / down by 0.8 / portrait down / down to a 14-row image
RESAMPLED = [(44, 82, 48, 96), (36, 90, 64, 128), (60, 120, 48, 96), (100, 74, 48, 96), (22, 150, 48, 96)]


def _host(buf, rows, cols, target, max_size, stride=STRIDE, means=MEANS, colour=0, **layout):
    bgr = image.nv12_to_bgr_host(buf, rows, cols, colour=colour, **layout)
    return np.concatenate([image.transform(image.resize(f, target, max_size, stride=stride)[0], means) for f in bgr]).astype(np.float32)


# ---- operator level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", [0, 3])
@pytest.mark.parametrize("rows,cols,stride", COPIES)
def test_frame_nv12_copies_at_step_one(ctx, rows, cols, stride, colour):
    buf = _tight(1, rows, cols, rows * 4096 + cols)
    target, max_size = min(rows, cols), max(rows, cols)
    g = _geometry(rows, cols, target, max_size, stride)
    assert g["step"] == 1.0 and (g["out_h"], g["out_w"]) == (rows, cols)
    _same(ctx.frame_nv12(buf, rows, cols, MEANS, colour=colour, **g), _host(buf, rows, cols, target, max_size, stride, colour=colour), (rows, cols, stride, g))


@pytest.mark.parametrize("colour", [1, 2])
@pytest.mark.parametrize("rows,cols,target,max_size", RESAMPLED)
def test_frame_nv12_resampled(ctx, rows, cols, target, max_size, colour):
    buf = _tight(1, rows, cols, rows * 4096 + cols)
    g = _geometry(rows, cols, target, max_size)
    assert g["step"] != 1.0
    _same(ctx.frame_nv12(buf, rows, cols, MEANS, colour=colour, **g), _host(buf, rows, cols, target, max_size, colour=colour), (rows, cols, target, max_size, g))


@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (16, 18, 16, 18), (44, 82, 48, 96)])
def test_frame_nv12_batch_of_three(ctx, rows, cols, target, max_size):
    buf = _tight(3, rows, cols, 77 + rows)
    got = ctx.frame_nv12(buf, rows, cols, MEANS, **_geometry(rows, cols, target, max_size))
    assert got.shape[0] == 3 and not np.array_equal(got[0], got[1])
    _same(got, _host(buf, rows, cols, target, max_size), "batch of 3")
    _same_bytes(ctx.nv12_to_bgr(buf, rows, cols), image.nv12_to_bgr_host(buf, rows, cols), "batch of 3, BGR")


def _same_bytes(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ from the host conversion, first at %s: %r != %r"
                             % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# pitch - w, bytes after a frame: the dword form (at w = 18 with 14) / odd pitch: byte loads / a tail of 5 bytes: the second frame is misaligned
@pytest.mark.parametrize("extra,tail", [(12, 0), (14, 0), (7, 0), (12, 5)])
@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (16, 18, 16, 18), (60, 120, 48, 96)])
def test_frame_nv12_pitch_plane_gap_and_frame_tail(ctx, rows, cols, target, max_size, extra, tail):
    tight = _tight(2, rows, cols, extra * 100 + tail)
    pitch = cols + extra
    uv_offset = pitch * (rows + 6)
    frame_bytes = uv_offset + (rows // 2) * pitch + tail
    spread = _spread(tight, rows, cols, pitch, uv_offset, frame_bytes, 5)       # the bytes in the gaps are not zero
    lay = dict(pitch=pitch, uv_offset=uv_offset, frame_bytes=frame_bytes)
    want = _host(tight, rows, cols, target, max_size, colour=2)
    _same(ctx.frame_nv12(spread, rows, cols, MEANS, colour=2, **lay, **_geometry(rows, cols, target, max_size)), want, lay)
    # the host buffer may end with the last frame's chroma plane
    short = spread.reshape(-1)[:spread.size - tail]
    if tail:
        from accel_amd import runtime
        out = np.empty_like(want)
        g = _geometry(rows, cols, target, max_size)
        runtime.check(runtime.lib().accel_frame_nv12(ctx.handle, short.ctypes.data_as(ctypes.c_void_p), 2, rows, cols, pitch, uv_offset, frame_bytes, 2,
                                                     (ctypes.c_double * 3)(*MEANS), g["out_h"], g["out_w"], g["step"], g["H"], g["W"],
                                                     out.ctypes.data_as(ctypes.c_void_p)))
        _same(out, want, "a buffer without the last tail")
    # the byte converter on the same layout, into tight rows and into pitched rows whose gaps stay as they were
    bgr = image.nv12_to_bgr_host(tight, rows, cols, colour=2)
    _same_bytes(ctx.nv12_to_bgr(spread, rows, cols, colour=2, **lay), bgr, lay)
    for out_pitch in (3 * cols + 4, 3 * cols + 5):
        before = np.random.default_rng(out_pitch).integers(0, 256, (2, rows, out_pitch), dtype=np.uint8)
        out = before.copy()
        assert ctx.nv12_to_bgr(spread, rows, cols, colour=2, out=out, **lay) is out
        _same_bytes(out[:, :, :3 * cols].reshape(bgr.shape), bgr, (lay, out_pitch))
        assert np.array_equal(out[:, :, 3 * cols:], before[:, :, 3 * cols:]), "bytes between the rows were written"


@pytest.mark.parametrize("level", [0, 255])
@pytest.mark.parametrize("colour", [0, 1, 2, 3])
@pytest.mark.parametrize("rows,cols,target,max_size", [(16, 18, 16, 18), (44, 82, 48, 96)])
def test_frame_nv12_constant_frames(ctx, level, colour, rows, cols, target, max_size):
    means = (0.0, 127.5, 254.999)
    buf = np.full((1, rows * cols * 3 // 2), level, np.uint8)
    g = _geometry(rows, cols, target, max_size)
    got = ctx.frame_nv12(buf, rows, cols, means, colour=colour, **g)
    _same(got, _host(buf, rows, cols, target, max_size, means=means, colour=colour), "constant %d" % level)
    bgr = [int(v) for v in image.yuv_to_bgr(level, level, level, colour)]
    for c in range(3):      # a resample of a constant frame is the constant; the padding is fp32(0 - mean), not 0
        assert np.all(got[0, 2 - c, :g["out_h"], :g["out_w"]] == np.float32(float(bgr[c]) - means[c]))
        assert np.all(got[0, 2 - c, g["out_h"]:, :] == np.float32(0.0 - means[c]))
        assert np.all(got[0, 2 - c, :, g["out_w"]:] == np.float32(0.0 - means[c]))


_EXHAUSTIVE = []


def _exhaustive_frame():
    """One 4096 x 4096 frame in which every (Y, Cb, Cr) triple occurs exactly once: chroma sample p = row * 2048 + column holds the pair
    (p & 255, (p >> 8) & 255), so every pair occurs 64 times (copy p >> 16), and the 4 luma bytes under copy k of a pair are 4k .. 4k + 3 plus an
    offset that depends on the pair, mod 256: a permutation of 0 .. 255 over the 64 copies."""
    if not _EXHAUSTIVE:
        side = 4096
        p = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
        cb, cr, k = p & 255, (p >> 8) & 255, p >> 16
        buf = np.empty(side * side * 3 // 2, np.uint8)
        luma = buf[:side * side].reshape(side, side)
        for dy in (0, 1):
            for dx in (0, 1):
                luma[dy::2, dx::2] = (4 * k + 2 * dy + dx + 37 * cb + 101 * cr) & 255
        buf[side * side:] = np.stack([cb, cr], axis=-1).astype(np.uint8).reshape(-1)
        up = lambda a: np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)
        triple = luma.astype(np.int64) << 16 | up(cb) << 8 | up(cr)
        assert np.array_equal(np.bincount(triple.reshape(-1), minlength=1 << 24), np.ones(1 << 24, np.int64))
        buf.setflags(write=False)
        _EXHAUSTIVE.append(buf)
    return _EXHAUSTIVE[0]


@pytest.mark.parametrize("colour", [0, 1, 2, 3])
def test_every_triple_through_both_kernels(ctx, colour):
    side = 4096
    buf = _exhaustive_frame()
    want = image.nv12_to_bgr_host(buf, side, side, colour=colour)           # the integer rule on every triple
    _same_bytes(ctx.nv12_to_bgr(buf, side, side, colour=colour), want, "nv12_to_bgr, colour %d" % colour)
    got = ctx.frame_nv12(buf, side, side, (0.0, 0.0, 0.0), side, side, 1.0, side, side, colour=colour)      # means 0: the fp32 values are the bytes
    assert got.shape == (1, 3, side, side) and got.dtype == np.float32
    for c in range(3):
        assert np.array_equal(got[0, 2 - c], want[0, :, :, c]), "frame_nv12, colour %d, channel %d" % (colour, c)


# ---- model level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (44, 82, 48, 96)])
def test_model_write_nv12_prefetch_commit_and_device_source(ctx, rows, cols, target, max_size):
    import torch
    from accel_amd import runtime
    g = _geometry(rows, cols, target, max_size)
    H, W = g["H"], g["W"]
    fb = rows * cols * 3 // 2
    lay = (rows, cols, cols, rows * cols, fb, 2)           # h, w, pitch, uv_offset, frame_bytes, colour
    fa, fb_, fc = (_tight(1, rows, cols, 300 + i) for i in range(3))
    ha, hb, hc = (_host(f, rows, cols, target, max_size, colour=2) for f in (fa, fb_, fc))
    m = _input_model(ctx, H, W)
    pin = runtime.PinnedBuffer(fa.shape, np.uint8)
    try:
        m.write_nv12("data", fa, rows, cols, MEANS, colour=2, **g)
        _same(m.read("data", (1, 3, H, W)), ha, "write_nv12")
        gen = m.generation("data")
        m.write("data", hb)
        m.write_nv12("data", fc, rows, cols, MEANS, colour=2, **g)
        _same(m.read("data", (1, 3, H, W)), hc, "write_nv12 after write")
        assert m.generation("data") == gen + 2
        # the overlapped upload: the bytes on the copy stream into the uint8 shadow, converted at commit
        with pytest.raises(runtime.AccelError, match="no uint8 frames were prefetched"):
            m.commit_nv12("data", 1, *lay, MEANS, **g)
        pin.array[...] = fb_
        m.prefetch_u8("data", pin)
        m.commit_nv12("data", 1, *lay, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), hb, "prefetch_u8 + commit_nv12")
        pin.array[...] = fa                          # a second round through the same shadow (waits for the first kernel)
        m.prefetch_u8("data", pin)
        m.commit_nv12("data", 1, *lay, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), ha, "second prefetch_u8 + commit_nv12")
        with pytest.raises(runtime.AccelError, match="no uint8 frames were prefetched"):
            m.commit_nv12("data", 1, *lay, MEANS, **g)
        # too few bytes prefetched: the shortfall is named, nothing is consumed
        m.prefetch_u8("data", pin)
        wide = (rows, cols, cols + 4, rows * (cols + 4), (rows + rows // 2) * (cols + 4), 2)      # the same frame at a pitch the bytes do not cover
        with pytest.raises(runtime.AccelError, match="%d bytes, %d were prefetched" % (wide[4], fb)):
            m.commit_nv12("data", 1, *wide, MEANS, **g)
        m.commit_nv12("data", 1, *lay, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), ha, "commit after the refused one")
        # a device-resident source (a frame a GPU decoder left in HBM), one byte off every alignment, read in place into the other input
        dev = torch.zeros(fc.size + 1, dtype=torch.uint8, device="cuda")
        dev[1:] = torch.from_numpy(fc.reshape(-1))
        torch.cuda.synchronize()                     # torch's stream and the library's compute stream are not ordered by themselves
        assert (dev.data_ptr() + 1) % 2 == 1
        m.write_nv12_device("data_key", dev.data_ptr() + 1, 1, *lay, MEANS, **g)
        _same(m.read("data_key", (1, 3, H, W)), hc, "device source")
        _same(m.read("data", (1, 3, H, W)), ha, "the other input is untouched")
        # and the byte converter from HBM into HBM
        out = torch.zeros((1, rows, cols, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.nv12_to_bgr_device(dev.data_ptr() + 1, out.data_ptr(), 1, rows, cols, cols, rows * cols, fb, 2, 3 * cols)
        ctx.sync()
        _same_bytes(out.cpu().numpy(), image.nv12_to_bgr_host(fc, rows, cols, colour=2), "nv12_to_bgr on the device")
        del dev, out
    finally:
        ctx.sync()
        pin.close()
        m.close()


def test_model_second_prefetch_of_another_size(ctx):
    """one model, one shadow: frames with more bytes than the shadow holds make it grow, smaller ones reuse it"""
    from accel_amd import runtime
    H, W = 48, 96
    m = _input_model(ctx, H, W)
    pins = []
    try:
        for rows, cols in ((44, 82), (60, 120), (36, 72)):
            g = _geometry(rows, cols, H, W)
            assert (g["H"], g["W"]) == (H, W)
            f = _tight(1, rows, cols, rows)
            pins.append(runtime.PinnedBuffer(f.shape, np.uint8))
            pins[-1].array[...] = f
            m.prefetch_u8("data", pins[-1])
            m.commit_nv12("data", 1, rows, cols, cols, rows * cols, f.shape[1], 0, MEANS, **g)
            _same(m.read("data", (1, 3, H, W)), _host(f, rows, cols, H, W), (rows, cols))
    finally:
        ctx.sync()
        for p in pins:
            p.close()
        m.close()


def test_argument_errors_return_err_arg(ctx):
    """every layout and geometry the kernels could not honour is refused before anything is enqueued, with a message that names the argument"""
    from accel_amd import runtime
    lib = runtime.lib()
    rows, cols = 44, 82
    g = _geometry(rows, cols, 48, 96)
    H, W = g["H"], g["W"]
    f = _tight(1, rows, cols, 9)
    want = _host(f, rows, cols, 48, 96)
    means = (ctypes.c_double * 3)(*MEANS)
    src = f.ctypes.data_as(ctypes.c_void_p)
    out = np.full((1, 3, H, W), 7.0, np.float32)
    bgr = np.full((1, rows, cols, 3), 7, np.uint8)
    fb = rows * cols * 3 // 2
    good = dict(n=1, h=rows, w=cols, pitch=cols, uv=rows * cols, fb=fb, colour=0, out_h=g["out_h"], out_w=g["out_w"], step=g["step"], H=H, W=W)
    layout = [(dict(h=rows + 1), "h ="), (dict(w=cols - 1), "w ="), (dict(h=0), "h ="), (dict(w=0), "w ="), (dict(h=-2), "h ="),
              (dict(h=32770), "h ="), (dict(w=32770), "w ="), (dict(pitch=cols - 1), "pitch"), (dict(uv=rows * cols - 1), "uv_offset"),
              (dict(fb=fb - 1), "frame_bytes"), (dict(pitch=cols + 1), "uv_offset"), (dict(pitch=cols + 1, uv=rows * (cols + 1)), "frame_bytes"),
              (dict(colour=-1), "colour"), (dict(colour=4), "colour"), (dict(n=0), "n =")]
    geometry = [(dict(out_h=H + 1), "out_h"), (dict(out_w=W + 1), "out_w"), (dict(out_h=0), "out_h"), (dict(step=0.0), "step"),
                (dict(step=-1.0), "step"), (dict(step=float("nan")), "step"), (dict(step=1.0), "step")]
    m = _input_model(ctx, H, W)
    pin = runtime.PinnedBuffer(f.shape, np.uint8)
    try:
        m.write_nv12("data", f, rows, cols, MEANS, **g)

        def lay(a):
            return a["n"], a["h"], a["w"], a["pitch"], a["uv"], a["fb"], a["colour"]

        def res(a):
            return a["out_h"], a["out_w"], a["step"], a["H"], a["W"]

        def op(a):
            return lib.accel_frame_nv12(ctx.handle, src, *lay(a), means, *res(a), out.ctypes.data_as(ctypes.c_void_p))

        def to_bgr(a):
            return lib.accel_nv12_to_bgr(ctx.handle, src, *lay(a), bgr.ctypes.data_as(ctypes.c_void_p), 3 * cols, 0)

        def write(a, buf=b"data"):
            return lib.accel_model_write_nv12(m.handle, buf, src, *lay(a), means, *res(a), 0)

        def commit(a, buf=b"data"):
            return lib.accel_model_commit_nv12(m.handle, buf, *lay(a), means, *res(a))

        pin.array[...] = f
        m.prefetch_u8("data", pin)
        for cases, calls in ((layout, (op, to_bgr, write, commit)), (geometry, (op, write, commit))):
            for change, word in cases:
                for call in calls:
                    rc = call(dict(good, **change))
                    msg = lib.accel_last_error().decode()
                    assert rc == -1, (call.__name__, change, rc, msg)       # ACCEL_ERR_ARG
                    assert word in msg, (call.__name__, change, msg)
        assert lib.accel_nv12_to_bgr(ctx.handle, src, *lay(good), bgr.ctypes.data_as(ctypes.c_void_p), 3 * cols - 1, 0) == -1
        assert "out_pitch" in lib.accel_last_error().decode()
        assert lib.accel_frame_nv12(ctx.handle, None, *lay(good), means, *res(good), out.ctypes.data_as(ctypes.c_void_p)) == -1
        assert "nv12" in lib.accel_last_error().decode()
        # n * 3 * H * W * 4 must be the size of the buffer
        for change in (dict(n=2), dict(H=H + 16)):
            for call in (write, commit):
                rc = call(dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1 and "buffer 'data' has" in msg, (call.__name__, change, rc, msg)
        for call in (write, commit):
            rc = call(good, b"no_such_buffer")
            assert rc == -1 and "unknown buffer 'no_such_buffer'" in lib.accel_last_error().decode()
        # a layout that needs more bytes than were prefetched
        rc = commit(dict(good, pitch=cols + 2, uv=rows * (cols + 2), fb=(rows + rows // 2) * (cols + 2)))
        assert rc == -1 and "were prefetched" in lib.accel_last_error().decode()
        # none of the refused calls touched a target or consumed the prefetch
        assert np.all(out == 7.0) and np.all(bgr == 7)
        _same(m.read("data", (1, 3, H, W)), want, "after the refused calls")
        assert commit(good) == 0
        _same(m.read("data", (1, 3, H, W)), want, "commit after the refused calls")
    finally:
        ctx.sync()
        pin.close()
        m.close()


# ---- whole path ---------------------------------------------------------------------------------------------------------------------
def _nv12_batches(clip_nv12, rows, cols, cfg, colour, ctx=None):
    from accel_amd import mx
    zero = mx.nd.array(np.zeros((1, cfg.network.DFF_FEAT_DIM, 1, 1)))
    arrs = [mx.nd.nv12_frames(b, rows, cols, cfg, colour=colour, ctx=ctx) for b in clip_nv12]
    return [[arrs[t], arrs[t - 1] if t else arrs[0], zero] for t in range(len(arrs))]


@pytest.mark.parametrize("rows,cols,stride", [(128, 256, 0),        # scale 1: the converted bytes themselves
                                              (120, 250, 16)])      # scale 1.024: a 123 x 256 interior padded to 128 x 256, resampled
def test_nv12_frames_give_the_logits_of_their_bgr_frames(demo_cfg, rows, cols, stride):
    """Accel-18, 4 frames, interval 3 (key and non-key frames): the input tensor is the same and a run is a pure function of its inputs, so NV12
    frames must give BIT-IDENTICAL logits and labels to raw BGR frames of their host conversion -- through the plain loop and the pinned
    prefetch loop -- and the finishing calls take an NV12 array as `like`."""
    from accel_amd import demo, mx
    from accel_amd.core import results, tester
    from test_results_gpu import PALETTE
    H, W = 128, 256
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = stride
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    nv = [image.bgr_to_nv12_host(f, 2) for f in synth.make_clip(rows, cols, 4)]
    bgr = [image.nv12_to_bgr_host(b, rows, cols, colour=2)[0] for b in nv]
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        ref = _run(r, demo.build_batches(bgr, demo_cfg, raw=True), 3)
        assert not np.array_equal(ref[0][0], ref[1][0])
        plain = _nv12_batches(nv, rows, cols, demo_cfg, "bt709")
        assert isinstance(plain[0][0], mx.nd.NV12Frames) and plain[0][0].shape == (1, 3, H, W)
        _identical(_run(r, plain, 3), ref, "NV12 frames, plain loop")
        assert plain[0][0]._host is None and plain[0][0]._frames is None, "the NV12 route must not convert anything on the host"
        pinned = _nv12_batches(nv, rows, cols, demo_cfg, "bt709", ctx=mx.cpu_pinned())
        assert pinned[0][0].pinned is not None and pinned[0][0].pinned.dtype == np.uint8
        _identical(_run(r, pinned, 3, prefetch=True), ref, "NV12 frames, pinned prefetch loop")
        assert pinned[1][0]._host is None and pinned[1][0]._frames is None
        # NV12 and BGR arrays may alternate on one runner
        raw = demo.build_batches(bgr, demo_cfg, pinned=True, raw=True)
        r.step(0, raw[0], 3)
        assert r.prefetch(pinned[1])
        assert np.array_equal(r.step(1, [pinned[1][0], raw[0][0], pinned[1][2]], 3)[0].asnumpy(), ref[1][0])
        # finishing with an NV12 array as `like`
        lg, lab = r.step(0, plain[0], 3)
        like = plain[0][0]
        out_h, out_w = like.geometry["out_h"], like.geometry["out_w"]
        want_src = image.labels_to_source_host(lab.asnumpy(), out_h, out_w, rows, cols)
        assert np.array_equal(results.labels_at_source(lab, like), want_src)
        assert np.array_equal(results.colour(lab, like, PALETTE, frames=True, alpha=128),
                              image.colour_host(want_src, PALETTE, frames=bgr[0][None], alpha=128))
        conf = results.confidence(lg, like)
        assert np.array_equal(conf, image.confidence_host(lg.asnumpy(), out_h, out_w, rows, cols)[0])
    finally:
        tester.release_models()


def test_nv12_frames_at_batch_two(demo_cfg):
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
        raw, nv = [], []
        for t in range(3):
            pair = image.bgr_to_nv12_host(np.stack([clips[0][t], clips[1][t]]), 0)
            raw.append(mx.nd.raw_frames(image.nv12_to_bgr_host(pair, rows, cols), demo_cfg))
            nv.append(mx.nd.nv12_frames(pair, rows, cols, demo_cfg, ctx=mx.cpu_pinned()))
            assert nv[-1].shape == raw[-1].shape == (2, 3, H, W)
        ref = _run(r, [[raw[t], raw[t - 1] if t else raw[0], zero] for t in range(3)], 3)
        assert ref[0][0].shape == (2, 19, H, W) and not np.array_equal(ref[0][0][0], ref[0][0][1])
        batches = [[nv[t], nv[t - 1] if t else nv[0], zero] for t in range(3)]
        _identical(_run(r, batches, 3), ref, "batch 2, plain loop")
        _identical(_run(r, batches, 3, prefetch=True), ref, "batch 2, prefetch loop")
    finally:
        tester.release_models()


def test_demo_runs_on_nv12_frames(demo_cfg, capsys):
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "3", "--num_ex", "2", "--synthetic", "128x256", "--nv12", "bt709", "--finish-on-gpu"])
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    assert out.rstrip().endswith("done") and out.count("testing synthetic_") == 6, out[-1500:]
