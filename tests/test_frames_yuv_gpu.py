"""I420, P010 and YUY2 video frames on the GPU (csrc/frames_yuv.hip behind accel_frame_yuv / accel_yuv_to_bgr / accel_model_write_yuv / _commit_yuv):
the tensor the kernel writes is the one accel_amd/utils/image.py builds on the host -- transform(resize(yuv_to_bgr_host(frame))) as fp32 -- BIT FOR
BIT.  The colour conversion is integer arithmetic and what follows it is the float64 arithmetic of the uint8 route with one defined rounding, so
every comparison is np.array_equal: no tolerance.  Random frames draw luma and both chroma components independently (all 16 bits of a P010 word,
so its low six are noise), and the bytes in every gap are non-zero noise.  (Host side, and why these cases can tell a wrong reader from a right
one: test_frames_yuv_cpu.py.)"""
import ctypes

import numpy as np
import pytest

from accel_amd.utils import image, synth

from test_frames_yuv_cpu import (FORMATS, MEANS, RESAMPLED, _copies, _host, _i420_of_nv12, _keywords, _p010_of_nv12, _spread, _tight, _tight_bytes,
                                 _yuy2_of_nv12)
from test_frames_nv12_gpu import _same_bytes
from test_frames_u8_gpu import _geometry, _identical, _input_model, _run, _same

pytestmark = pytest.mark.gpu

STEP_ONE = [(fmt,) + case for fmt in FORMATS for case in _copies(fmt)]


# ---- operator level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", [0, 3])
@pytest.mark.parametrize("fmt,rows,cols,stride", STEP_ONE)
def test_frame_yuv_copies_at_step_one(ctx, fmt, rows, cols, stride, colour):
    buf = _tight(fmt, 1, rows, cols, rows * 4096 + cols)
    target, max_size = min(rows, cols), max(rows, cols)
    g = _geometry(rows, cols, target, max_size, stride)
    assert g["step"] == 1.0 and (g["out_h"], g["out_w"]) == (rows, cols)
    _same(ctx.frame_yuv(buf, fmt, rows, cols, MEANS, colour=colour, **g), _host(buf, fmt, rows, cols, target, max_size, stride, colour=colour),
          (fmt, rows, cols, stride, g))
    _same_bytes(ctx.yuv_to_bgr(buf, fmt, rows, cols, colour=colour), image.yuv_to_bgr_host(buf, fmt, rows, cols, colour=colour), (fmt, rows, cols))


@pytest.mark.parametrize("colour", [1, 2])
@pytest.mark.parametrize("rows,cols,target,max_size", RESAMPLED)
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_yuv_resampled(ctx, fmt, rows, cols, target, max_size, colour):
    buf = _tight(fmt, 1, rows, cols, rows * 4096 + cols)
    g = _geometry(rows, cols, target, max_size)
    assert g["step"] != 1.0
    _same(ctx.frame_yuv(buf, fmt, rows, cols, MEANS, colour=colour, **g), _host(buf, fmt, rows, cols, target, max_size, colour=colour),
          (fmt, rows, cols, target, max_size, g))


@pytest.mark.parametrize("rows,cols,target,max_size", [(16, 18, 16, 18), (44, 82, 48, 96)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_yuv_batch_of_three(ctx, fmt, rows, cols, target, max_size):
    buf = _tight(fmt, 3, rows, cols, 77 + rows)
    got = ctx.frame_yuv(buf, fmt, rows, cols, MEANS, **_geometry(rows, cols, target, max_size))
    assert got.shape[0] == 3 and not np.array_equal(got[0], got[1])
    _same(got, _host(buf, fmt, rows, cols, target, max_size), "batch of 3")
    _same_bytes(ctx.yuv_to_bgr(buf, fmt, rows, cols), image.yuv_to_bgr_host(buf, fmt, rows, cols), "batch of 3, BGR")


def _up(v, k):
    return -(-v // k) * k


def _layout_case(fmt, name, rows, cols):
    """the layout keywords of a named case, and the bytes after each frame"""
    if fmt == "i420":
        pitch = _up(cols + 9, 4)                     # a multiple of 4: dword loads, also at w = 18 where the last patch of a row is cut
        if name == "pitch_c":                        # pitch_c other than pitch / 2
            return dict(pitch=pitch, pitch_c=pitch // 2 + 2), 0
        if name == "odd_pitch_c":                    # forces byte loads
            return dict(pitch=pitch, pitch_c=(cols // 2 + 6) | 1), 0
        if name == "yv12":                           # Cr before Cb
            return dict(v_offset=rows * cols, u_offset=rows * cols + rows * cols // 4), 0
        if name == "interleaved":                    # every row of the chroma area holds a Cb row, then a Cr row
            return dict(pitch=pitch, pitch_c=pitch, u_offset=rows * pitch, v_offset=rows * pitch + pitch // 2), 0
        if name == "gap":
            return dict(pitch=pitch, pitch_c=pitch // 2, u_offset=(rows + 6) * pitch, v_offset=(rows + 6) * pitch + (rows // 2) * (pitch // 2) + 10), 0
        if name == "tail":                           # the second frame is misaligned
            return dict(pitch=pitch, pitch_c=pitch // 2), 5
    if fmt == "yuy2":
        if name == "odd_pitch":
            return dict(pitch=2 * cols + 7), 0
        if name == "tail":
            return dict(pitch=2 * cols + 12), 5
    if fmt == "p010":
        if name == "pitch_plus_2":                   # breaks the 8-byte alignment, keeps the 2-byte one
            return dict(pitch=2 * cols + 2), 0
        if name == "gap":                            # a multiple of 8: 8-byte loads, also at w = 18
            return dict(pitch=_up(2 * cols + 2, 8), u_offset=_up(2 * cols + 2, 8) * (rows + 3)), 0
        if name == "tail":
            return dict(pitch=_up(2 * cols + 2, 8)), 6
    raise KeyError((fmt, name))


LAYOUTS = [("i420", n) for n in ("pitch_c", "odd_pitch_c", "yv12", "interleaved", "gap", "tail")] + [("yuy2", "odd_pitch"), ("yuy2", "tail")] \
    + [("p010", n) for n in ("pitch_plus_2", "gap", "tail")]


@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (16, 18, 16, 18), (60, 120, 48, 96)])
@pytest.mark.parametrize("fmt,name", LAYOUTS)
def test_frame_yuv_layouts(ctx, fmt, name, rows, cols, target, max_size):
    tight = _tight(fmt, 2, rows, cols, len(name) * 100 + rows)
    keywords, tail = _layout_case(fmt, name, rows, cols)
    lay = image.yuv_layout(fmt, rows, cols, **keywords)
    if tail:
        keywords["frame_bytes"] = lay["frame_bytes"] + tail
    # (with a tail the buffer ends with the last byte of the last frame)
    spread, lay = _spread(fmt, tight, rows, cols, 5, tail=tail, **keywords)
    kw = _keywords(lay)
    assert not tail or spread.size == lay["frame_bytes"] + image.yuv_extent(lay)
    want = _host(tight, fmt, rows, cols, target, max_size, colour=2)
    _same(ctx.frame_yuv(spread, fmt, rows, cols, MEANS, colour=2, **kw, **_geometry(rows, cols, target, max_size)), want, (fmt, name, lay))
    # the byte converter on the same layout, into tight rows and into pitched rows whose gaps stay as they were
    bgr = image.yuv_to_bgr_host(tight, fmt, rows, cols, colour=2)
    _same_bytes(ctx.yuv_to_bgr(spread, fmt, rows, cols, colour=2, **kw), bgr, (fmt, name, lay))
    for out_pitch in (3 * cols + 4, 3 * cols + 5):
        before = np.random.default_rng(out_pitch).integers(0, 256, (2, rows, out_pitch), dtype=np.uint8)
        out = before.copy()
        assert ctx.yuv_to_bgr(spread, fmt, rows, cols, colour=2, out=out, **kw) is out
        _same_bytes(out[:, :, :3 * cols].reshape(bgr.shape), bgr, (fmt, name, out_pitch))
        assert np.array_equal(out[:, :, 3 * cols:], before[:, :, 3 * cols:]), "bytes between the rows were written"


@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (16, 18, 16, 18), (44, 82, 48, 96)])
def test_formats_agree_with_the_nv12_kernels(ctx, rows, cols, target, max_size):
    """the same picture in four layouts: bit for bit one tensor and one BGR frame, from two kernel files"""
    nv = np.random.default_rng(rows + cols).integers(0, 256, (2, rows * cols * 3 // 2), dtype=np.uint8)
    g = _geometry(rows, cols, target, max_size)
    for colour in range(4):
        want = ctx.frame_nv12(nv, rows, cols, MEANS, colour=colour, **g)
        bgr = ctx.nv12_to_bgr(nv, rows, cols, colour=colour)
        cases = [("i420", _i420_of_nv12(nv, rows, cols)), ("yuy2", _yuy2_of_nv12(nv, rows, cols))]
        if colour in (0, 2):       # limited range: the 10-bit signal is 4 times the 8-bit one
            cases.append(("p010", _p010_of_nv12(nv, low=colour + 1)))
        for fmt, buf in cases:
            _same(ctx.frame_yuv(buf, fmt, rows, cols, MEANS, colour=colour, **g), want, (fmt, colour))
            _same_bytes(ctx.yuv_to_bgr(buf, fmt, rows, cols, colour=colour), bgr, (fmt, colour))


_COVER = []


def _p010_cover():
    """One 2048 x 2048 P010 frame, as (bytes, Y10, Cb10, Cr10 at full size): chroma sample p = row * 1024 + column holds the pair (p & 1023, p >> 10),
    so every pair occurs once; the four luma samples under it are (Cb + Cr + t) & 1023 for t in (0, 1, 2, 1023): under one Cb value Cr runs over
    all 1024 values, and so does the luma, and likewise under one Cr value; t = 0, 1, 2 and 1023 put luma 0 and 1023 under each corner of the
    chroma square.  The low six bits of every word are noise."""
    if not _COVER:
        side = 2048
        p = np.arange(1024 * 1024, dtype=np.int64).reshape(1024, 1024)
        cb, cr = p & 1023, p >> 10
        luma = np.empty((side, side), np.int64)
        for j, t in enumerate((0, 1, 2, 1023)):
            luma[j >> 1::2, j & 1::2] = (cb + cr + t) & 1023
        up = lambda a: np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)
        ucb, ucr = up(cb), up(cr)
        assert np.array_equal(np.bincount((cb << 10 | cr).reshape(-1), minlength=1 << 20), np.ones(1 << 20, np.int64))      # every (Cb, Cr) pair
        assert np.all(np.bincount((luma << 10 | ucb).reshape(-1), minlength=1 << 20) > 0)                                     # every luma under every Cb
        assert np.all(np.bincount((luma << 10 | ucr).reshape(-1), minlength=1 << 20) > 0)                                     # ... and under every Cr
        for y in (0, 1023):                           # all eight corners of the cube
            for b in (0, 1023):
                for r in (0, 1023):
                    assert np.any((luma == y) & (ucb == b) & (ucr == r)), ("corner", y, b, r)
        words = np.concatenate([luma.reshape(-1), np.stack([cb, cr], axis=-1).reshape(-1)]).astype("<u2") << 6
        words |= np.random.default_rng(10).integers(0, 64, words.shape).astype("<u2")
        buf = words.view(np.uint8)
        buf.setflags(write=False)
        _COVER.append((buf, luma, ucb, ucr))
    return _COVER[0]


@pytest.mark.parametrize("colour", [0, 1, 2, 3])
def test_p010_range_cover_through_both_kernels(ctx, colour):
    side = 2048
    buf, luma, cb, cr = _p010_cover()
    want = np.stack(image.yuv10_to_bgr(luma, cb, cr, colour), axis=-1)[None]           # the integer rule on the samples themselves
    _same_bytes(ctx.yuv_to_bgr(buf, "p010", side, side, colour=colour), want, "yuv_to_bgr, colour %d" % colour)
    got = ctx.frame_yuv(buf, "p010", side, side, (0.0, 0.0, 0.0), side, side, 1.0, side, side, colour=colour)      # means 0: the fp32 values are the bytes
    assert got.shape == (1, 3, side, side) and got.dtype == np.float32
    for c in range(3):
        assert np.array_equal(got[0, 2 - c], want[0, :, :, c]), "frame_yuv, colour %d, channel %d" % (colour, c)


@pytest.mark.parametrize("level", [0, 255])
@pytest.mark.parametrize("colour", [0, 1, 2, 3])
@pytest.mark.parametrize("rows,cols,target,max_size", [(16, 18, 16, 18), (44, 82, 48, 96)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_yuv_constant_frames(ctx, fmt, level, colour, rows, cols, target, max_size):
    """every byte 0 or 255: the 8-bit samples are 0 or 255, P010's 0 or 1023"""
    means = (0.0, 127.5, 254.999)
    buf = np.full((1, _tight_bytes(fmt, rows, cols)), level, np.uint8)
    g = _geometry(rows, cols, target, max_size)
    got = ctx.frame_yuv(buf, fmt, rows, cols, means, colour=colour, **g)
    _same(got, _host(buf, fmt, rows, cols, target, max_size, means=means, colour=colour), "constant %d" % level)
    if fmt == "p010":
        bgr = [int(v) for v in image.yuv10_to_bgr(level * 1023 // 255, level * 1023 // 255, level * 1023 // 255, colour)]
    else:
        bgr = [int(v) for v in image.yuv_to_bgr(level, level, level, colour)]
    for c in range(3):      # a resample of a constant frame is the constant; the padding is fp32(0 - mean), not 0
        assert np.all(got[0, 2 - c, :g["out_h"], :g["out_w"]] == np.float32(float(bgr[c]) - means[c]))
        assert np.all(got[0, 2 - c, g["out_h"]:, :] == np.float32(0.0 - means[c]))
        assert np.all(got[0, 2 - c, :, g["out_w"]:] == np.float32(0.0 - means[c]))


# ---- model level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_model_write_yuv_prefetch_commit_and_device_source(ctx, fmt):
    import torch
    from accel_amd import runtime
    rows, cols, target, max_size = 44, 82, 48, 96
    g = _geometry(rows, cols, target, max_size)
    H, W = g["H"], g["W"]
    lay = dict(image.yuv_layout(fmt, rows, cols), colour=2)
    fb = lay["frame_bytes"]
    fa, fb_, fc = (_tight(fmt, 1, rows, cols, 300 + i) for i in range(3))
    ha, hb, hc = (_host(f, fmt, rows, cols, target, max_size, colour=2) for f in (fa, fb_, fc))
    m = _input_model(ctx, H, W)
    pin = runtime.PinnedBuffer(fa.shape, np.uint8)
    try:
        m.write_yuv("data", fa, fmt, rows, cols, MEANS, colour=2, **g)
        _same(m.read("data", (1, 3, H, W)), ha, "write_yuv")
        gen = m.generation("data")
        m.write("data", hb)
        m.write_yuv("data", fc, fmt, rows, cols, MEANS, colour=2, **g)
        _same(m.read("data", (1, 3, H, W)), hc, "write_yuv after write")
        assert m.generation("data") == gen + 2
        # the overlapped upload: the bytes on the copy stream into the uint8 shadow, converted at commit
        with pytest.raises(runtime.AccelError, match="no uint8 frames were prefetched"):
            m.commit_yuv("data", 1, lay, MEANS, **g)
        pin.array[...] = fb_
        m.prefetch_u8("data", pin)
        m.commit_yuv("data", 1, lay, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), hb, "prefetch_u8 + commit_yuv")
        pin.array[...] = fa                          # a second round through the same shadow (waits for the first kernel)
        m.prefetch_u8("data", pin)
        m.commit_yuv("data", 1, lay, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), ha, "second prefetch_u8 + commit_yuv")
        with pytest.raises(runtime.AccelError, match="no uint8 frames were prefetched"):
            m.commit_yuv("data", 1, lay, MEANS, **g)
        # too few bytes prefetched: the shortfall is named, nothing is consumed
        m.prefetch_u8("data", pin)
        wide = dict(image.yuv_layout(fmt, rows, cols, pitch=lay["pitch"] + 4), colour=2)      # the same frame at a pitch the bytes do not cover
        with pytest.raises(runtime.AccelError, match="%d bytes, %d were prefetched" % (image.yuv_extent(wide), fb)):
            m.commit_yuv("data", 1, wide, MEANS, **g)
        m.commit_yuv("data", 1, lay, MEANS, **g)
        _same(m.read("data", (1, 3, H, W)), ha, "commit after the refused one")
        # a device-resident source (a frame a decoder left in HBM) off every alignment but the one the format needs, read in place into the other input
        off = 2 if fmt == "p010" else 1
        dev = torch.zeros(fc.size + off, dtype=torch.uint8, device="cuda")
        dev[off:] = torch.from_numpy(fc.reshape(-1))
        torch.cuda.synchronize()                     # torch's stream and the library's compute stream are not ordered by themselves
        assert (dev.data_ptr() + off) % (2 * off) == off
        m.write_yuv_device("data_key", dev.data_ptr() + off, 1, lay, MEANS, **g)
        _same(m.read("data_key", (1, 3, H, W)), hc, "device source")
        _same(m.read("data", (1, 3, H, W)), ha, "the other input is untouched")
        # and the byte converter from HBM into HBM
        out = torch.zeros((1, rows, cols, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.yuv_to_bgr_device(dev.data_ptr() + off, out.data_ptr(), 1, lay, 3 * cols)
        ctx.sync()
        _same_bytes(out.cpu().numpy(), image.yuv_to_bgr_host(fc, fmt, rows, cols, colour=2), "yuv_to_bgr on the device")
        del dev, out
    finally:
        ctx.sync()
        pin.close()
        m.close()


def _refusals(fmt, rows, cols, good):
    """(change of a layout field, the word the message must hold) for every layout the C ABI refuses for this format"""
    row = cols if fmt == "i420" else 2 * cols
    cases = [(dict(format=3), "format"), (dict(format=-1), "format"), (dict(colour=-1), "colour"), (dict(colour=4), "colour"),
             (dict(h=0), "h ="), (dict(h=-2), "h ="), (dict(h=32770), "h ="), (dict(w=0), "w ="), (dict(w=cols - 1), "w ="), (dict(w=32770), "w ="),
             (dict(pitch=row - 1 - (fmt == "p010")), "pitch"), (dict(frame_bytes=good["frame_bytes"] - 1 - (fmt == "p010")), "frame_bytes")]
    if fmt != "yuy2":
        cases += [(dict(h=rows + 1), "h ="), (dict(u_offset=rows * good["pitch"] - 2), "u_offset")]
    if fmt == "i420":
        cases += [(dict(pitch_c=cols // 2 - 1), "pitch_c"), (dict(v_offset=rows * cols - 1), "v_offset"), (dict(pitch=cols + 1), "u_offset"),
                  (dict(pitch_c=cols // 2 + 1), "frame_bytes")]
    else:
        cases += [(dict(pitch_c=row), "pitch_c"), (dict(v_offset=good["frame_bytes"]), "v_offset"), (dict(pitch=row + 2), "u_offset" if fmt == "p010" else "frame_bytes")]
    if fmt == "yuy2":
        cases += [(dict(u_offset=rows * row), "u_offset")]
    if fmt == "p010":
        cases += [(dict(pitch=row + 1, u_offset=rows * (row + 1) + rows % 2, frame_bytes=4 * rows * cols), "pitch"),
                  (dict(u_offset=good["u_offset"] + 1, frame_bytes=good["frame_bytes"] + 2), "u_offset"), (dict(frame_bytes=good["frame_bytes"] + 1), "frame_bytes")]
    return cases


@pytest.mark.parametrize("fmt", FORMATS)
def test_argument_errors_return_err_arg(ctx, fmt):
    """every layout and geometry the kernels could not honour is refused before anything is enqueued, with a message that names the argument"""
    import torch
    from accel_amd import runtime
    lib = runtime.lib()
    rows, cols = 44, 82
    g = _geometry(rows, cols, 48, 96)
    H, W = g["H"], g["W"]
    f = _tight(fmt, 1, rows, cols, 9)
    want = _host(f, fmt, rows, cols, 48, 96)
    means = (ctypes.c_double * 3)(*MEANS)
    src = f.ctypes.data_as(ctypes.c_void_p)
    out = np.full((1, 3, H, W), 7.0, np.float32)
    bgr = np.full((1, rows, cols, 3), 7, np.uint8)
    lay0 = image.yuv_layout(fmt, rows, cols)
    good = dict(lay0, colour=0, n=1, out_h=g["out_h"], out_w=g["out_w"], step=g["step"], H=H, W=W)
    geometry = [(dict(n=0), "n ="), (dict(out_h=H + 1), "out_h"), (dict(out_w=W + 1), "out_w"), (dict(out_h=0), "out_h"), (dict(step=0.0), "step"),
                (dict(step=-1.0), "step"), (dict(step=float("nan")), "step"), (dict(step=1.0), "step")]
    m = _input_model(ctx, H, W)
    pin = runtime.PinnedBuffer(f.shape, np.uint8)
    try:
        m.write_yuv("data", f, fmt, rows, cols, MEANS, **g)

        def lay(a):
            return ctypes.byref(runtime.YUVLayout(*(a[k] for k in ("format", "colour", "h", "w", "pitch", "pitch_c", "u_offset", "v_offset", "frame_bytes"))))

        def res(a):
            return a["out_h"], a["out_w"], a["step"], a["H"], a["W"]

        def op(a):
            return lib.accel_frame_yuv(ctx.handle, src, a["n"], lay(a), means, *res(a), out.ctypes.data_as(ctypes.c_void_p))

        def to_bgr(a):
            return lib.accel_yuv_to_bgr(ctx.handle, src, a["n"], lay(a), bgr.ctypes.data_as(ctypes.c_void_p), 3 * cols, 0)

        def write(a, buf=b"data"):
            return lib.accel_model_write_yuv(m.handle, buf, src, a["n"], lay(a), means, *res(a), 0)

        def commit(a, buf=b"data"):
            return lib.accel_model_commit_yuv(m.handle, buf, a["n"], lay(a), means, *res(a))

        pin.array[...] = f
        m.prefetch_u8("data", pin)
        for cases, calls in ((_refusals(fmt, rows, cols, lay0), (op, to_bgr, write, commit)), (geometry[:1], (op, to_bgr, write, commit)),
                             (geometry[1:], (op, write, commit))):
            for change, word in cases:
                for call in calls:
                    rc = call(dict(good, **change))
                    msg = lib.accel_last_error().decode()
                    assert rc == -1, (call.__name__, change, rc, msg)       # ACCEL_ERR_ARG
                    assert word in msg, (call.__name__, change, msg)
        assert lib.accel_yuv_to_bgr(ctx.handle, src, 1, lay(good), bgr.ctypes.data_as(ctypes.c_void_p), 3 * cols - 1, 0) == -1
        assert "out_pitch" in lib.accel_last_error().decode()
        assert lib.accel_frame_yuv(ctx.handle, None, 1, lay(good), means, *res(good), out.ctypes.data_as(ctypes.c_void_p)) == -1
        assert "yuv" in lib.accel_last_error().decode()
        assert lib.accel_frame_yuv(ctx.handle, src, 1, None, means, *res(good), out.ctypes.data_as(ctypes.c_void_p)) == -1
        assert "layout" in lib.accel_last_error().decode()
        if fmt == "p010":       # an odd device address: refused, never read
            dev = torch.zeros(f.size + 2, dtype=torch.uint8, device="cuda")
            target = torch.zeros(bgr.size, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            odd = ctypes.c_void_p(dev.data_ptr() + 1)
            assert lib.accel_model_write_yuv(m.handle, b"data", odd, 1, lay(good), means, *res(good), 1) == -1
            assert "yuv =" in lib.accel_last_error().decode() and "even" in lib.accel_last_error().decode()
            assert lib.accel_yuv_to_bgr(ctx.handle, odd, 1, lay(good), ctypes.c_void_p(target.data_ptr()), 3 * cols, 1) == -1
            assert "yuv =" in lib.accel_last_error().decode()
            ctx.sync()
            assert not bool(target.any())
            del dev, target
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
        rc = commit(dict(good, **image.yuv_layout(fmt, rows, cols, pitch=lay0["pitch"] + 2)))
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
def _yuv_batches(clip, fmt, rows, cols, cfg, colour, ctx=None):
    from accel_amd import mx
    zero = mx.nd.array(np.zeros((1, cfg.network.DFF_FEAT_DIM, 1, 1)))
    arrs = [mx.nd.yuv_frames(b, fmt, rows, cols, cfg, colour=colour, ctx=ctx) for b in clip]
    return [[arrs[t], arrs[t - 1] if t else arrs[0], zero] for t in range(len(arrs))]


@pytest.mark.parametrize("fmt", FORMATS)
def test_yuv_frames_give_the_logits_of_their_bgr_frames(demo_cfg, fmt):
    """Accel-18, 4 frames of 120 x 250 (a 123 x 256 interior padded to 128 x 256, resampled), interval 3 (key and non-key frames): the input
    tensor is the same and a run is a pure function of its inputs, so I420 / P010 / YUY2 frames must give BIT-IDENTICAL logits and labels to raw
    BGR frames of their host conversion -- through the plain loop and the pinned prefetch loop, with nothing converted on the host -- and the
    finishing calls take such an array as `like`."""
    from accel_amd import demo, mx
    from accel_amd.core import results, tester
    from test_results_gpu import PALETTE
    H, W, rows, cols = 128, 256, 120, 250
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = 16
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    clip = synth.make_clip(rows, cols, 4)
    yuv = [image.bgr_to_yuv_host(f, fmt, 2) for f in clip]
    bgr = [image.yuv_to_bgr_host(b, fmt, rows, cols, colour=2)[0] for b in yuv]
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        ref = _run(r, demo.build_batches(bgr, demo_cfg, raw=True), 3)
        assert not np.array_equal(ref[0][0], ref[1][0])
        plain = _yuv_batches(yuv, fmt, rows, cols, demo_cfg, "bt709")
        assert isinstance(plain[0][0], mx.nd.YUVFrames) and plain[0][0].shape == (1, 3, H, W)
        _identical(_run(r, plain, 3), ref, "%s frames, plain loop" % fmt)
        assert plain[0][0]._host is None and plain[0][0]._frames is None, "the YUV route must not convert anything on the host"
        pinned = _yuv_batches(yuv, fmt, rows, cols, demo_cfg, "bt709", ctx=mx.cpu_pinned())
        assert pinned[0][0].pinned is not None and pinned[0][0].pinned.dtype == np.uint8
        _identical(_run(r, pinned, 3, prefetch=True), ref, "%s frames, pinned prefetch loop" % fmt)
        assert pinned[1][0]._host is None and pinned[1][0]._frames is None
        # a RawFrames, a YUVFrames and an NV12Frames alternate on one runner (frame 0 is a key frame: its logits depend on `data` alone)
        raw = demo.build_batches(bgr, demo_cfg, pinned=True, raw=True)
        zero = raw[0][2]
        nv = mx.nd.nv12_frames(image.bgr_to_nv12_host(clip[2], 2), rows, cols, demo_cfg, colour=2, ctx=mx.cpu_pinned())
        nv_bgr = mx.nd.raw_frames(image.nv12_to_bgr_host(nv.nv12, rows, cols, colour=2), demo_cfg)
        nv_ref = r.step(0, [nv_bgr, nv_bgr, zero], 3)[0].asnumpy().copy()
        r.step(0, raw[0], 3)
        assert r.prefetch(pinned[1])
        assert np.array_equal(r.step(1, [pinned[1][0], raw[0][0], zero], 3)[0].asnumpy(), ref[1][0])
        assert r.prefetch([nv, nv, zero])
        assert np.array_equal(r.step(0, [nv, nv, zero], 3)[0].asnumpy(), nv_ref)
        assert r.prefetch(pinned[0])
        assert np.array_equal(r.step(0, pinned[0], 3)[0].asnumpy(), ref[0][0])
        assert nv._frames is None and pinned[0][0]._frames is None
        # finishing with a YUV array as `like`
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


def test_demo_runs_on_p010_frames(demo_cfg, capsys):
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "3", "--num_ex", "2", "--synthetic", "128x256", "--yuv", "p010", "--finish-on-gpu"])
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    assert out.rstrip().endswith("done") and out.count("testing synthetic_") == 6, out[-1500:]
