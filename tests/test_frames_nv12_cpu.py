"""NV12 video frames, host side: the C ABI declares and exports the entry points, the library's coefficient table is the one utils/image.py
derives from the standards, the integer rule is a fair restatement of the standards' float matrices, the host conversion honours the layout,
the NV12 array stands for the tensor transform(resize(nv12_to_bgr_host(frame))) and the demo takes --nv12.  (GPU side: test_frames_nv12_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
MEANS = (103.06, 115.9, 123.15)
ENTRY_POINTS = ("accel_nv12_coefficients", "accel_frame_nv12", "accel_nv12_to_bgr", "accel_model_write_nv12", "accel_model_commit_nv12")
# colour -> (yoff, ky, krv, kgu, kgv, kbu): round(65536 x the standard's value)
TABLE = {0: (16, 76309, 104597, 25675, 53279, 132201),      # BT.601 limited
         1: (0, 65536, 91881, 22553, 46802, 116130),        # BT.601 full
         2: (16, 76309, 117489, 13975, 34925, 138438),      # BT.709 limited
         3: (0, 65536, 103206, 12276, 30679, 121609)}       # BT.709 full


def test_header_declares_and_library_exports_the_entry_points():
    from accel_amd import runtime
    hdr = open(os.path.join(ROOT, "include", "accel_hip.h")).read()
    declared = set(re.findall(r"\b(accel_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in ENTRY_POINTS + ("accel_model_prefetch_u8",):       # six symbols: the prefetch is the uint8 one
        assert name in declared, "include/accel_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libaccel_hip.so does not export %s" % name
    runtime.lib()
    assert set(ENTRY_POINTS) <= set(runtime.EXPORTS)
    for name in ("frame_nv12", "nv12_to_bgr"):
        assert hasattr(runtime.Context, name)
    for name in ("write_nv12", "write_nv12_device", "commit_nv12"):
        assert hasattr(runtime.Model, name)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


def test_coefficients_of_the_library_of_python_and_of_the_table_agree():
    from accel_amd import runtime
    assert image.NV12_COLOURS == {"bt601": 0, "bt601-full": 1, "bt709": 2, "bt709-full": 3}
    for name, c in image.NV12_COLOURS.items():
        assert image.nv12_coefficients(c) == image.nv12_coefficients(name) == TABLE[c]
        assert runtime.nv12_coefficients(c) == TABLE[c]
    out = (ctypes.c_int32 * 6)()
    for bad in (-1, 4):
        assert runtime.lib().accel_nv12_coefficients(bad, out) == -1       # ACCEL_ERR_ARG
        assert "colour" in runtime.lib().accel_last_error().decode()
        with pytest.raises(ValueError, match="colour"):
            image.nv12_coefficients(bad)
    with pytest.raises(ValueError, match="colour"):
        image.nv12_coefficients("bt2020")


@pytest.mark.parametrize("colour", [0, 1, 2, 3])
def test_integer_rule_is_within_one_level_of_the_float_matrix(colour):
    """all 2^24 (Y, Cb, Cr) triples: the integer rule against clip(rint(the standard's float64 matrix)) differs by at most one level per
    channel, at a share of at most 1e-3 of the triples per channel.  (R does not depend on Cb and B not on Cr, in either rule: their 2^16
    pairs stand for the 2^24 triples with the same share.)"""
    yoff, ky, krv, kgu, kgv, kbu = image.nv12_matrix(colour)
    v = np.arange(256)
    quant = lambda a: np.clip(np.rint(a), 0, 255).astype(np.int64)
    y2, c2 = np.meshgrid(v, v, indexing="ij")
    yf, cf = ky * (y2.astype(np.float64) - yoff), c2.astype(np.float64) - 128.0
    b, _, _ = image.yuv_to_bgr(y2, c2, np.full_like(c2, 128), colour)
    _, _, r = image.yuv_to_bgr(y2, np.full_like(c2, 128), c2, colour)
    y3, cb3, cr3 = np.meshgrid(v, v, v, indexing="ij")
    _, g, _ = image.yuv_to_bgr(y3, cb3, cr3, colour)
    gf = ky * (y3.astype(np.float64) - yoff) - kgu * (cb3.astype(np.float64) - 128.0) - kgv * (cr3.astype(np.float64) - 128.0)
    assert g.size == 1 << 24
    for name, got, want in (("R", r, quant(yf + krv * cf)), ("G", g, quant(gf)), ("B", b, quant(yf + kbu * cf))):
        diff = np.abs(got.astype(np.int64) - want)
        share = float(np.count_nonzero(diff)) / diff.size
        print("colour %d %s: max %d level(s), share %.3g" % (colour, name, diff.max(), share))
        assert diff.max() <= 1, (colour, name, int(diff.max()))
        assert share <= 1e-3, (colour, name, share)


@pytest.mark.parametrize("colour", [0, 1, 2, 3])
def test_known_answers(colour):
    v = np.arange(256, dtype=np.uint8)
    grey = np.full(256, 128, np.uint8)
    b, g, r = image.yuv_to_bgr(v, grey, grey, colour)
    assert np.array_equal(b, g) and np.array_equal(g, r)        # no chroma: a grey pixel
    if colour in (1, 3):
        assert np.array_equal(g, v)                               # full range gives back Y exactly
    else:
        assert g[16] == 0 and g[235] == 255
        assert np.all(g[:16] == 0) and np.all(g[235:] == 255)     # below black and above white clip
        assert np.all(np.diff(g[16:236].astype(int)) >= 1)
    # strong chroma saturates instead of wrapping
    b, g, r = image.yuv_to_bgr(np.uint8([255, 0]), np.uint8([255, 0]), np.uint8([255, 0]), colour)
    assert (b[0], r[0]) == (255, 255) and (b[1], r[1]) == (0, 0)


def _tight(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h * w * 3 // 2), dtype=np.uint8)


def _spread(tight, h, w, pitch, uv_offset, frame_bytes, seed):
    """the frames of `tight` laid out with a row pitch, a gap between the planes and a tail, random bytes in every gap"""
    n = tight.shape[0]
    out = np.random.default_rng(seed).integers(0, 256, (n, frame_bytes), dtype=np.uint8)
    for i in range(n):
        for y in range(h):
            out[i, y * pitch:y * pitch + w] = tight[i, y * w:(y + 1) * w]
        for y in range(h // 2):
            out[i, uv_offset + y * pitch:uv_offset + y * pitch + w] = tight[i, h * w + y * w:h * w + (y + 1) * w]
    return out


def test_layout_gaps_are_not_interpreted():
    h, w = 6, 10
    tight = _tight(2, h, w, 1)
    want = image.nv12_to_bgr_host(tight, h, w, colour=2)
    assert want.shape == (2, h, w, 3) and want.dtype == np.uint8
    assert np.array_equal(image.nv12_to_bgr_host(tight.reshape(-1), h, w, colour=2), want)       # a flat run of whole frames
    pitch, uv_offset = w + 7, (w + 7) * (h + 3)
    frame_bytes = uv_offset + (h // 2) * pitch + 5
    for seed in (2, 3):
        spread = _spread(tight, h, w, pitch, uv_offset, frame_bytes, seed)
        assert np.array_equal(image.nv12_to_bgr_host(spread, h, w, pitch, uv_offset, frame_bytes, colour=2), want)
    # chroma is replicated over each 2 x 2 block and read in (Cb, Cr) order
    one = np.zeros((1, 6), np.uint8)
    one[0] = (50, 100, 150, 200, 90, 240)
    got = image.nv12_to_bgr_host(one, 2, 2, colour=1)[0]
    for (y, x), luma in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (50, 100, 150, 200)):
        b, g, r = image.yuv_to_bgr(luma, 90, 240, 1)
        assert tuple(got[y, x]) == (int(b), int(g), int(r))
    assert got[0, 0, 2] > got[0, 0, 0]                # Cr = 240 is red
    for bad in (dict(pitch=w - 1), dict(uv_offset=h * w - 1), dict(frame_bytes=h * w * 3 // 2 - 1)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            image.nv12_layout(h, w, **bad)
    with pytest.raises(ValueError):
        image.nv12_to_bgr_host(tight.reshape(-1)[:-1], h, w)


@pytest.mark.parametrize("colour", [0, 3])
def test_bgr_to_nv12_has_the_documented_size_and_is_accepted_back(colour):
    rng = np.random.default_rng(colour)
    f = rng.integers(0, 256, (2, 8, 12, 3), dtype=np.uint8)
    nv = image.bgr_to_nv12_host(f, colour)
    assert nv.dtype == np.uint8 and nv.shape == (2, 8 * 12 * 3 // 2)
    assert image.bgr_to_nv12_host(f[0], colour).shape == (1, 8 * 12 * 3 // 2)
    assert image.nv12_to_bgr_host(nv, 8, 12, colour=colour).shape == f.shape
    flat = np.empty((1, 8, 12, 3), np.uint8)
    flat[...] = (40, 120, 200)                        # a frame of one colour comes back within the quantisation of two conversions
    back = image.nv12_to_bgr_host(image.bgr_to_nv12_host(flat, colour), 8, 12, colour=colour)
    assert np.abs(back.astype(int) - flat.astype(int)).max() <= 2
    for bad in (f[:, :7], f[:, :, :11]):
        with pytest.raises(ValueError, match="even"):
            image.bgr_to_nv12_host(bad, colour)


def _cfg(demo_cfg, target, max_size, stride):
    demo_cfg.SCALES[0] = (target, max_size)
    demo_cfg.network.IMAGE_STRIDE = stride
    return demo_cfg


def _host(bgr, cfg):
    t, m = cfg.SCALES[0]
    return np.concatenate([image.transform(image.resize(f, t, m, stride=cfg.network.IMAGE_STRIDE)[0], cfg.network.PIXEL_MEANS)
                           for f in bgr]).astype(np.float32)


@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (44, 82, 48, 96), (60, 46, 48, 80), (120, 250, 128, 256)])
def test_nv12_array_stands_for_the_host_tensor(demo_cfg, rows, cols, target, max_size):
    from accel_amd import mx
    cfg = _cfg(demo_cfg, target, max_size, 16)
    buf = _tight(2, rows, cols, rows * 1000 + cols)
    keep = buf.copy()
    arr = mx.nd.nv12_frames(buf, rows, cols, cfg, colour="bt709")
    assert isinstance(arr, mx.nd.NDArray) and isinstance(arr, mx.nd.RawFrames) and isinstance(arr, mx.nd.NV12Frames)
    like = mx.nd.raw_frames(np.zeros((2, rows, cols, 3), np.uint8), cfg)
    assert arr.shape == like.shape and arr.geometry == like.geometry and arr.scale == like.scale and arr.means == like.means == MEANS
    assert arr.layout == dict(n=2, h=rows, w=cols, pitch=cols, uv_offset=rows * cols, frame_bytes=rows * cols * 3 // 2, colour=2)
    buf[...] = 0                                      # the payload is a copy: editing the source does not reach it
    assert np.array_equal(arr.nv12, keep) and not arr.nv12.flags.writeable
    assert arr._frames is None                        # nothing converted on the host so far
    bgr = image.nv12_to_bgr_host(keep, rows, cols, colour=2)
    want = _host(bgr, cfg)
    got = arr.asnumpy()
    assert got.dtype == np.float32 and got.shape == arr.shape and np.array_equal(got, want)
    assert np.array_equal(arr.frames, bgr) and arr.frames.shape == like.frames.shape and not arr.frames.flags.writeable
    # one flat frame, a flat run of frames and a list of frames
    assert np.array_equal(mx.nd.nv12_frames(keep[0], rows, cols, cfg, colour=2).asnumpy(), want[:1])
    assert np.array_equal(mx.nd.nv12_frames(keep.reshape(-1), rows, cols, cfg, colour="bt709").asnumpy(), want)
    assert np.array_equal(mx.nd.nv12_frames([keep[0], keep[1]], rows, cols, cfg, colour="bt709").asnumpy(), want)
    assert not np.array_equal(mx.nd.nv12_frames(keep, rows, cols, cfg).asnumpy(), want)      # the default is BT.601 limited range
    # a pitched layout: rows of an n x frame_bytes buffer are the frames
    pitch, uv_offset = cols + 12, (cols + 12) * (rows + 6)
    frame_bytes = uv_offset + (rows // 2) * pitch + 5
    spread = _spread(keep, rows, cols, pitch, uv_offset, frame_bytes, 7)
    pitched = mx.nd.nv12_frames(spread, rows, cols, cfg, colour="bt709", pitch=pitch, uv_offset=uv_offset)
    assert pitched.layout["frame_bytes"] == frame_bytes and np.array_equal(pitched.asnumpy(), want)


def test_nv12_array_refuses_what_is_not_nv12(demo_cfg):
    from accel_amd import mx
    cfg = _cfg(demo_cfg, 48, 96, 16)
    good = _tight(1, 48, 96, 0)
    with pytest.raises(ValueError, match="h = 47"):
        mx.nd.nv12_frames(good, 47, 96, cfg)
    with pytest.raises(ValueError, match="w = 95"):
        mx.nd.nv12_frames(good, 48, 95, cfg)
    with pytest.raises(ValueError, match="frame_bytes"):
        mx.nd.nv12_frames(good.reshape(-1)[:-1], 48, 96, cfg)          # a wrong byte count
    with pytest.raises(ValueError, match="frame_bytes"):
        mx.nd.nv12_frames(good[:, :-2], 48, 96, cfg)
    with pytest.raises(ValueError, match="uint8"):
        mx.nd.nv12_frames(good.astype(np.float32), 48, 96, cfg)
    with pytest.raises(ValueError, match="colour"):
        mx.nd.nv12_frames(good, 48, 96, cfg, colour="rec2020")
    with pytest.raises(ValueError, match="same number of bytes"):
        mx.nd.nv12_frames([good[0], good[0][:-2]], 48, 96, cfg)


def test_build_batches_nv12(demo_cfg):
    from accel_amd import demo, mx
    from accel_amd.utils import synth
    cfg = _cfg(demo_cfg, 128, 256, 16)
    frames = synth.make_clip(120, 250, 3)
    raw = demo.build_batches(frames, cfg, raw=True)
    nv = demo.build_batches(frames, cfg, raw=True, nv12="bt709-full")
    for t in range(3):
        assert isinstance(nv[t][0], mx.nd.NV12Frames) and nv[t][0].layout["colour"] == 3
        assert [a.shape for a in nv[t]] == [a.shape for a in raw[t]]
        assert nv[t][1] is (nv[t - 1][0] if t else nv[0][0])
        assert np.array_equal(nv[t][0].nv12, image.bgr_to_nv12_host(frames[t], 3))
    with pytest.raises(ValueError, match="odd-sized"):
        demo.build_batches(synth.make_clip(121, 250, 1), cfg, raw=True, nv12="bt601")


def test_demo_has_the_nv12_flag_and_rejects_odd_sized_frames(demo_cfg):
    from accel_amd import demo
    with pytest.raises(SystemExit) as e:
        demo.main(["--nv12", "bt709", "--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit) as e:
        demo.main(["--nv12", "bt2020"])
    assert e.value.code != 0
    with pytest.raises(ValueError, match="odd-sized"):
        demo.main(["--version", "18", "--num_ex", "1", "--interval", "2", "--synthetic", "127x256", "--nv12"])
