"""uint8 video frames, host side: the C ABI declares and exports the entry points, the geometry helper agrees with `resize`, the raw-frame
array stands for the tensor transform(resize(frame)) and the demo builds its batches from raw frames.  (GPU side: test_frames_u8_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
MEANS = (103.06, 115.9, 123.15)
ENTRY_POINTS = ("accel_frame_u8", "accel_model_write_u8", "accel_model_prefetch_u8", "accel_model_commit_u8")

# (rows, cols, target, max) at stride 16: scale 1 / up with padded columns / up with padded rows / up / down / down / portrait down with
# padded rows / portrait with both padded / down to a 16-row image
SIZES = [(48, 96, 48, 96), (96, 48, 48, 96), (45, 83, 48, 96), (37, 91, 64, 128), (33, 57, 48, 96), (60, 120, 48, 96),
         (50, 100, 64, 96), (100, 75, 48, 96), (61, 47, 48, 80), (23, 150, 48, 96)]


def test_header_declares_and_library_exports_the_entry_points():
    from accel_amd import runtime
    hdr = open(os.path.join(ROOT, "include", "accel_hip.h")).read()
    declared = set(re.findall(r"\b(accel_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, "include/accel_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libaccel_hip.so does not export %s" % name
    runtime.lib()
    assert set(ENTRY_POINTS) <= set(runtime.EXPORTS)
    for name in ("frame_u8",):
        assert hasattr(runtime.Context, name)
    for name in ("write_u8", "write_u8_device", "prefetch_u8", "commit_u8"):
        assert hasattr(runtime.Model, name)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


@pytest.mark.parametrize("rows,cols,target,max_size", SIZES + [(1024, 2048, 1024, 2048), (720, 1280, 1024, 2048), (120, 250, 128, 256)])
@pytest.mark.parametrize("stride", [0, 16])
def test_geometry_agrees_with_resize(rows, cols, target, max_size, stride):
    im = np.zeros((rows, cols, 3), np.uint8)
    plain, scale = image.resize(im, target, max_size)
    padded, scale2 = image.resize(im, target, max_size, stride=stride)
    g = image.resize_geometry(rows, cols, target, max_size, stride)
    assert g[0] == scale == scale2
    assert (g[1], g[2]) == plain.shape[:2]
    assert (g[3], g[4]) == padded.shape[:2]
    step = image.resample_step(rows, cols, g[0], g[1], g[2])
    assert step == (1.0 if (g[1], g[2]) == (rows, cols) else 1.0 / scale)


def test_geometry_of_the_named_cases():
    assert image.resize_geometry(1024, 2048, 1024, 2048, 0) == (1.0, 1024, 2048, 1024, 2048)
    assert image.resize_geometry(120, 250, 128, 256, 16) == (1.024, 123, 256, 128, 256)
    # a scale other than 1 whose rounded size is the frame's own: `resize` copies the frame, so the step is exactly 1
    rows, cols = 100, 200
    g = image.resize_geometry(rows, cols, 100.2, 400, 0)
    assert g[0] != 1.0 and g[1:3] == (rows, cols)
    assert image.resample_step(rows, cols, g[0], g[1], g[2]) == 1.0
    im = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    assert image.resize(im, 100.2, 400)[0] is im


def _cfg(demo_cfg, target, max_size, stride):
    demo_cfg.SCALES[0] = (target, max_size)
    demo_cfg.network.IMAGE_STRIDE = stride
    return demo_cfg


def _host(frames, cfg):
    t, m = cfg.SCALES[0]
    return np.concatenate([image.transform(image.resize(f, t, m, stride=cfg.network.IMAGE_STRIDE)[0], cfg.network.PIXEL_MEANS)
                           for f in frames]).astype(np.float32)


@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (45, 83, 48, 96), (61, 47, 48, 80), (120, 250, 128, 256)])
def test_raw_frame_array_stands_for_the_host_tensor(demo_cfg, rows, cols, target, max_size):
    from accel_amd import mx
    cfg = _cfg(demo_cfg, target, max_size, 16)
    rng = np.random.default_rng(rows * 1000 + cols)
    frames = rng.integers(0, 256, (2, rows, cols, 3), dtype=np.uint8)
    keep = frames.copy()
    raw = mx.nd.raw_frames(frames, cfg)
    assert isinstance(raw, mx.nd.NDArray) and isinstance(raw, mx.nd.RawFrames)
    scale, out_h, out_w, H, W = image.resize_geometry(rows, cols, target, max_size, 16)
    assert raw.shape == (2, 3, H, W)
    assert raw.frames.dtype == np.uint8 and raw.frames.shape == (2, rows, cols, 3)
    assert raw.means == MEANS and raw.geometry["H"] == H and raw.geometry["out_w"] == out_w
    frames[...] = 0                               # the payload is a copy: editing the source does not reach it
    np.testing.assert_array_equal(raw.frames, keep)
    assert not raw.frames.flags.writeable
    want = _host(keep, cfg)
    got = raw.asnumpy()
    assert got.dtype == np.float32 and got.shape == raw.shape
    assert np.array_equal(got, want)
    neg = -np.asarray(MEANS, np.float64)
    for c in range(3):                             # plane 2 - c holds source channel c: the padding is fp32(0 - mean[c]), not 0
        assert np.all(got[:, 2 - c, out_h:, :] == np.float32(neg[c]))
        assert np.all(got[:, 2 - c, :, out_w:] == np.float32(neg[c]))
    one = mx.nd.raw_frames(keep[0], cfg)           # one h x w x 3 frame, and a list of frames
    assert one.shape == (1, 3, H, W)
    assert np.array_equal(mx.nd.raw_frames([keep[0], keep[1]], cfg).asnumpy(), want)
    with pytest.raises(ValueError):
        mx.nd.raw_frames([keep[0], keep[1][:-1]], cfg)
    with pytest.raises(ValueError):
        mx.nd.raw_frames(keep.astype(np.float32), cfg)


def test_fp32_subtraction_is_not_the_contract():
    """the value is fp32(double(grey) - mean): subtracting in fp32 differs at 128, 64 and 64 of the 256 grey levels"""
    g = np.arange(256)
    diff = [int(np.count_nonzero((g.astype(np.float64) - m).astype(np.float32) != g.astype(np.float32) - np.float32(m))) for m in MEANS]
    assert diff == [128, 64, 64]


def test_build_batches_raw(demo_cfg):
    from accel_amd import demo, mx
    from accel_amd.utils import synth
    cfg = _cfg(demo_cfg, 128, 256, 16)
    frames = synth.make_clip(120, 250, 4)
    plain = demo.build_batches(frames, cfg)
    raw = demo.build_batches(frames, cfg, raw=True)
    assert len(raw) == len(plain) == 4
    for t in range(4):
        assert [a.shape for a in raw[t]] == [a.shape for a in plain[t]]
        assert isinstance(raw[t][0], mx.nd.RawFrames) and raw[t][0].pinned is None
        assert raw[t][1] is (raw[t - 1][0] if t else raw[0][0])      # frame t's data is frame t + 1's data_key OBJECT
        assert np.array_equal(raw[t][0].asnumpy(), plain[t][0].asnumpy())
    assert raw[0][0].shape == (1, 3, 128, 256)


def test_demo_has_the_raw_frames_flag():
    from accel_amd import demo
    with pytest.raises(SystemExit) as e:
        demo.main(["--raw-frames", "--help"])
    assert e.value.code == 0
