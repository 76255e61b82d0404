"""Finished frames, host side: the C ABI declares and exports the entry points, the integer nearest rule is the evaluator's float64 rule,
and the two host restatements the GPU is tested against (utils/image.py labels_to_source_host, colour_host) do what they say.
(GPU side: test_results_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

from test_frames_u8_cpu import SIZES

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("accel_labels_to_source", "accel_labels_hist", "accel_labels_colour", "accel_model_labels_to_source", "accel_model_hist_add",
                "accel_model_hist_read", "accel_model_labels_colour")
ALPHAS = (0, 1, 128, 255, 256)


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
    for name in ("labels_to_source", "labels_hist", "labels_colour"):
        assert hasattr(runtime.Context, name)
    for name in ("labels_to_source", "hist_add", "hist_read", "labels_colour"):
        assert hasattr(runtime.Model, name)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


def test_python_surface():
    from accel_amd.core import results
    for name in ("labels_at_source", "colour", "Evaluator"):
        assert hasattr(results, name)
    ev = results.Evaluator(19)
    assert ev.hist().dtype == np.int64 and ev.hist().shape == (19, 19) and not ev.hist().any()
    for name in ("add", "hist", "per_class_iu"):
        assert hasattr(ev, name)
    with pytest.raises(ValueError):
        results.Evaluator(33)


def test_integer_nearest_rule_is_the_float64_rule_of_the_evaluator():
    """min(i * src // dst, src - 1) against the expression of dataset/cityscape._nearest_resize, for every (src, dst) pair of the grid"""
    from accel_amd.dataset import cityscape
    sizes = list(range(1, 260)) + [720, 1024, 1080, 1280, 1920, 2048, 4096]
    for src in sizes:
        ramp = np.arange(src)[None, :]                           # a 1 x src map whose value is its column: resizing it returns the index
        for dst in sizes:
            want = cityscape._nearest_resize(ramp, 1, dst)[0]
            got = image.nearest_index(dst, src)
            assert np.array_equal(got, want), (src, dst, np.flatnonzero(got != want)[:4])


@pytest.mark.parametrize("rows,cols,target,max_size", SIZES)
@pytest.mark.parametrize("stride", [0, 16])
def test_labels_to_source_host_inverts_the_geometry(rows, cols, target, max_size, stride):
    """a label map that is one class on the valid region and another in the padding: no padding value may reach the source size"""
    scale, out_h, out_w, H, W = image.resize_geometry(rows, cols, target, max_size, stride)
    labels = np.full((2, H, W), 7, np.uint8)
    labels[:, :out_h, :out_w] = 3
    got = image.labels_to_source_host(labels, out_h, out_w, rows, cols)
    assert got.dtype == np.uint8 and got.shape == (2, rows, cols) and got.flags.c_contiguous
    assert np.all(got == 3)
    # and it is _nearest_resize of the cropped region, pixel for pixel
    from accel_amd.dataset import cityscape
    rnd = np.random.default_rng(rows * 131 + cols).integers(0, 19, (H, W), dtype=np.uint8)
    assert np.array_equal(image.labels_to_source_host(rnd, out_h, out_w, rows, cols), cityscape._nearest_resize(rnd[:out_h, :out_w], rows, cols))


def test_labels_to_source_host_at_scale_one_is_the_crop():
    rnd = np.random.default_rng(3).integers(0, 19, (3, 48, 96), dtype=np.uint8)
    assert np.array_equal(image.labels_to_source_host(rnd, 48, 96, 48, 96), rnd)
    assert np.array_equal(image.labels_to_source_host(rnd, 45, 83, 45, 83), rnd[:, :45, :83])
    assert np.array_equal(image.labels_to_source_host(rnd[0], 45, 83, 45, 83), rnd[0, :45, :83])


def test_colour_host_is_the_palette_lookup_and_the_stated_blend():
    from accel_amd.dataset.cityscape import getpallete
    pal = getpallete(256)
    rng = np.random.default_rng(11)
    labels = rng.integers(0, 256, (2, 9, 13), dtype=np.uint8)
    frames = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    frames[0, 0, 0] = 255
    frames[0, 0, 1] = 0
    rgb = pal.reshape(-1, 3)[labels]
    assert np.array_equal(image.colour_host(labels, pal), rgb)
    assert np.array_equal(image.colour_host(labels, pal, rgb=False), rgb[..., ::-1])
    assert np.array_equal(image.colour_host(labels, pal.reshape(256, 3), frames=frames), rgb)       # alpha 256: the pure colour
    for alpha in ALPHAS:
        for order in (True, False):
            c = (rgb if order else rgb[..., ::-1]).astype(np.int64)
            f = (frames[..., ::-1] if order else frames).astype(np.int64)      # the frame is B, G, R
            want = ((alpha * c + (256 - alpha) * f + 128) >> 8)
            assert want.min() >= 0 and want.max() <= 255
            got = image.colour_host(labels, pal, frames=frames, alpha=alpha, rgb=order)
            assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)), (alpha, order)
    assert np.array_equal(image.colour_host(labels, pal, frames=frames, alpha=0, rgb=False), frames)
    assert np.array_equal(image.colour_host(labels, pal, frames=frames, alpha=0), frames[..., ::-1])
    with pytest.raises(ValueError):
        image.colour_host(labels, pal, frames=frames, alpha=257)


def test_demo_has_the_finish_on_gpu_flag():
    from accel_amd import demo
    with pytest.raises(SystemExit) as e:
        demo.main(["--raw-frames", "--finish-on-gpu", "--help"])
    assert e.value.code == 0
