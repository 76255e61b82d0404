"""Per-pixel confidence, host side: utils.image.confidence_host -- the float64 specification the GPU is tested against -- does what it
says, the C ABI declares and exports the entry points, and the GUARD CONDITION holds for every input the GPU tests use: no pixel has 256 * p
within 1e-9 of an integer unless its byte cannot depend on the last bits of an exp.  That is what lets test_confidence_gpu.py demand
equality of every byte.  (GPU side: test_confidence_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from accel_amd.utils import image

import confidence_ref as ref

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("accel_scores_confidence", "accel_model_confidence")


def _some_cases():
    """one case per class count and scale, over different geometries"""
    out = []
    for i, ncls in enumerate(ref.NCLS):
        for j, s in enumerate(ref.SCALES):
            out.append(ref.small_case(*ref.SMALL[(4 * i + j) % len(ref.SMALL)], ncls=ncls, n=2, scale=s))
    return out


def _map_result(case):
    """confidence_host at the MAP's own resolution (the valid region, no resampling)"""
    return image.confidence_host(ref.scores(case), case.out_h, case.out_w, case.out_h, case.out_w, is_prob=ref.is_prob(case))


def test_header_declares_and_library_exports_the_entry_points():
    from accel_amd import runtime
    from accel_amd.core import results
    hdr = open(os.path.join(ROOT, "include", "accel_hip.h")).read()
    declared = set(re.findall(r"\b(accel_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, "include/accel_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libaccel_hip.so does not export %s" % name
    runtime.lib()
    assert set(ENTRY_POINTS) <= set(runtime.EXPORTS)
    assert hasattr(runtime.Context, "scores_confidence")
    assert hasattr(runtime.Model, "confidence") and hasattr(runtime.Model, "confidence_device")
    assert hasattr(results, "confidence")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name


@pytest.mark.parametrize("case", _some_cases(), ids=lambda c: "ncls%d-s%g" % (c.ncls, c.scale))
def test_conf_is_the_largest_softmax_probability_in_256_levels(case):
    """against torch.softmax in float64 (another exp, another summation order: equal bytes because of the guard condition below)"""
    conf, _, _, _ = _map_result(case)
    s = torch.from_numpy(ref.scores(case)[:, :, :case.out_h, :case.out_w].copy()).double()
    p = torch.softmax(s, dim=1).max(dim=1).values.numpy()
    want = np.minimum(255.0, np.floor(256.0 * p)).astype(np.uint8)
    assert conf.dtype == np.uint8 and conf.shape == (case.n, case.out_h, case.out_w)
    assert np.array_equal(conf, want), int(np.count_nonzero(conf != want))


@pytest.mark.parametrize("case", _some_cases(), ids=lambda c: "ncls%d-s%g" % (c.ncls, c.scale))
def test_second_and_margin_are_the_sort_based_restatement(case):
    _, margin, second, _ = _map_result(case)
    s = ref.scores(case)[:, :, :case.out_h, :case.out_w]
    order = np.argsort(-s.astype(np.float64), axis=1, kind="stable")      # descending, the earlier index first among equals
    best, runner = order[:, 0], order[:, 1]
    assert np.array_equal(best, np.argmax(s, axis=1))
    assert second.dtype == np.uint8 and np.array_equal(second, runner)
    top1, top2 = np.take_along_axis(s, best[:, None], 1)[:, 0], np.take_along_axis(s, runner[:, None], 1)[:, 0]
    assert margin.dtype == np.float32 and np.array_equal(margin, top1 - top2)
    assert (margin >= 0).all()


@pytest.mark.parametrize("case", _some_cases() + ref.multiblock_cases() + ref.prob_cases()[:2], ids=str)
def test_source_mapping_is_that_of_the_labels(case):
    """every output at the source size is labels_to_source_host of the map-resolution output, and hist is bincount of conf"""
    conf, margin, second, hist = ref.reference(case)
    mc, mm, ms, _ = _map_result(case)
    for got, at_map in ((conf, mc), (margin, mm), (second, ms)):
        assert got.shape == (case.n, case.h, case.w)
        assert np.array_equal(got, image.labels_to_source_host(at_map, case.out_h, case.out_w, case.h, case.w))
    assert hist.dtype == np.uint64 and hist.shape == (case.n, 256)
    for f in range(case.n):
        assert np.array_equal(hist[f].astype(np.int64), np.bincount(conf[f].reshape(-1), minlength=256))
        assert int(hist[f].sum()) == case.h * case.w


def test_padding_never_reaches_the_source_size():
    s = np.full((1, 19, 32, 64), 50.0, np.float32)      # padding: all classes equal -> conf 13
    s[:, :, :29, :50] = 0
    s[:, 4, :29, :50] = 100                            # valid region: saturated on class 4
    conf, margin, second, hist = image.confidence_host(s, 29, 50, 58, 75)
    assert (conf == 255).all() and (margin == 100).all() and (second == 0).all() and int(hist[0, 255]) == 58 * 75


@pytest.mark.parametrize("case", ref.known_cases(), ids=str)
def test_known_answers(case):
    conf, margin, second, hist = ref.reference(case)
    if case.kind == "equal":            # p = 1 / ncls
        assert (conf == {2: 128, 19: 13, 21: 12}[case.ncls]).all() and (margin == 0).all() and (second == 1).all()
    elif case.kind == "one100":         # p = 1 -> 256 -> 255
        assert (conf == 255).all() and (margin == 100).all()
        assert (second == (1 if ref.known_winner(case) == 0 else 0)).all()
    else:                               # a two-way tie at the top: margin 0, the runner-up is the later index
        a, b = ref.known_tie(case)
        assert (margin == 0).all() and (second == b).all()
        # p = 1 / (2 + (ncls - 2) * exp(-3))
        want = int(np.floor(256.0 / (2.0 + (case.ncls - 2) * np.exp(-3.0))))
        assert (conf == want).all()
    assert int(hist.sum()) == case.n * case.h * case.w


def test_two_equal_classes_give_exactly_128():
    s = np.random.default_rng(5).standard_normal((1, 1, 8, 8)).astype(np.float32).repeat(2, axis=1)
    conf, margin, second, _ = image.confidence_host(s, 8, 8, 8, 8)
    assert (conf == 128).all() and (margin == 0).all() and (second == 1).all()


def test_probabilities_are_scaled_not_exponentiated():
    p = np.array([0.5, 0.25, 0.25, 1.0, 0.0, 0.0, 0.999, 0.0005, 0.0005], np.float32).reshape(1, 3, 3, 1).transpose(0, 2, 1, 3).copy()
    conf, margin, second, _ = image.confidence_host(p, 3, 1, 3, 1, is_prob=True)
    assert conf.reshape(-1).tolist() == [128, 255, int(np.floor(256.0 * float(np.float32(0.999))))]
    assert second.reshape(-1).tolist() == [1, 1, 1]
    assert np.array_equal(margin.reshape(-1), np.array([0.25, 1.0, np.float32(0.999) - np.float32(0.0005)], np.float32))


def test_guard_condition_of_the_gpu_inputs():
    """For every input of test_confidence_gpu.py: 256 * p is farther than GUARD = 1e-9 from every integer at every pixel whose byte an exp
    could move.  float64 exp implementations and summation orders differ by a few ulp (~1e-13 at 256): with this margin the byte has one
    value, and the GPU tests compare with np.array_equal.  A condition, not a tolerance: if a seed violates it, change the seed."""
    cases = ref.all_cases()
    assert len(cases) >= 240
    for case in cases:
        v, exact = ref.scaled_float64(case)
        dist = np.abs(v - np.rint(v))
        bad = (dist < ref.GUARD) & ~exact
        assert not bad.any(), (case, int(bad.sum()), v[bad][:4])


def test_demo_has_the_confidence_flag():
    from accel_amd import demo
    with pytest.raises(SystemExit) as e:
        demo.main(["--raw-frames", "--finish-on-gpu", "--confidence", "--help"])
    assert e.value.code == 0
    with pytest.raises(ValueError, match="finish-on-gpu"):
        demo.main(["--confidence", "--synthetic", "32x64"])


def test_confidence_summary_reads_the_histogram():
    from accel_amd.core import results
    h = np.zeros(256, np.uint64)
    h[255], h[0] = 3, 1
    mean, low = results.confidence_summary(h)
    assert low == 0.25 and abs(mean - (3 * 255.5 / 256 + 0.5 / 256) / 4) < 1e-15
