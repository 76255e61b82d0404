"""conv_ref.py against the oracle and torch: the float64 reference of a plan `conv` line is right, an honest fp32 evaluation of every
case of the table (the C oracle's convolution, the epilogue in numpy fp32) stays inside the bound and the bar test_conv_views_gpu.py
asserts for it, and the table covers what it says it covers.

Measured here: the fp32 restatement of Winograd F(2x2, 3x3) (conv_ref.wino32) against float64, relative to max|ref| --
K = 288 (Cin 32, 12x18): 2.0e-07; K = 576 (Cin 64, 8x8): 2.8e-07; K = 1152 (Cin 128, 8x8): 3.9e-07; K = 2304 (Cin 256, 6x8): 6.8e-07
(Cout 136) and 7.9e-07 (Cout 18) -- four times that is the deep-K bar of the GPU test where it exceeds 3e-6 (the last one: 3.15e-6)."""
import numpy as np
import pytest
import torch

import conv_ref as R
from oracle import ops as O
from plan_helpers import conv64, deconv64


def _unique(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


def test_the_table_covers_every_launch_geometry_and_epilogue():
    import test_ops_gpu
    assert R.ALL_TILES == test_ops_gpu.ALL_TILES and sorted(t for ids in R.CLASSES.values() for t in ids) == R.ALL_TILES
    ids = [c.id for c in R.CASES]
    assert len(set(ids)) == len(ids)
    run = lambda pred: [c for c in R.RUN_CASES if pred(c)]
    # every fp32 schedule class: all four epilogues, a pad case, a strided dilated 3x3 and a strided 1x1
    for cls, tiles in R.CLASSES.items():
        cs = run(lambda c: c.fam == "igemm-" + cls)
        assert {c.tile for c in cs} == set(tiles)
        assert {(tuple(sorted(c.epi)), c.act) for c in cs} >= {(tuple(sorted(e.split("+"))), a) for e, a in R.ROT}
        assert any(c.Cout == 18 for c in cs) and any(c.d == 2 and c.s == 2 for c in cs) and any(c.k == 1 and c.s == 2 for c in cs)
    # every id conv_tile_valid accepts (conv_igemm.hip), under every form it has; 86 / 87 refused
    valid = set(range(0, 20)) | set(range(31, 36)) | {40, 41, 42, 43, 50, 51, 60, 78} | set(range(70, 78)) | {79, 80, 81} | set(range(82, 90))
    assert {c.tile for c in run(lambda c: c.tile is not None)} == valid - {86, 87}
    assert {c.tile for c in R.REFUSED} >= {86, 87, 50, 51, 60, 78}
    for split in ("b3", "h2"):
        assert {c.tile for c in run(lambda c: c.split == split and not c.f16)} >= set(R.B3_TILES) | {41, 42, 43, 51}
        assert {c.tile for c in run(lambda c: c.split == split and c.Cin == 40)} >= set(R.B3_TILES)
    assert {c.tile for c in run(lambda c: c.f16)} == set(R.F16_TILES)
    assert {c.narrow for c in run(lambda c: c.tile is None)} == {"pixel", "strip4", "strip8"}
    assert {c.tile for c in run(lambda c: c.ksplit)} >= {0, 40, 41, 42, 43, 76}
    assert any(c.ksplit and c.mode == "deconv2x" for c in R.RUN_CASES) and any("dual" in c.epi and c.ksplit for c in R.RUN_CASES)
    # shapes: ragged against every tile height, a ragged 128-column tile, pad channels
    for c in run(lambda c: c.fam.startswith("igemm") and c.s == 1):
        assert c.N * c.Ho * c.Wo == 741 and all(741 % bm for bm in (32, 64, 128, 256))
    assert all(c.Ho % 2 == 0 and c.Wo % 2 == 0 for c in R.RUN_CASES if c.wino)


@pytest.mark.parametrize("s,p,d,k", [(1, 1, 1, 3), (2, 2, 2, 3), (2, 0, 1, 1), (2, 3, 1, 7)])
def test_conv64_is_torch_in_double(s, p, d, k):
    rng = np.random.default_rng(k + s)
    x, w = rng.standard_normal((3, 8, 13, 19)), rng.standard_normal((10, 8, k, k))
    ref = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, s, p, d).numpy()
    assert np.abs(conv64(x, w, s, p, d) - ref).max() <= 1e-12 * np.abs(ref).max()


def test_deconv64_is_torch_in_double():
    rng = np.random.default_rng(5)
    x, w = rng.standard_normal((3, 8, 6, 9)), rng.standard_normal((8, 10, 4, 4))
    ref = torch.nn.functional.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(w), None, 2, 1).numpy()
    assert ref.shape == (3, 10, 12, 18)
    assert np.abs(deconv64(x, w) - ref).max() <= 1e-12 * np.abs(ref).max()


def conv32(case, x, w):
    """the oracle's fp32 contraction of a case"""
    if case.mode == "deconv2x":
        return O.deconv2d(x, w, None, 2, 1)[:, :, :case.Ho, :case.Wo]
    if case.mode == "cols":
        return O.conv2d(x, np.ascontiguousarray(np.transpose(w, (0, 2, 3, 1))).reshape(case.Cout, 9 * case.Cin, 1, 1))
    return O.conv2d(x, w, None, case.s, case.p, case.d)


SIGNATURE = lambda c: (c.data_key, c.f16, tuple(sorted(c.epi)), c.act)


@pytest.mark.parametrize("case", _unique(R.RUN_CASES, SIGNATURE), ids=lambda c: c.id)
def test_an_fp32_evaluation_meets_the_bound(case):
    """conv_ref against oracle.ops: the convolution in fp32 (f16 mode: on operands rounded to half), scale / shift / residual /
    activation / second output in fp32 -- inside the bound WITHOUT what a split form may add, and inside the bar of the case"""
    o = R.operands(case)
    x, w = o["x"], o["w"]
    if case.f16:
        x, w = x.astype(np.float16).astype(np.float32), w.astype(np.float16).astype(np.float32)
    scale, shift, s2, b2 = R.epilogue_constants(case, o)
    bc = lambda a: a[None, :, None, None]
    v = conv32(case, x, w) * bc(scale) + bc(shift)
    if "res" in case.epi:
        v = v + o["res"]
    y = np.maximum(v, np.float32(0)) if case.act == 1 else np.where(v > 0, v, v * np.float32(R.SLOPE)) if case.act == 2 else v
    y2 = np.maximum(y * bc(s2) + bc(b2), np.float32(0)) if s2 is not None else None
    assert y.dtype == np.float32
    plain = R.Case(case.fam, None, case.Cin, case.Cout, case.H, case.W, case.N, case.k, case.s, case.p, case.d,
                   "+".join(case.epi), case.act, "", case.f16, case.mode, odd=case.odd)
    assert R.form_of(plain) == ("f16" if case.f16 else "")
    ratio = R.check(plain, y, y2)
    print("%s: fp32 evaluation at %.3f of the bound" % (case.id, ratio))
    # the reference itself: the same contraction by torch in double
    if case.mode == "conv" and not case.f16:
        t = torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64)), None, case.s, case.p, case.d).numpy()
        ref = R.reference(plain)
        want = R.act64(t * bc(scale).astype(np.float64) + bc(shift) + (o["res"] if "res" in case.epi else 0.0), case.act)
        assert np.abs(ref.y - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("case", _unique([c for c in R.RUN_CASES if c.wino], lambda c: c.data_key), ids=lambda c: c.id)
def test_winograd_in_fp32_meets_its_bar(case):
    """the fp32 restatement of F(2x2, 3x3) against float64: inside 3e-6 max|ref|; beyond K = 576 four times its error is the bar"""
    e = R.wino32_error(case)
    print("%s: wino32 at %.3g of max|ref|" % (case.id, e))
    assert e <= 3e-6
    o = R.operands(case)
    got = R.wino32(o["x"], o["w"])
    assert got.dtype == np.float32 and np.abs(got - O.conv2d(o["x"], o["w"], None, 1, 1, 1)).max() <= 3e-6 * np.abs(got).max()


def test_the_fold_of_bn_params_is_exact():
    """moving_var = 1 - eps: sqrt(var + eps) is 1 in fp32, so scale = gamma and shift = beta - gamma * mean, as the oracle folds them"""
    o = R.operands(R.RUN_CASES[1])
    for name in ("bn", "bn2"):
        scale, shift = R.bn_fold32(o[name], name, 1e-5)
        assert np.array_equal(scale, o[name][name + "_gamma"])
        s, b = O.bn_fold(o[name][name + "_gamma"], o[name][name + "_beta"], o[name][name + "_moving_mean"], o[name][name + "_moving_var"], 1e-5)
        assert np.array_equal(s, scale) and np.array_equal(b, shift)


def test_split_forms_add_little():
    """what the fp16x2 model drops stays below 2^-20 A (a few units of the 22-23 bits the form keeps) on the table's inputs"""
    for case in _unique([c for c in R.RUN_CASES if R.form_of(c) == "h2" and not c.wino], lambda c: c.data_key):
        conv, A, D = R._core(case.data_key, "h2")
        assert (D <= 2.0 ** -20 * A).all() and D.max() > 0, case.id
