"""conv_ref.py against the oracle and torch: the float64 reference of a plan `conv` line is right, an honest fp32 evaluation of every
case of the table (the C oracle's convolution, the epilogue in numpy fp32) stays inside the bound and the bar test_conv_views_gpu.py
asserts for it, and the table covers what it says it covers.  For the geometry sweep (conv_ref.GEOMETRY: kernel size, stride, padding
and dilation as (h, w) pairs): the same on every new case, the properties the table is built for, and a matrix of loader mutants --
pairs swapped, taps transposed or decoded with the wrong divisor, replicate padding, a dropped K granule, border rows read from the
neighbouring image -- each of which some shape must put at least 100 times its own bound away from the reference.

Measured here: the fp32 restatement of Winograd F(2x2, 3x3) (conv_ref.wino32) against float64, relative to max|ref| --
K = 288 (Cin 32, 12x18): 2.0e-07; K = 576 (Cin 64, 8x8): 2.8e-07; K = 1152 (Cin 128, 8x8): 3.9e-07; K = 2304 (Cin 256, 6x8): 6.8e-07
(Cout 136) and 7.9e-07 (Cout 18) -- four times that is the deep-K bar of the GPU test where it exceeds 3e-6 (the last one: 3.15e-6).

For the Winograd block sweep (conv_ref.WINO_GEOMETRY): the table has every block class, K loop, K split, swizzle branch and channel
block it is for, as conv_ref.wino_blocks / wino_split / wino_slices see them; the references agree on the Gaussian operands (wino32
there: 1.9e-07 at K = 144 to 5.1e-07 at K = 1584, and 1.08e-06 at K = 4608 -- `deep`, the one shape whose bar is four times that); on
the dyadic operands wino32 and the fp16x2 model ARE the float64 convolution and every output is an integer below 2^24; and a float64
evaluation that walks the map block by block the way the kernels do (block_walk) is the convolution, while each of ten mutants of it --
a ragged block row or column never computed, the block-shape threshold off by one, a tile past TW taken for valid, a patch column at
ix = W or a patch row outside the image read from the neighbouring memory, a linear block keeping its first tile's image, an odd last
K step dropped, a short last slice run to full length, the channel quads of a K step swapped -- is 100 bars or more away from the
reference on the shapes built for that edge and changes output words on the dyadic set."""
import collections

import numpy as np
import pytest
import torch

import conv_ref as R
import h2_model as H2
from oracle import ops as O
from plan_helpers import conv64, deconv64, pair, r4


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


@pytest.mark.parametrize("s,p,d,k", [(1, 1, 1, 3), (2, 2, 2, 3), (2, 0, 1, 1), (2, 3, 1, 7), ((1, 2), 1, 1, 3), ((2, 1), (0, 1), 1, (3, 1)),
                                     (1, (2, 0), (1, 2), (1, 3)), ((2, 1), (1, 3), (1, 2), (3, 5)), ((1, 2), (3, 1), (2, 1), (5, 3))])
def test_conv64_is_torch_in_double(s, p, d, k):
    rng = np.random.default_rng(sum(pair(k)) + sum(pair(s)))
    x, w = rng.standard_normal((3, 8, 13, 19)), rng.standard_normal((10, 8) + pair(k))
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


@pytest.mark.parametrize("case", _unique(R.RUN_CASES + R.GEOMETRY_RUN, SIGNATURE), ids=lambda c: c.id)
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
    assert R.form_of(plain) == ("f16" if case.f16 else "") and plain.data_key == case.data_key
    assert y.shape == (case.N, case.Cout, case.Ho, case.Wo)
    ratio = R.check(plain, y, y2)
    print("%s: fp32 evaluation at %.3f of the bound" % (case.id, ratio))
    # the reference itself: the same contraction by torch in double
    if case.mode == "conv" and not case.f16:
        t = torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64)), None, case.s, case.p, case.d).numpy()
        ref = R.reference(plain)
        want = R.act64(t * bc(scale).astype(np.float64) + bc(shift) + (o["res"] if "res" in case.epi else 0.0), case.act)
        assert ref.y.shape == want.shape and np.abs(ref.y - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


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
    for case in _unique([c for c in R.RUN_CASES + R.GEOMETRY_RUN if R.form_of(c) == "h2" and not c.wino], lambda c: c.data_key):
        conv, A, D = R._core(case.data_key, "h2")
        assert (D <= 2.0 ** -20 * A).all() and D.max() > 0, case.id


# ---- the geometry sweep -----------------------------------------------------------------------------------------------------------
def test_pairs_leave_the_old_cases_their_inputs():
    """an int geometry gives the data_key repr -- and so the crc32 seed -- the table had before geometry pairs (values of the
    commit before them)"""
    import zlib
    pinned = {"igemm-s0-t0-b3-n3-32x136-13x19-k3s1p1d1-act0-bias": 2688908207,
              "stem-t50-b3-n3-3x64-26x38-k7s2p3d1-act0-bias": 1667214737,
              "deconv-t0-b3-deconv2x-n3-32x18-6x9-k3s1p1d1-odd-act2-bias": 748408745}
    by_id = {c.id: c for c in R.CASES}
    for cid, seed in pinned.items():
        assert zlib.crc32(repr(by_id[cid].data_key).encode()) == seed, cid
    assert repr(by_id["igemm-s0-t0-b3-n3-32x136-13x19-k3s1p1d1-act0-bias"].data_key) == "('conv', False, 32, 136, 13, 19, 3, 3, 1, 1, 1)"
    assert len(R.CASES) == 224 and len(R.RUN_CASES) == 217      # nothing left the old table


def _shape(name, **kw):
    return R.Case("", 0, **dict(R.GEOMETRY[name], **kw))


def oor_sides(c):
    """the sides ("t", "b", "l", "r") on which some tap of some output pixel falls outside the map"""
    iy = (np.arange(c.Ho) * c.sh - c.ph)[:, None] + np.arange(c.kh) * c.dh
    ix = (np.arange(c.Wo) * c.sw - c.pw)[:, None] + np.arange(c.kw) * c.dw
    return "".join(s for s, hit in (("t", (iy < 0).any()), ("b", (iy >= c.H).any()), ("l", (ix < 0).any()), ("r", (ix >= c.W).any())) if hit)


def test_the_geometry_table_has_the_edges_it_is_for():
    shapes = {name: _shape(name) for name in R.GEOMETRY}
    pairs = lambda c: {"k": (c.kh, c.kw), "s": (c.sh, c.sw), "p": (c.ph, c.pw), "d": (c.dh, c.dw)}
    uneq = lambda c: {n for n, (h, w) in pairs(c).items() if h != w}
    # every pair with unequal members, each on its own in both orders, and all four at once on a non-square map
    alone = [shapes[n] for n in R.ANISOTROPIC[:-1]]
    assert all(len(uneq(c)) == 1 for c in alone)
    for n in "ksdp":
        got = {pairs(c)[n] for c in alone if uneq(c) == {n}}
        assert any(h < w for h, w in got) and any(h > w for h, w in got), (n, got)
    assert {pairs(c)["k"] for c in alone} >= {(1, 3), (3, 1), (1, 7), (5, 3)}
    a4 = shapes["all4"]
    assert uneq(a4) == set("kspd") and a4.H != a4.W and a4.Ho != a4.Wo
    assert all(not uneq(c) for n, c in shapes.items() if n not in R.ANISOTROPIC)
    # the networks' own geometries, maps smaller than the filter
    geo = {(c.k, c.s, c.p, c.d) for c in shapes.values()}
    assert geo >= {(7, 2, 3, 1), (5, 2, 2, 1), (3, 2, 1, 1), (1, 2, 0, 1), (3, 1, 2, 2), (3, 1, 0, 1)}
    assert shapes["net7x7s2"].Cin == 6 and shapes["net3x3s2odd"].H % 2 == 1 and shapes["net3x3s2even"].H % 2 == 0 and shapes["net3x3s2even"].W % 2 == 0
    small = {(c.H, c.W, c.k, c.s, c.p) for c in shapes.values() if c.H < c.kh or c.W < c.kw}
    assert small >= {(1, 1, 3, 1, 1), (2, 3, 3, 1, 1), (1, 19, 3, 1, 1), (4, 5, 7, 2, 3)}
    assert all(c.H <= 20 and c.W <= 24 and 1 <= c.N <= 3 for c in shapes.values())
    # out-of-range taps on all four sides, but for the shapes (and sides) EDGE_FREE names
    for n, c in shapes.items():
        assert set(oor_sides(c)) == set("tblr") - set(R.EDGE_FREE.get(n, "")), (n, oor_sides(c))
    assert set(R.EDGE_FREE) <= set(shapes) and len(R.EDGE_FREE) <= len(shapes) // 3
    # the K loop: one, two, three and odd step counts, K far below K_pad, both granule classes (padded Cin % 8 == 4: the two
    # granules of a lane's chunk of 8 lie in different taps)
    steps = {n: R.k_pad(c) // 32 for n, c in shapes.items()}
    assert steps["k1step"] == 1 and shapes["k1step"].Cin == 32 and steps["k3steps"] == 3 and shapes["k3steps"].Cin == 96
    assert {1, 2, 3} <= set(steps.values()) and any(v > 3 and v % 2 for v in steps.values()) and any(v > 3 and v % 2 == 0 for v in steps.values())
    assert (shapes["k1cin4"].K, R.k_pad(shapes["k1cin4"])) == (4, 32) and (shapes["k3x3cin4"].K, R.k_pad(shapes["k3x3cin4"])) == (36, 64)
    assert {c.Cin for c in shapes.values()} >= {4, 6, 12, 20, 36, 40, 96}
    assert {r4(c.Cin) % 8 for c in shapes.values()} == {0, 4}
    assert any(r4(c.Cin) % 8 == 4 and c.kw > 1 and c.kh > 1 for c in shapes.values())
    # the pixel tile: below one tile, exactly one and two tiles of 128, one pixel above a multiple, three images sharing tiles
    M = {n: c.N * c.Ho * c.Wo for n, c in shapes.items()}
    assert min(M.values()) < 64 and 128 in M.values() and 256 in M.values()
    assert any(m > 128 and m % 128 == 1 for m in M.values()) and any(m % 128 == 0 for m in M.values()) and any(0 < m % 128 < 127 for m in M.values())
    assert any(c.N == 3 and M[n] > 128 and (c.Ho * c.Wo) % 128 and (c.Ho * c.Wo) % 64 for n, c in shapes.items())
    # the channel tile
    assert {c.Cout for c in shapes.values()} >= {5, 33, 129, 260} and all(c.Cout > 4 for c in shapes.values())
    # the epilogue rotates: residual and dual outputs meet unequal pairs
    for epi, act in R.ROT:
        assert any(c.epi == frozenset(epi.split("+")) and c.act == act and c.kh != c.kw for c in R.GEOMETRY_RUN)
        assert any(c.epi == frozenset(epi.split("+")) and c.sh != c.sw for c in R.GEOMETRY_RUN)


def test_the_geometry_kernels_and_their_refusals():
    rows = [(t, split, f16) for _, t, split, f16, _ in R.GEOMETRY_KERNELS]
    assert len(set(rows)) == len(rows)
    assert [t for t, s, f in rows if not f and t is not None and t < 70] == [0, 5, 10, 13, 31, 16]
    assert {t for ids in R.CLASSES.values() for t in ids[:1]} == {0, 5, 10, 13, 16, 31}
    assert [(t, s) for t, s, f in rows if not f and t is not None and t >= 70] == [(70, "b3"), (75, "b3"), (76, "b3"), (77, "b3"), (80, "b3"),
                                                                                  (76, "h2"), (77, "h2"), (80, "h2")]
    assert [t for t, s, f in rows if f] == [0, 10, 76, 82, 84, 88]
    assert [(t, s) for t, s, f in rows if t is None] == [(None, "b3"), (None, "h2")]
    ids = [c.id for c in R.CASES + R.GEOMETRY_RUN + R.GEOMETRY_REFUSED + R.GEOMETRY_DEMOTED]
    assert len(set(ids)) == len(ids)
    # every shape x kernel pair is run, refused or (f16 mode on a layer it cannot take) left in fp32; at most a third is not run
    crossed = lambda cs: [c for c in cs if c.fam not in ("geo-narrow", "geo-splitk", "geo-square")]
    run, refused, demoted = crossed(R.GEOMETRY_RUN), crossed(R.GEOMETRY_REFUSED), R.GEOMETRY_DEMOTED
    assert len(run) + len(refused) + len(demoted) == len(R.GEOMETRY) * len(R.GEOMETRY_KERNELS)
    assert 3 * (len(refused) + len(demoted)) <= len(R.GEOMETRY) * len(R.GEOMETRY_KERNELS)
    print("geometry sweep: %d run (%d of the cross), %d refused (%d of the cross), %d left in fp32" % (
        len(R.GEOMETRY_RUN), len(run), len(R.GEOMETRY_REFUSED), len(refused), len(demoted)))
    assert (len(R.GEOMETRY_RUN), len(run), len(R.GEOMETRY_REFUSED), len(refused), len(demoted)) == (524, 507, 57, 50, 15)      # conv_ref's docstring
    assert all(c.raises for c in R.GEOMETRY_REFUSED) and not any(c.raises for c in R.GEOMETRY_RUN + R.GEOMETRY_DEMOTED)
    assert {c.tile for c in R.GEOMETRY_REFUSED if c.fam == "geo-square"} == {40, 50, 60, 78}
    assert all(c.kh != c.kw or c.sh != c.sw for c in R.GEOMETRY_REFUSED if c.fam == "geo-square")
    # every kernel row meets every pair with unequal members, every small map and all four epilogues
    for fam, t, split, f16, rule in R.GEOMETRY_KERNELS:
        mine = [c for c in run if (c.tile, c.split, c.f16) == (t, split, f16)]
        assert len(mine) >= len(R.GEOMETRY) // 3, (t, len(mine))
        for name, f in (("k", lambda c: c.kh != c.kw), ("s", lambda c: c.sh != c.sw), ("p", lambda c: c.ph != c.pw), ("d", lambda c: c.dh != c.dw),
                        ("small", lambda c: c.H < c.kh or c.W < c.kw), ("Cout 260", lambda c: c.Cout == 260)):
            assert any(f(c) for c in mine), (t, split, f16, name)
        assert {(tuple(sorted(c.epi)), c.act) for c in mine} == {(tuple(sorted(e.split("+"))), a) for e, a in R.ROT}
        # a rule keeps some shapes and drops others
        if rule is not None:
            assert 0 < len(mine) < len(R.GEOMETRY)
    # narrow outputs: the pixel kernel on every anisotropic shape at Cout 2 and 3; the reduce behind 0 and 76 on a deep anisotropic K
    narrow = [c for c in R.GEOMETRY_RUN if c.fam == "geo-narrow"]
    assert len(narrow) == len(R.ANISOTROPIC) and {c.Cout for c in narrow} == {2, 3} and all(c.narrow == "pixel" and c.tile is None for c in narrow)
    deep = [c for c in R.GEOMETRY_RUN if c.fam == "geo-splitk"]
    assert {(c.tile, c.split) for c in deep} == {(0, "b3"), (76, "b3"), (76, "h2")} and all(c.ksplit and c.Cin == 256 for c in deep)
    assert all(c.kh != c.kw and c.sh != c.sw and c.ph != c.pw and c.dh != c.dw for c in deep)


# ---- mutants: the loader bugs the table is for, in float64 --------------------------------------------------------------------------
def taps_conv(c, x, w, s=None, p=None, d=None, decode=None, replicate=False, wrap_rows=False, drop_last=False):
    """The contraction of case c tap by tap the way a loader decodes it -- tap t of the packed K axis sits at (t // kw, t % kw), reads
    x[oy sh - ph + ky dh, ox sw - pw + kx dw], zero outside the map -- on the case's OWN output grid (a kernel takes Ho x Wo from the
    output view), with one thing wrong: s, p, d another pair; decode: the divisor of the tap decode; replicate: the border pixel in
    place of zeros; wrap_rows: rows beyond the top / bottom of an image read on in the neighbouring image of the batch (zero only
    outside the whole batch); drop_last: the last 4-wide K granule (last tap, last channels) is left out."""
    (sh, sw), (ph, pw), (dh, dw) = pair(c.s if s is None else s), pair(c.p if p is None else p), pair(c.d if d is None else d)
    N, C, H, W = x.shape
    out = np.zeros((N, w.shape[0], c.Ho, c.Wo))
    wt = w.reshape(w.shape[0], C, c.kh * c.kw).astype(np.float64)
    rows_all = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(C, N * H, W)
    for t in range(c.kh * c.kw):
        ky, kx = divmod(t, decode or c.kw)
        iy, ix = np.arange(c.Ho) * sh - ph + ky * dh, np.arange(c.Wo) * sw - pw + kx * dw
        if replicate:
            g = x[:, :, np.clip(iy, 0, H - 1)][:, :, :, np.clip(ix, 0, W - 1)]
        else:
            okx = (ix >= 0) & (ix < W)
            if wrap_rows:
                r = np.arange(N)[:, None] * H + iy[None, :]
                oky = (r >= 0) & (r < N * H)
                g = rows_all[:, np.clip(r, 0, N * H - 1)].transpose(1, 0, 2, 3) * oky[:, None, :, None]
            else:
                g = x[:, :, np.clip(iy, 0, H - 1)] * ((iy >= 0) & (iy < H))[None, None, :, None]
            g = g[:, :, :, np.clip(ix, 0, W - 1)] * okx
        wk = wt[:, :, t].copy()
        if drop_last and t == c.kh * c.kw - 1:
            wk[:, r4(C) - 4:] = 0.0
        out += np.einsum('kc,nchw->nkhw', wk, g)
    return out


MUTANTS = {
    "ph <-> pw": (lambda c: c.ph != c.pw, lambda c, x, w: taps_conv(c, x, w, p=(c.pw, c.ph))),
    "sh <-> sw": (lambda c: c.sh != c.sw, lambda c, x, w: taps_conv(c, x, w, s=(c.sw, c.sh))),
    "dh <-> dw": (lambda c: c.dh != c.dw, lambda c, x, w: taps_conv(c, x, w, d=(c.dw, c.dh))),
    "filter taps transposed": (lambda c: c.kh == c.kw > 1, lambda c, x, w: taps_conv(c, x, np.ascontiguousarray(w.transpose(0, 1, 3, 2)))),
    "tap decode with kh for kw": (lambda c: c.kh != c.kw, lambda c, x, w: taps_conv(c, x, w, decode=c.kh)),
    "replicate padding": (lambda c: c.ph + c.pw > 0, lambda c, x, w: taps_conv(c, x, w, replicate=True)),
    "last K granule dropped": (lambda c: True, lambda c, x, w: taps_conv(c, x, w, drop_last=True)),
    "border rows read the neighbouring image": (lambda c: c.N > 1 and c.ph > 0, lambda c, x, w: taps_conv(c, x, w, wrap_rows=True)),
}


def test_the_geometry_table_kills_every_mutant():
    """every mutant is at least 100 times the case's own bound away from the reference somewhere in the output of at least one shape
    (a condition on the INPUTS: a mutant moves outputs by O(1), the bounds are near 1e-5 or below) -- and on every shape it applies to
    but the few where it changes nothing (recorded below)"""
    cases = {}
    for c in R.GEOMETRY_RUN:
        if c.fam == "geo-igemm" and c.tile == 0:
            cases[[n for n in R.GEOMETRY if R.Case("", 0, **R.GEOMETRY[n]).data_key == c.data_key][0]] = c
    assert list(cases) == list(R.GEOMETRY)
    killed = {m: [] for m in MUTANTS}
    for name, c in cases.items():
        o = R.operands(c)
        x, w = o["x"].astype(np.float64), o["w"].astype(np.float64)
        ref = R.reference(c)
        plain = taps_conv(c, x, w)
        assert np.abs(plain - conv64(x, w, c.s, c.p, c.d)).max() <= 1e-12 * np.abs(plain).max(), name      # the model without a mutation is the convolution
        for m, (applies, run) in MUTANTS.items():
            if not applies(c):
                continue
            ratio = float((np.abs(R.finish64(c, run(c, x, w)) - ref.y) / ref.bound).max())
            if ratio >= 100.0:
                killed[m].append((name, ratio))
    for m, by in killed.items():
        print("%-42s killed by %s" % (m, ", ".join("%s (%.2g x bound)" % nr for nr in by) or "NOTHING"))
        assert by, m
    # each swap is killed by the shape that has that pair alone (the failure names the pair), both orders
    for m, names in (("ph <-> pw", ("p0x1", "p2x0")), ("sh <-> sw", ("s1x2", "s2x1")), ("dh <-> dw", ("d1x2", "d2x1")),
                     ("tap decode with kh for kw", ("k1x3", "k3x1", "k1x7", "k5x3"))):
        assert set(names) <= {n for n, _ in killed[m]}, (m, killed[m])
    assert "all4" in {n for n, _ in killed["ph <-> pw"]} & {n for n, _ in killed["sh <-> sw"]} & {n for n, _ in killed["dh <-> dw"]}
    # (the last tap of a 3x3 window never lies inside a map one row high)
    assert set(R.GEOMETRY) - {n for n, _ in killed["last K granule dropped"]} == {"map1x1", "map1xW"}


# ---- the Winograd block sweep -------------------------------------------------------------------------------------------------------
WINO_SHAPES = {name: R.Case("", 0, **g) for name, g in R.WINO_GEOMETRY.items()}
WINO_GAUSS = [R.wino_case(name, "wino-geo-fp32", 40, "b3") for name in R.WINO_GEOMETRY]
WINO_DYADIC = [R.wino_case(name, "wino-geo-fp32", 40, "b3", dyadic=True) for name in R.WINO_GEOMETRY]


def raggedness(tile, c):
    """(block class, "fit" / "rows" / "cols" / "both", tiles in the last block of the map) of a rectangular form on a shape"""
    TH, TW = c.H // 2, c.W // 2
    BH, BW, per, MT = R.wino_blocks(tile, c.H, c.W, c.N)
    rr, rc = TH % BH, TW % BW
    return "%dx%d" % (BH, BW), ("both" if rr and rc else "rows" if rr else "cols" if rc else "fit"), (rr or BH) * (rc or BW)


def test_the_winograd_table_has_the_edges_it_is_for():
    shapes = WINO_SHAPES
    assert all(c.H % 2 == 0 and c.W % 2 == 0 and c.Cin % 16 == 0 and (c.k, c.s, c.p, c.d) == (3, 1, 1, 1) for c in shapes.values())
    assert len(shapes) == 13 and len(R.WINO_KERNELS) == 7 and len(R.WINO_RUN) == 182 and len({c.id for c in R.WINO_RUN}) == 182
    assert not any(c.raises for c in R.WINO_RUN) and all(c.raises for c in R.WINO_REFUSED)
    assert sum(c.dyadic for c in R.WINO_RUN) == 91 and {(c.tile, c.split) for c in R.WINO_RUN} == {(t, s) for _, t, s in R.WINO_KERNELS}
    assert [(t, s) for _, t, s in R.WINO_KERNELS] == [(40, "b3"), (41, "b3"), (42, "b3"), (43, "b3"), (41, "h2"), (42, "h2"), (43, "h2")]
    # the block classes of the rectangular forms: each fits exactly, is ragged in the rows alone, in the columns alone, and in both
    # with a corner block of ONE tile
    for tile, classes in ((42, ("8x8", "4x16", "2x32")), (43, ("4x8", "2x16"))):
        seen = collections.defaultdict(set)
        for name, c in shapes.items():
            cls, how, last = raggedness(tile, c)
            seen[cls].add(how)
            if how == "both" and last == 1:
                seen[cls].add("corner")
        assert set(seen) == set(classes), (tile, dict(seen))
        for cls in classes:
            assert seen[cls] == {"fit", "rows", "cols", "both", "corner"}, (tile, cls, seen[cls])
    # ... and both sides of every threshold of `bhs`
    assert {c.H // 2 for c in shapes.values()} >= {1, 2, 3, 4, 5, 7, 8, 9, 17}
    assert raggedness(42, shapes["strip"])[0] == "2x32" and shapes["strip"].W // 2 > 32      # a full 2x32 block: the largest raw patch copy, 6 x 66 pixels
    # linear blocks (40 / 41): T below, at and above 64 with a last block that is not full; a block in two images; a block in three tile rows
    T = {n: c.N * (c.H // 2) * (c.W // 2) for n, c in shapes.items()}
    assert min(T.values()) < 64 and 64 in T.values() and any(t > 64 and t % 64 for t in T.values())
    assert any(c.N > 1 and ((c.H // 2) * (c.W // 2)) % 64 for c in shapes.values())      # an image boundary inside a block
    assert any(2 * (c.W // 2) < 64 <= T[n] for n, c in shapes.items())                     # a full block over more than two tile rows
    assert T["strip"] == 99 and T["fit"] == 64 and T["onetile"] == 1
    # the K loop
    steps = lambda t: {c.Cin // R.wino_kstep(t) for n, c in shapes.items() if n not in R.WINO_SPLIT_SHAPES}
    assert steps(41) >= {1, 2, 3, 4, 5, 32} and steps(40) >= {2, 64}
    # the K split: for every id equal slices and a short last slice (the earlier table has the equal ones of 41-43), never a step lost
    old = [c for c in R.RUN_CASES if c.wino and c.ksplit]
    for t in R.WINO_TILES:
        slices = [R.wino_slices(t, c) for c in old if c.tile == t] + [R.wino_slices(t, R.wino_case(n, "", t, "b3")) for n in R.WINO_SPLIT_SHAPES]
        assert all(len(s) > 1 for s in slices), (t, slices)
        assert any(len(set(s)) == 1 for s in slices) and any(s[-1] < s[0] for s in slices), (t, slices)
    for c in R.WINO_RUN:
        s = R.wino_slices(c.tile, c)
        assert sum(s) * R.wino_kstep(c.tile) == c.Cin and (len(s) > 1) == c.ksplit == (c.fam == "wino-geo-splitk"), c.id
        assert c.tile != 40 or all(v % 2 == 0 for v in s)
    want = {(40, "split54"): [6, 6, 6], (41, "split54"): [5, 4], (40, "split_ragged"): [6, 6, 6, 4], (43, "split_ragged"): [6, 5], (42, "split_ragged"): [6, 5]}
    for (t, n), s in want.items():
        assert R.wino_slices(t, R.wino_case(n, "", t, "b3")) == s, (t, n)
    assert R.wino_slices(41, R.Case("", 41, Cin=128, Cout=72, H=8, W=8, N=1, ksplit=True)) == [4, 4]      # CASES: KT 8 -> 4 + 4
    assert R.wino_slices(41, R.Case("", 41, Cin=256, H=6, W=8, N=1, ksplit=True)) == [4, 4, 4, 4]          # KT 16 -> 4 x 4
    # the XCD swizzle: nblk below 8 (r8 alone), a multiple of 8 (q8 alone), above 8 and not a multiple (both)
    for t in R.WINO_TILES:
        nblk = {R.wino_blocks(t, c.H, c.W, c.N)[3] * R.wino_nt(c) for c in shapes.values()}
        assert any(v < 8 for v in nblk) and any(v % 8 == 0 for v in nblk) and any(v > 8 and v % 8 for v in nblk), (t, nblk)
    # the channel block
    assert {r4(c.Cout) for c in shapes.values()} >= {8, 64, 68, 132} and {R.wino_nt(c) for c in shapes.values()} == {1, 2, 3}
    # epilogues: all of ROT on the Gaussian set, on every kernel row; nothing that rounds on the dyadic set
    for _, t, s in R.WINO_KERNELS:
        mine = [c for c in R.WINO_RUN if (c.tile, c.split) == (t, s)]
        assert {(tuple(sorted(c.epi)), c.act) for c in mine if not c.dyadic} == {(tuple(sorted(e.split("+"))), a) for e, a in R.ROT}
        assert {(tuple(sorted(c.epi)), c.act) for c in mine if c.dyadic} == {(("bias",), 0), ((), 1), (("res",), 1), (("res",), 0)}
    assert all(c.K > 576 for c in R.WINO_RUN if c.Cin > 64) and shapes["th9w9"].K == 720
    # refusals of the family
    ref = {(c.tile, c.Cin, c.H % 2 or c.W % 2, c.p) for c in R.WINO_REFUSED}
    assert ref >= {(40, 32, 1, 1), (43, 32, 1, 1), (41, 24, 0, 1), (40, 8, 0, 1), (40, 32, 0, 0)}
    ids = [c.id for c in R.CASES + R.GEOMETRY_RUN + R.GEOMETRY_REFUSED + R.GEOMETRY_DEMOTED + R.WINO_RUN + R.WINO_REFUSED]
    assert len(set(ids)) == len(ids)


def test_the_block_model_is_the_launchers():
    """wino_blocks against the sentences of the issue it restates, spelled out by hand for a few maps"""
    assert R.wino_blocks(42, 16, 16, 2) == (8, 8, 1, 2) and R.wino_blocks(42, 14, 32, 2) == (4, 16, 2, 4) and R.wino_blocks(42, 6, 64, 2) == (2, 32, 2, 4)
    assert R.wino_blocks(43, 8, 32, 1) == (4, 8, 2, 2) and R.wino_blocks(43, 6, 64, 2) == (2, 16, 4, 8) and R.wino_blocks(43, 2, 66, 3) == (2, 16, 3, 9)
    assert R.wino_blocks(42, 18, 18, 1) == (8, 8, 4, 4) and R.wino_blocks(42, 2, 66, 3) == (2, 32, 2, 6)
    assert R.wino_blocks(40, 2, 66, 3)[2:] == (None, 2) and R.wino_blocks(41, 8, 32, 1)[2:] == (None, 1) and R.wino_blocks(41, 10, 34, 2)[3] == 3
    assert [R.wino_bhs(42, th) for th in (1, 3, 4, 7, 8, 9)] == [1, 1, 2, 2, 3, 3] and [R.wino_bhs(43, th) for th in (1, 3, 4, 5)] == [1, 1, 2, 2]
    assert [R.wino_rows(c) for c in (8, 64, 68, 128, 132)] == [64, 64, 128, 128, 192]


@pytest.mark.parametrize("case", WINO_GAUSS, ids=lambda c: c.id)
def test_winograd_sweep_references_agree(case):
    """Gaussian operand set: the float64 reference is torch's, the oracle's fp32 convolution meets the bound, wino32 its bar"""
    test_an_fp32_evaluation_meets_the_bound(case)
    test_winograd_in_fp32_meets_its_bar(case)


@pytest.mark.parametrize("name", list(R.WINO_GEOMETRY))
def test_dyadic_operands_are_exact_in_every_form(name):
    """integer x in [-DYADIC_X, DYADIC_X], w in {-8, -4, 0, 4, 8}, integer bias and residual: the fp32 restatement of F(2x2, 3x3) IS
    the convolution, so is the fp16x2 model at the scale the view's maximum gives, every output is an integer below 2^24 -- the GPU
    test may ask for the bits of the float64 reference"""
    case = R.wino_case(name, "", 40, "b3", dyadic=True)
    o = R.operands(case)
    x, w = o["x"], o["w"]
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() == R.DYADIC_X and set(np.unique(w)) == {-8.0, -4.0, 0.0, 4.0, 8.0}
    assert np.array_equal(o["res"], np.rint(o["res"])) and np.array_equal(o["bias"], np.rint(o["bias"]))
    conv, A, _ = R._core(case.data_key, "")
    assert np.array_equal(R.wino32(x, w).astype(np.float64), conv), "wino32 is not exact"
    assert np.array_equal(conv, torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64)), None, 1, 1).numpy())
    # the largest intermediate any form sees: 16 positions of |U| |V| <= A' with U = G |g| G^T, V = B^T |d| B -- bounded by 4 A
    assert 4 * A.max() + 64 + 16 < 2 ** 24
    s = H2.range_scale(H2.float_bits(np.abs(x).max()))
    assert np.array_equal(H2.conv(x, w, s, lambda a, b: conv64(a, b, 1, 1, 1)), conv), "the fp16x2 model is not exact"
    assert np.array_equal(R._core(case.data_key, "h2")[2], np.zeros_like(conv)) and np.array_equal(R._core(case.data_key, "h2")[0], conv)
    # U = G g G^T (|U| <= 1.5 x 1.5 x 8, a multiple of 4 / 4) and V = B^T d B (|V| <= 4 max|x|) are integers that fit the first term
    # of either split (11 bits in half, 8 in bf16), V at the quarter scale stays inside the half range
    assert 4 * R.DYADIC_X * s / 4 <= 2 ** 14 and 1.5 * 1.5 * 8 < 2 ** 8 and 4 * R.DYADIC_X < 2 ** 8
    for epi, act in R.DYADIC_ROT:
        c = R.Case("", 40, epi=epi, act=act, dyadic=True, **R.WINO_GEOMETRY[name])
        y = R.reference(c).y
        assert np.array_equal(y, np.rint(y)) and np.abs(y).max() < 2 ** 24 and np.array_equal(y.astype(np.float32).astype(np.float64), y)
    assert R.wino32_error(case) == 0.0


# ---- mutants of the block walk, in float64 ------------------------------------------------------------------------------------------
def block_walk(tile, c, x, w, behind, mut=None):
    """The convolution of case c the way geometry `tile` walks it (float64): the map block by block in launch order (block origin,
    the tiles of the block, tile valid iff ty < TH and tx < TW), per tile the 4x4 pixel patch at (2 ty - 1, 2 tx - 1) of image n
    (zero outside the image), its four outputs stored at pixel (n Ho + 2 ty) Wo + 2 tx of the flat output and at + 1, + Wo, + Wo + 1
    (later stores win, stores behind the output are dropped); K in slices of steps (conv_ref.wino_slices), a step = 8 or 16 channels.
    `behind`: (N, C', H, W), the channels that follow the view's in its canvas.  One thing wrong with mut:
      "BX floor", "BY floor"   the block columns / rows counted by floor (grid and decode alike): a ragged one is never computed
      "bhs"                    the kernel decodes with the threshold off by one (TH > 8 for TH >= 8 on 42, TH > 4 for TH >= 4 on 43)
                               under the grid of the right rule
      "past TW"                the tile at tx == TW of a ragged block column is valid: its outputs land in the next row
      "ix W"                   the patch column at ix == W is read (the first pixel of the next row) instead of zero
      "rows wrap"              patch rows above / below an image are read from the neighbouring image (zero outside the batch)
      "first tile's image"     a linear block takes the image index of its first tile for all its tiles
      "odd step"               the last K step of a slice is dropped when the slice has an odd number of steps (a loop unrolled by 2)
      "slice overrun"          the last slice of a split runs kt_per_split steps, into the channels behind the view
      "quad swap"              the channel quads (q, q + 2) of a K step are swapped on the pixel side"""
    N, C, H, W = x.shape
    TH, TW, K = H // 2, W // 2, w.shape[0]
    THW, T = TH * TW, N * TH * TW
    tiles = []
    if tile in (40, 41):
        for mt in range(R.wino_blocks(tile, H, W, N)[3]):
            for tg in range(mt * 64, min(mt * 64 + 64, T)):
                n = (mt * 64) // THW if mut == "first tile's image" else tg // THW
                ty, tx = divmod(tg - n * THW, TW)
                tiles.append((n, ty, tx))
    else:
        bhs = R.wino_bhs(tile, TH)
        MT = R.wino_blocks(tile, H, W, N)[3]
        if mut == "bhs":
            bhs = R.wino_bhs(tile, TH - 1) if TH > 1 else bhs
        BH = 1 << bhs
        BW = (64 if tile == 42 else 32) // BH
        BX, BY = (TW + BW - 1) // BW, (TH + BH - 1) // BH
        if mut == "BX floor":
            BX = TW // BW
        if mut == "BY floor":
            BY = TH // BH
        if mut in ("BX floor", "BY floor"):
            MT = N * BX * BY
        for mt in range(MT):
            un, rem = divmod(mt, BX * BY)
            by, bx = divmod(rem, BX)
            if un >= N:      # a block behind the batch: loads outside the buffer are zero, stores are dropped
                continue
            for tl in range(BH * BW):
                ty, tx = by * BH + tl // BW, bx * BW + tl % BW
                if ty < TH and (tx < TW or (mut == "past TW" and tx == TW)):
                    tiles.append((un, ty, tx))
    out = np.zeros((K, N * H * W))
    if not tiles:
        return out.reshape(K, N, H, W).transpose(1, 0, 2, 3)
    n, ty, tx = (np.array(v)[:, None, None] for v in zip(*tiles))
    iy, ix = 2 * ty - 1 + np.arange(4)[None, :, None], 2 * tx - 1 + np.arange(4)[None, None, :]
    row = n * H + iy
    oky = (row >= 0) & (row < N * H) if mut == "rows wrap" else (iy >= 0) & (iy < H)
    okx = (ix >= 0) & (ix <= W if mut == "ix W" else ix < W)
    flat = row * W + ix
    ok = oky & okx & (flat >= 0) & (flat < N * H * W)
    # K: the channels every step of every slice reads, pixel side and weight side
    step, slices, per = R.wino_kstep(tile), R.wino_slices(tile, c), R.wino_split(tile, c)[1]
    xc, wc = [], []
    for i, nk in enumerate(slices):
        if mut == "odd step":
            nk -= nk % 2
        if mut == "slice overrun" and len(slices) > 1 and i == len(slices) - 1:
            nk = per
        for k in range(i * per, i * per + nk):
            ch = np.arange(k * step, (k + 1) * step)
            xc.append(ch.reshape(-1, 4)[[2, 3, 0, 1]].reshape(-1) if mut == "quad swap" and step == 16 else ch)
            wc.append(ch % C)      # (steps behind the last one: whatever follows in the weight planes -- here the first steps again)
    if not xc:
        return out.reshape(K, N, H, W).transpose(1, 0, 2, 3)
    xc, wc = np.concatenate(xc), np.concatenate(wc)
    xf = np.concatenate([x, behind], 1).transpose(1, 0, 2, 3).reshape(C + behind.shape[1], N * H * W)
    P = xf[xc][:, np.where(ok, flat, 0)] * ok      # (channels, tiles, 4, 4)
    Wk = w[:, wc].reshape(K, -1)                   # (K, channels x 3 x 3)
    pix00 = ((n * H + 2 * ty) * W + 2 * tx).reshape(-1)
    vals, dst = np.zeros((K, len(tiles), 4)), np.zeros((len(tiles), 4), np.int64)
    for o, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        win = P[:, :, oy:oy + 3, ox:ox + 3].transpose(1, 0, 2, 3).reshape(len(tiles), -1)
        vals[:, :, o] = (win @ Wk.T).T
        dst[:, o] = pix00 + oy * W + ox
    vals, dst = vals.reshape(K, -1), dst.reshape(-1)      # block by block, tile by tile: a later store wins
    keep = dst < N * H * W
    out[:, dst[keep]] = vals[:, keep]
    return out.reshape(K, N, H, W).transpose(1, 0, 2, 3)


# mutant -> (the ids it applies to, the (id, shape) pairs that must be among its killers: the shape built for that edge)
WINO_MUTANTS = collections.OrderedDict([
    ("BX floor", ((42, 43), [(42, "th5w17"), (43, "th5w17"), (42, "wide"), (43, "wide"), (42, "strip"), (43, "th9w9")])),
    ("BY floor", ((42, 43), [(42, "th5w17"), (43, "th5w17"), (42, "tall"), (43, "tall"), (42, "strip"), (42, "th9w9")])),
    ("bhs", ((42, 43), [(42, "th8"), (43, "split54")])),
    ("past TW", ((42, 43), [(42, "th5w17"), (43, "th5w17"), (42, "th9w9"), (43, "wide")])),
    ("ix W", ((40, 41, 42, 43), [(40, "fit"), (41, "fit"), (42, "fit"), (43, "fit")])),
    ("rows wrap", ((40, 41, 42, 43), [(40, "th8"), (41, "th8"), (42, "th8"), (43, "th8"), (42, "strip"), (43, "strip")])),
    ("first tile's image", ((40, 41), [(40, "strip"), (41, "strip"), (41, "th5w17")])),
    ("odd step", ((41, 42, 43), [(41, "th3w32"), (42, "th3w32"), (43, "th3w32"), (42, "th9w9"), (43, "onetile"), (41, "split54")])),
    ("slice overrun", ((40, 41, 42, 43), [(40, "split_ragged"), (41, "split_ragged"), (42, "split_ragged"), (43, "split_ragged"), (42, "split54")])),
    ("quad swap", ((41, 42, 43), [(41, "onetile"), (42, "onetile"), (43, "onetile")])),
])


def test_the_winograd_table_kills_every_mutant():
    """every mutant of the block walk lies at least 100 bars away from the reference on the shape built for its edge (Gaussian set),
    and changes at least one output word on the dyadic set; the walk without a mutation is the convolution on every shape and id"""
    killed = {m: [] for m in WINO_MUTANTS}
    unchanged = {m: [] for m in WINO_MUTANTS}
    dyadic_killed = {m: set() for m in WINO_MUTANTS}
    for dyadic, cases in ((False, WINO_GAUSS), (True, WINO_DYADIC)):
        for name, c0 in zip(R.WINO_GEOMETRY, cases):
            o = R.operands(c0)
            x, w = o["x"].astype(np.float64), o["w"].astype(np.float64)
            rng = np.random.default_rng(c0.Cin + c0.H)
            behind = np.rint(rng.uniform(-4, 4, (c0.N, 6 * 16, c0.H, c0.W))) if dyadic else rng.standard_normal((c0.N, 6 * 16, c0.H, c0.W))
            ref = R.reference(c0)
            conv = R._core(c0.data_key, "")[0]
            for t in R.WINO_TILES:
                c = R.wino_case(name, "", t, "b3", dyadic)
                assert c.data_key == c0.data_key
                b = R.bar(c, ref)(float(np.abs(ref.y).max()))
                plain = block_walk(t, c, x, w, behind)
                assert np.abs(plain - conv).max() <= 1e-12 * np.abs(conv).max(), (name, t)
                assert not dyadic or np.array_equal(plain, conv)
                for m, (tiles, _) in WINO_MUTANTS.items():
                    if t not in tiles:
                        continue
                    walked = block_walk(t, c, x, w, behind, m)
                    y = R.finish64(c0, walked)
                    if dyadic:
                        if not np.array_equal(y.astype(np.float32), ref.y.astype(np.float32)):
                            dyadic_killed[m].add((t, name))
                        continue
                    ratio = float(np.abs(y - ref.y).max()) / b
                    if ratio >= 100.0:
                        killed[m].append((t, name, ratio))
                    elif np.array_equal(walked, plain):
                        unchanged[m].append((t, name))
                    else:
                        raise AssertionError("%s on %d / %s: %.3g bars from the reference -- neither killed nor unchanged" % (m, t, name, ratio))
    for m, (tiles, named) in WINO_MUTANTS.items():
        print("%-20s killed by %s" % (m, ", ".join("%d/%s (%.2g bars)" % k for k in killed[m]) or "NOTHING"))
        print("%-20s changes nothing on %s" % ("", ", ".join("%d/%s" % k for k in unchanged[m]) or "no shape"))
        got = {(t, n) for t, n, _ in killed[m]}
        assert set(named) <= got, (m, sorted(set(named) - got))
        assert set(named) <= dyadic_killed[m] and dyadic_killed[m] == got, (m, sorted(got ^ dyadic_killed[m]))
    # where a mutant changes nothing, that is the geometry's doing: exact-fit maps for the ragged-edge mutants, one image for the
    # image mutants, an even number of steps, no split or equal slices
    assert all(raggedness(t, WINO_SHAPES[n])[1] in ("fit", "rows") for t, n in unchanged["BX floor"] + unchanged["past TW"])
    assert all(raggedness(t, WINO_SHAPES[n])[1] in ("fit", "cols") for t, n in unchanged["BY floor"])
    assert all(WINO_SHAPES[n].N == 1 for t, n in unchanged["rows wrap"])
    assert all(len(set(R.wino_slices(t, R.wino_case(n, "", t, "b3")))) == 1 for t, n in unchanged["slice overrun"])      # one slice, or equal ones
    assert all(not any(v % 2 for v in R.wino_slices(t, R.wino_case(n, "", t, "b3"))) for t, n in unchanged["odd step"])
    assert not unchanged["quad swap"] and not unchanged["ix W"]
