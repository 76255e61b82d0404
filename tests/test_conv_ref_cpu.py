"""conv_ref.py against the oracle and torch: the float64 reference of a plan `conv` line is right, an honest fp32 evaluation of every
case of the table (the C oracle's convolution, the epilogue in numpy fp32) stays inside the bound and the bar test_conv_views_gpu.py
asserts for it, and the table covers what it says it covers.  For the geometry sweep (conv_ref.GEOMETRY: kernel size, stride, padding
and dilation as (h, w) pairs): the same on every new case, the properties the table is built for, and a matrix of loader mutants --
pairs swapped, taps transposed or decoded with the wrong divisor, replicate padding, a dropped K granule, border rows read from the
neighbouring image -- each of which some shape must put at least 100 times its own bound away from the reference.

Measured here: the fp32 restatement of Winograd F(2x2, 3x3) (conv_ref.wino32) against float64, relative to max|ref| --
K = 288 (Cin 32, 12x18): 2.0e-07; K = 576 (Cin 64, 8x8): 2.8e-07; K = 1152 (Cin 128, 8x8): 3.9e-07; K = 2304 (Cin 256, 6x8): 6.8e-07
(Cout 136) and 7.9e-07 (Cout 18) -- four times that is the deep-K bar of the GPU test where it exceeds 3e-6 (the last one: 3.15e-6)."""
import numpy as np
import pytest
import torch

import conv_ref as R
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
