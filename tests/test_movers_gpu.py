"""The bandwidth-bound kernels (csrc/misc.hip) one op at a time against float64 (movers_ref.py), in the modes the lowered plans use:
batches, operands that are channel sub-views of wider buffers (each with its own stride), second outputs, every kernel the
launchers choose between.  Plans are hand-written (plan_helpers.Builder) with `option tune=0`.

Inputs and outputs are sub-views of canvases the host writes and reads raw.  Every output canvas is filled with distinct non-zero
words before a run; afterwards every word outside the view's channels (rounded up to 4) must still hold its canary.  Every plan runs
captured and eagerly with identical bits.  Dyadic inputs (features on multiples of 1/4, flows and offsets of 1/8, warp sizes with
H - 1 and W - 1 powers of two) make every intermediate exact in fp32, contracted or not: those cases have no tolerance.  The others
carry the bound their operation count gives; test_movers_ref_cpu.py holds the oracle to the same bounds on the same inputs."""
import numpy as np
import pytest

import movers_ref as R
from accel_amd import runtime
from movers_ref import U
from plan_helpers import Builder, V, pair, r4

pytestmark = pytest.mark.gpu


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)


def run(ctx, b, params, feeds, outs, arena=False, check=None):
    """bind b's plan, write the input canvases, then twice (graph replay, eager issue): canary into the output canvases, run, read
    them back raw.  Both issues must give the same bits.  Returns {canvas: (words (N, H, W, Cs), tail)} (and "A": the arena)."""
    m = runtime.Model(ctx)
    try:
        m.set_params(params)
        plan = m.add_plan("p", b.text())
        plan.finalize()
        for name, data in feeds.items():
            b.write_canvas(m, name, data)
        got = []
        for issue in (plan.run, plan.run_serial):
            for name in outs:
                b.write_canvas(m, name)
            issue()
            r = {name: b.read_canvas(m, name) for name in outs}
            if arena:
                r["A"] = plan.arena().copy()
            got.append(r)
        for name, first in got[0].items():
            pairs = [(first, got[1][name])] if name == "A" else zip(first, got[1][name])
            assert all(np.array_equal(x, y) for x, y in pairs), "graph replay and eager issue differ in " + name
        if check:
            check(m)
        return got[0]
    finally:
        m.close()


def view_of(b, res, name, v):
    """the values of view v of output canvas `name`, after the canary check of everything around it"""
    words, tail = res[name]
    assert b.untouched(name, words, tail, v.c0, v.C), "words outside the view of %s were written" % name
    return f32(words[..., v.c0:v.c0 + v.C])


def filled(rng_seed, b, name):
    """input canvases are random everywhere: what a kernel reads beyond its view is never zero by luck"""
    N, H, W, Cs, _ = b.canvases[name]
    return R.gauss(rng_seed, N, H, W, Cs)


def put(canvas, v, data):
    canvas[..., v.c0:v.c0 + data.shape[-1]] = data
    return canvas


# ---- warp -------------------------------------------------------------------------------------------------------------------------
def warp_plan(H, W, C, second, N=3):
    b = Builder(N)
    feat = b.canvas("F", C + 8, H, W).sub(4, C)
    flow = b.canvas("FL", 8, H, W).sub(4, 2)
    out = b.canvas("O", C + 12, H, W).sub(8, C)
    out2 = b.canvas("O2", C + 16, H, W).sub(12, C) if second else None
    b.warp("w", feat, flow, out, out2, "wb")
    return b, feat, flow, out, out2


def run_warp(ctx, feat_v, flow_v, bias, H, W, C, second):
    b, feat, flow, out, out2 = warp_plan(H, W, C, second)
    feeds = {"F": put(filled(1, b, "F"), feat, feat_v), "FL": put(filled(2, b, "FL"), flow, flow_v)}
    res = run(ctx, b, {"wb": bias}, feeds, ["O", "O2"] if second else ["O"])
    return view_of(b, res, "O", out), (view_of(b, res, "O2", out2) if second else None)


@pytest.mark.parametrize("second", [False, True], ids=["out", "out2"])
@pytest.mark.parametrize("C", R.WARP_EXACT_C)
@pytest.mark.parametrize("H,W", R.WARP_EXACT_SIZES)
def test_warp_exact(ctx, H, W, C, second):
    """dyadic inputs: bit for bit the float64 value, at every discontinuity (sampling positions exactly on -1, 0, W - 1, W and beyond
    every side), three different images, every operand a strided sub-view; out2 = relu(out + bias) at a dyadic bias as well"""
    feat, flow, bias = R.warp_exact_inputs(H, W, C)
    ref = R.warp64(feat, flow)
    got, got2 = run_warp(ctx, feat, flow, bias, H, W, C, second)
    np.testing.assert_array_equal(got, ref)
    if second:
        np.testing.assert_array_equal(got2, np.maximum(ref + bias, 0.0))


@pytest.mark.parametrize("H,W,mag", R.WARP_BOUNDED)
def test_warp_bounded(ctx, H, W, mag):
    """Gaussian data at general sizes: a continuous piecewise bilinear function (slope <= 2 max|feat| per axis) of a coordinate that
    carries a few fp32 roundings at magnitude max(|x + fx|, W - 1): 2^-24 (max(|x + fx|, W - 1) + max(|y + fy|, H - 1)) 2 max|feat|
    + 2^-22 max|feat| per output, border pixels included; out2 adds the rounding of out + bias"""
    C = 20
    feat, flow, bias = R.warp_bounded_inputs(H, W, mag, C)
    ref, bound = R.warp64(feat, flow), R.warp_bound(feat, flow)
    got, got2 = run_warp(ctx, feat, flow, bias, H, W, C, True)
    r1 = np.abs(got - ref) / bound
    ref2 = np.maximum(ref + bias, 0.0)
    r2 = np.abs(got2 - ref2) / (bound + U * np.abs(ref + bias))
    print("warp %dx%d flow scale %g: out at %.3f of the bound, out2 at %.3f" % (H, W, mag, r1.max(), r2.max()))
    assert r1.max() <= 1.0, (np.unravel_index(np.argmax(r1), r1.shape), r1.max())
    assert r2.max() <= 1.0, (np.unravel_index(np.argmax(r2), r2.shape), r2.max())


# ---- dcn_cols ---------------------------------------------------------------------------------------------------------------------
def dcn_plan(k, s, p, d, dg, C, H, W, N, half=False):
    b = Builder(N)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    taps, Ho, Wo = kh * kw, R.conv_out(H, kh, sh, ph, dh), R.conv_out(W, kw, sw, pw, dw)
    x = b.canvas("X", C + 8, H, W).sub(4, C)
    off = b.canvas("OFF", r4(dg * 2 * taps) + 12, Ho, Wo).sub(8, dg * 2 * taps)
    if not half:
        cols = b.canvas("COL", taps * C + 8, Ho, Wo).sub(4, taps * C)
    else:
        # a half view lives in the arena, which the host cannot write: its canary arrives through a copy (whole buffers, fp32 words)
        b.options.append("dtype=f16")
        CsH = taps * C + 16
        a = b.buf(CsH // 2, Ho, Wo)
        b.copy("canary", b.canvas("K", CsH // 2, Ho, Wo), a)
        cols = V(a.off + 2 * 8, taps * C, CsH, Ho, Wo, N, half=True)
    b.dcn_cols("d", x, off, cols, k, s, p, d, dg)
    return b, x, off, cols


DCN_IDS = lambda c: "k%ds%dp%dd%ddg%d_c%d_%dx%d" % c[:8]


@pytest.mark.parametrize("case", R.DCN_CASES, ids=DCN_IDS)
def test_dcn_cols_exact(ctx, case):
    """dyadic inputs, whole-number and fractional offsets in [-2, 2]: the column buffer [pixel][tap][c] bit for bit, with at least 8
    taps of the case in every branch of the rule (outside on each side, exactly on row / column 0, clamped in h / in w, interior);
    3x3 windows at 1, 2, 7, 8, 9 and 13 blocks per kernel row of the XCD swizzle, 1x1 and 5x5 windows in the one-tap kernel"""
    k, s, p, d, dg, C, H, W, _ = case
    x_v, off_v = R.dcn_inputs(case)
    ref, _, rec = R.dcn_cols64(x_v, off_v, k, s, p, d, dg)
    for what, n in R.branch_counts(rec).items():
        assert n >= R.DCN_MIN_TAPS, (what, n)
    if k == 3:
        assert R.dcn_blocks(case) == R.DCN_BLOCKS[R.DCN_CASES.index(case)]
    b, x, off, cols = dcn_plan(k, s, p, d, dg, C, H, W, 3)
    res = run(ctx, b, {}, {"X": put(filled(3, b, "X"), x, x_v), "OFF": put(filled(4, b, "OFF"), off, off_v)}, ["COL"])
    np.testing.assert_array_equal(view_of(b, res, "COL", cols).reshape(ref.shape), ref)


@pytest.mark.parametrize("case", R.DCN_PAIR_CASES, ids=lambda c: "k%dx%ds%dx%dp%dx%dd%dx%ddg%d_c%d_%dx%d" % (
    pair(c[0]) + pair(c[1]) + pair(c[2]) + pair(c[3]) + tuple(c[4:8])))
def test_dcn_cols_exact_with_unequal_pairs(ctx, case):
    """1x3 and 3x1 windows, dilation (1, 2), padding (0, 2), one and two deformable groups, dyadic inputs: bit for bit, every branch
    of the rule taken.  The plan reports no kernel for a mover; launch_dcn_cols (misc.hip) takes the three-taps-per-thread kernel
    only `if (p.kh == 3 && p.kw == 3)`, so these run dcn_cols_kernel: tap t = i kw + j, offsets at g 2 taps + 2 t."""
    k, s, p, d, dg, C, H, W, _ = case
    assert pair(k) != (3, 3) and pair(k)[0] != pair(k)[1] and pair(p)[0] != pair(p)[1] and pair(d)[0] != pair(d)[1]
    x_v, off_v = R.dcn_inputs(case)
    ref, _, rec = R.dcn_cols64(x_v, off_v, k, s, p, d, dg)
    for what, n in R.branch_counts(rec).items():
        assert n >= R.DCN_MIN_TAPS, (what, n)
    b, x, off, cols = dcn_plan(k, s, p, d, dg, C, H, W, 3)
    res = run(ctx, b, {}, {"X": put(filled(3, b, "X"), x, x_v), "OFF": put(filled(4, b, "OFF"), off, off_v)}, ["COL"])
    np.testing.assert_array_equal(view_of(b, res, "COL", cols).reshape(ref.shape), ref)


@pytest.mark.parametrize("case", [c for c in R.DCN_CASES if c[0] == 3], ids=DCN_IDS)
def test_dcn_cols_half_columns(ctx, case):
    """the same 3x3 cases with the column view stored as half (f16-mode plans): the exact value rounded to nearest even"""
    k, s, p, d, dg, C, H, W, _ = case
    x_v, off_v = R.dcn_inputs(case)
    ref = R.dcn_cols64(x_v, off_v, k, s, p, d, dg)[0]
    b, x, off, cols = dcn_plan(k, s, p, d, dg, C, H, W, 3, half=True)
    res = run(ctx, b, {}, {"X": put(filled(3, b, "X"), x, x_v), "OFF": put(filled(4, b, "OFF"), off, off_v), "K": None}, [], arena=True)
    N, Ho, Wo = ref.shape[:3]
    first = cols.off - 16
    got = res["A"][first:first + N * Ho * Wo * cols.Cs * 2].view(np.uint16).reshape(N, Ho, Wo, cols.Cs)
    want = b.canary("K")[:N * Ho * Wo * cols.Cs // 2].view(np.uint16).reshape(N, Ho, Wo, cols.Cs)
    assert np.array_equal(got[..., :8], want[..., :8]) and np.array_equal(got[..., 8 + cols.C:], want[..., 8 + cols.C:])
    np.testing.assert_array_equal(np.ascontiguousarray(got[..., 8:8 + cols.C]).view(np.float16).reshape(ref.shape), ref.astype(np.float16))


def test_dcn_cols_bounded(ctx):
    """Gaussian features, dyadic offsets (exact weights): four products and three sums, at most four roundings on one term"""
    case = R.DCN_CASES[3]
    k, s, p, d, dg, C, H, W, _ = case
    x_v, off_v = R.dcn_inputs(case, gaussian=True)
    ref, S, _ = R.dcn_cols64(x_v, off_v, k, s, p, d, dg)
    b, x, off, cols = dcn_plan(k, s, p, d, dg, C, H, W, 3)
    res = run(ctx, b, {}, {"X": put(filled(3, b, "X"), x, x_v), "OFF": put(filled(4, b, "OFF"), off, off_v)}, ["COL"])
    got = view_of(b, res, "COL", cols).reshape(ref.shape)
    assert (np.abs(got - ref) <= 4 * U * S).all()


def test_dcn_cols_streaming_stores(ctx):
    """the instantiation launch_dcn_cols takes for a column buffer beyond 256 MB, at the smallest shape that reaches it (302 MB):
    every tap of one channel in every 16 bit for bit, the canary around every pixel's columns"""
    c = R.BIG_DCN
    k, s, p, d, dg, C, H, W = (c[n] for n in ("k", "s", "p", "d", "dg", "C", "H", "W"))
    x_v, off_v = R.big_dcn_inputs()
    ch = R.BIG_DCN_CHANNELS
    ref = R.dcn_cols64(x_v[..., ch], off_v, k, s, p, d, dg, grp=ch // (C // dg))[0]
    b, x, off, cols = dcn_plan(k, s, p, d, dg, C, H, W, 1)
    assert H * W * (9 * C + 8) * 4 > 256 << 20
    res = run(ctx, b, {}, {"X": put(filled(3, b, "X"), x, x_v), "OFF": put(filled(4, b, "OFF"), off, off_v)}, ["COL"])
    got = view_of(b, res, "COL", cols).reshape(1, H, W, 9, C)
    np.testing.assert_array_equal(got[..., ch], ref)


# ---- copy, pools ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [24, 18])
def test_copy_between_sub_views(ctx, C):
    """three images, source and destination with different strides and offsets; an 18-channel view moves 20 (the pad may be written)"""
    b = Builder(3)
    H, W = 7, 11
    src = b.canvas("S", r4(C) + 8, H, W).sub(4, C)
    dst = b.canvas("D", r4(C) + 12, H, W).sub(8, C)
    b.copy("c", src, dst)
    s = filled(5, b, "S")
    res = run(ctx, b, {}, {"S": s}, ["D"])
    np.testing.assert_array_equal(view_of(b, res, "D", dst), s[..., 4:4 + C])


def pool_plan(C, k, s, p, full, kind, bn=None, fixg=0):
    b = Builder(3)
    H, W = R.POOL_HW
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(s), pair(p)
    x = b.canvas("X", r4(C) + 8, H, W).sub(4, C)
    y = b.canvas("Y", r4(C) + 12, R.pool_out(H, kh, sh, ph, full), R.pool_out(W, kw, sw, pw, full)).sub(8, C)
    b.pool("q", x, y, kind, k, s, p, bn=bn, fixg=fixg, act=1 if bn else 0)
    return b, x, y


def bn_params(name, bn):
    return {name + "_gamma": bn["gamma"], name + "_beta": bn["beta"], name + "_moving_mean": bn["mean"], name + "_moving_var": bn["var"]}


@pytest.mark.parametrize("C", R.POOL_C)
@pytest.mark.parametrize("kind,k,s,p,full", R.POOL_MAX_CASES, ids=["3x3s2_full", "3x3s2_valid", "2x2s2"])
def test_max_pool_exact(ctx, kind, k, s, p, full, C):
    """a maximum is exact: three images, strided views, a channel count off the quad (13 x 19: clipped windows on every side)"""
    x_v = R.pool_inputs(C)
    b, x, y = pool_plan(C, k, s, p, full, kind)
    res = run(ctx, b, {}, {"X": put(filled(6, b, "X"), x, x_v)}, ["Y"])
    np.testing.assert_array_equal(view_of(b, res, "Y", y), R.pool64(x_v, kind, k, s, p, full)[0])


@pytest.mark.parametrize("C", R.POOL_C)
@pytest.mark.parametrize("kind,k,s,p,full", R.POOL_PAIR_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pool_with_unequal_pairs(ctx, kind, k, s, p, full, C):
    """3x2 / (2, 1) / (1, 0) windows and the reverse on dyadic inputs: a maximum is exact; an average is an exact sum and ONE
    division (exact where the window's clipped area is a power of two, correctly rounded elsewhere: half an ulp).  The plan reports
    no kernel for a mover; launch_pool (misc.hip) takes the nine-loads kernel only `if (p.is_max && p.kh == 3 && p.kw == 3 &&
    p.sh == 2 && p.sw == 2)`, so these run pool_kernel."""
    assert k[0] != k[1] and s[0] != s[1] and p[0] != p[1]
    x_v = R.pool_dyadic_inputs(C)
    ref, S = R.pool64(x_v, kind, k, s, p, full)
    b, x, y = pool_plan(C, k, s, p, full, kind)
    res = run(ctx, b, {}, {"X": put(filled(6, b, "X"), x, x_v)}, ["Y"])
    got = view_of(b, res, "Y", y)
    if kind == "max":
        np.testing.assert_array_equal(got, ref)
    else:
        exact = ref.astype(np.float32) == ref
        assert exact.any() and not exact.all()
        np.testing.assert_array_equal(got[exact], ref[exact])
        assert (np.abs(got - ref) <= U * np.abs(ref)).all()


@pytest.mark.parametrize("C", R.POOL_C)
def test_avg_pool_bounded(ctx, C):
    """avg 2x2/2 `full` on odd sizes (windows of 4, 2 and 1 elements): three sums and the division"""
    x_v = R.pool_inputs(C)
    ref, S = R.pool64(x_v, "avg", 2, 2, 0, True)
    b, x, y = pool_plan(C, 2, 2, 0, True, "avg")
    res = run(ctx, b, {}, {"X": put(filled(6, b, "X"), x, x_v)}, ["Y"])
    assert (np.abs(view_of(b, res, "Y", y) - ref) <= 5 * U * S).all()


@pytest.mark.parametrize("fixg", [0, 1])
@pytest.mark.parametrize("C", R.POOL_C)
@pytest.mark.parametrize("kind,k,s,p,full", R.POOL_MAX_CASES[1:], ids=["3x3s2_valid", "2x2s2"])
def test_pool_bn_relu_bounded(ctx, kind, k, s, p, full, C, fixg):
    """the BatchNorm + ReLU epilogue of both pool kernels: scale = g / sqrt(var + eps) (three roundings), shift = beta - g mean / sd
    (five with sd's), then v scale + shift: at most 8 roundings on |v scale| + |beta| + |mean scale|"""
    x_v, bn = R.pool_inputs(C), R.bn_inputs(C)
    v = R.pool64(x_v, kind, k, s, p, full)[0]
    ref, S = R.bn_apply64(v, bn["gamma"], bn["beta"], bn["mean"], bn["var"], 2e-5, fixg, True)
    b, x, y = pool_plan(C, k, s, p, full, kind, bn="pbn", fixg=fixg)
    res = run(ctx, b, bn_params("pbn", bn), {"X": put(filled(6, b, "X"), x, x_v)}, ["Y"])
    got = view_of(b, res, "Y", y)
    assert (np.abs(got - ref) <= 8 * U * S).all()
    assert (got >= 0).all() and (got == 0).any() and (got > 0).any()


# ---- image inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "bn", "bn_fixed_gamma"])
def test_prep_rgb(ctx, mode):
    """three NCHW images -> NHWC4 (299 pixels each: a ragged second block), plain (a copy: exact, fourth channel zero) and through
    bn_data (the bound of the BatchNorm epilogue)"""
    H, W = R.PREP_RGB_HW
    img, _ = R.image_inputs(H, W)
    bn = R.bn_inputs(3)
    fixg = int(mode == "bn_fixed_gamma")
    b = Builder(3)
    b.flat("img", 3 * 3 * H * W)
    dst = b.canvas("D", 4, H, W)
    b.prep_rgb("pr", "img", dst, H, W, bn=None if mode == "plain" else "dbn", fixg=fixg)
    res = run(ctx, b, bn_params("dbn", bn), {"img": img}, ["D"])
    got = view_of(b, res, "D", dst)
    ref, S = R.prep_rgb64(img, None if mode == "plain" else (bn["gamma"], bn["beta"], bn["mean"], bn["var"], 2e-5, fixg))
    if mode == "plain":
        np.testing.assert_array_equal(got, ref)
    else:
        assert (np.abs(got - ref) <= 8 * U * S).all()
        assert not got[..., 3].any()


def test_prep_flow(ctx):
    """three image pairs -> Concat(cur / 255, prev / 255) pooled 2x2 as NHWC8 (323 outputs each): four divisions, three sums and the
    division by 4 -- 8 roundings of sum |v| / 1020; channels 6 and 7 zero"""
    H, W = R.PREP_FLOW_HW
    cur, prev = R.image_inputs(H, W, seed=7)
    b = Builder(3)
    b.flat("cur", 3 * 3 * H * W)
    b.flat("prev", 3 * 3 * H * W)
    dst = b.canvas("D", 8, H // 2, W // 2)
    b.prep_flow("pf", "cur", "prev", dst, H, W)
    res = run(ctx, b, {}, {"cur": cur, "prev": prev}, ["D"])
    got = view_of(b, res, "D", dst)
    ref, S = R.prep_flow64(cur, prev)
    assert (np.abs(got - ref) <= 8 * U * S).all()
    assert not got[..., 6:].any()


# ---- score tail -------------------------------------------------------------------------------------------------------------------
def run_tail(ctx, name):
    """the plan of one TAIL_CASES entry: (logits or probabilities (N, ncls, H, W), labels (N, H, W), its inputs)"""
    ncls, N, (Hs, Ws), right, uniform, opts = R.ALL_TAIL[name]
    d = R.tail_inputs(name)
    H, W = 16 * Hs, 16 * Ws
    b = Builder(N)
    left = b.canvas("L", r4(ncls) + 8, Hs, Ws).sub(4, ncls)
    rv = b.canvas("RT", r4(ncls) + 16, right[0], right[1]).sub(8, ncls) if right else None
    b.flat("lg", N * ncls * H * W)
    b.flat("lb", N * H * W // 4)
    b.score_tail("t", left, "lg", "lb", ncls, "wl", rv, "wr", "cw", "cb", extra=opts)
    feeds = {"L": put(filled(7, b, "L"), left, d["left"])}
    if right:
        feeds["RT"] = put(filled(8, b, "RT"), rv, d["right"])
    lowres = uniform and "lowres=0" not in opts and (right is None or right == (Hs, Ws))

    def check(m):       # the score-resolution path leaves its map in the model's `scores` buffer; the general kernel has none
        assert m.has_buffer("scores") == lowres

    res = run(ctx, b, {k: v for k, v in d.items() if k not in ("left", "right")}, feeds, ["lg", "lb"], check=check)
    for nm in ("lg", "lb"):
        assert b.untouched(nm, res[nm][0], res[nm][1], 0, b.canvases[nm][3]), nm
    return f32(res["lg"][0]).reshape(N, ncls, H, W), np.ascontiguousarray(res["lb"][0]).view(np.uint8).reshape(N, H, W), d


def check_tail_values(name, got, ref, bound):
    """logits within their bound; with softmax=1 the probabilities: a logit error of B moves p by the factor e^(2B) at the most (its
    own logit and the normaliser), expf, the subtraction, ncls sums and the division add ncls + 8 roundings, results below the
    normal range may be flushed; rows sum to 1 within ncls + 2 roundings"""
    ncls = got.shape[1]
    if "softmax" in R.ALL_TAIL[name][5]:
        p_ref, B = R.softmax64(ref), bound.max(axis=1, keepdims=True)
        lim = p_ref * (2 * B + (ncls + 8) * U) + 2.0 ** -126
        print("score tail %s: probabilities at %.3f of the bound" % (name, (np.abs(got - p_ref) / lim).max()))
        assert (np.abs(got - p_ref) <= lim).all()
        assert (np.abs(got.astype(np.float64).sum(axis=1) - 1) <= (ncls + 2) * U).all()
    else:
        print("score tail %s: logits at %.3f of the bound" % (name, (np.abs(got - ref) / bound).max()))
        assert (np.abs(got - ref) <= bound).all()


@pytest.mark.parametrize("name", sorted(R.TAIL_CASES))
def test_score_tail(ctx, name):
    """Deconvolution 32x32/16 + Crop(8, 8) of one or two score maps (strided sub-views, different strides), the 1x1 correction and
    its bias, optional softmax, labels: |logit - ref| <= (2 ncls + 8) 2^-24 S with S = |cb| + sum |cw| sum |w s| -- at most
    2 ncls + 5 roundings on any term whether the correction runs after the upsampling (score_tail_kernel) or before it at score
    resolution (score_fuse_lowres_kernel + score_tail_uniform_kernel).  Labels are the first maximum of the kernel's own output and
    the reference's label wherever its top-2 margin exceeds twice the bound (>= 90 % of the pixels)."""
    ncls, N = R.TAIL_CASES[name][:2]
    got, labels, d = run_tail(ctx, name)
    ref, S = R.tail64(**d)
    bound = R.tail_bound(ncls, S)
    check_tail_values(name, got, ref, bound)
    np.testing.assert_array_equal(labels, R.argmax_first(got))
    srt = np.sort(ref, axis=1)
    sure = (srt[:, -1] - srt[:, -2]) > 2 * bound.max(axis=1)
    assert sure.mean() >= 0.9
    np.testing.assert_array_equal(labels[sure], R.argmax_first(ref)[sure])
    for n in range(N):
        assert len(np.unique(labels[n])) >= 2


@pytest.mark.parametrize("name", sorted(R.TIE_CASES))
def test_score_tail_ties_take_the_first_class(ctx, name):
    """two classes with identical arithmetic (same scores and filter, or same correction row and bias) and the largest logits: the
    label is the first of them, in both kernels"""
    got, labels, d = run_tail(ctx, name)
    ref, S = R.tail64(**d)
    check_tail_values(name, got, ref, R.tail_bound(got.shape[1], S))
    a, c = R.TIE_CLASSES
    assert np.array_equal(got[:, a], got[:, c])
    assert ((got.max(axis=1) == got[:, a]).sum(axis=(1, 2)) >= 100).all()      # ... of every image
    np.testing.assert_array_equal(labels, R.argmax_first(got))
    assert (labels == a).sum() >= 300 and not (labels == c).any()
