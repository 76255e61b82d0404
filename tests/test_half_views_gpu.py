"""One f16-mode convolution with HALF views at a time, bit for bit: the six XH instantiations of conv_b3d_kernel (tiles 82, 83, 84, 85,
88, 89), conv_epilogue_h, the half branches of splitk_reduce_kernel and the host side of half views (tap table, extents, the :h tag,
finalize_conv's rules), on channel sub-views of wider buffers -- half_ref.CASES: the ten combinations of half / fp32 x, half / fp32 / no
residual and half / fp32 y on every tile, the edges of the K loop and of the tiles, Cout 8 / 18 / 129 / 260, split K, the column GEMM on
a half column buffer and the deconvolution with half views (test_f16_storage_gpu.py holds chains of such layers to a statistical
criterion, on dense views).

The host cannot write half views, so every half buffer of a plan is filled over its WHOLE width, and one image beyond the view, by a
producer of the same plan: an f16-mode 1x1 convolution with identity weights from an fp32 canvas (half_ref.half_buffer); a buffer
that will hold a half output is filled the same way with a pattern.  The arena is read raw afterwards.  fp32 operands are sub-views
of canvases as in test_conv_views_gpu.py.  Each plan is issued as a graph and eagerly:

 1. both issues leave identical bytes in the arena and in every canvas;
 2. every element of the output buffer outside channels [c0, c0 + r4(Cout)) of the view's pixels still holds what was there -- the
    image behind the view and an fp32 canvas's tail included; a half buffer its fill pattern, an fp32 canvas its canary;
 3. the pad channels [Cout, r4(Cout)) hold +0;
 4. every input reads back as written: canvases, and half buffers as the half bits of their canvas (the producers -- fp32 in, half
    out, a half-exact value stored exactly -- are code under test too, and a fault of theirs is reported as one);
 5. values: exact cases (dyadic operands: the store to half is the only rounding) bit for bit against np.float16(float64 value),
    signs of zero, ties, infinities from 65520 on and subnormals included; bounded cases inside the bound of conv_ref.py with D = 0
    (fp32 output) or inside [h(ref - b), h(ref + b)] (half output: every element, no cap);
 6. a second plan of the same shape whose producers add a NaN on every channel outside the input views and hold NaN in the whole
    image behind them, its fp32 canvases poisoned as in test_conv_views_gpu.py, leaves the same bits in the outputs;
 7. ops() reports the forced tile (none forced: one of the six), mode 1, and a split over K exactly where the case says.

What finalize_conv and the launcher rule out is refused with AccelError: Cs % 8, an offset that is no multiple of 16 bytes, a half view
in a persistent buffer, Cin 24, a second output, a forced tile outside the six.

Every bounded test with an fp32 output prints its largest error-to-bound ratio (run with -s), the last test the largest per family.
One run on an MI355X: bounded (base shape, tiles 84 and 89) 0.006, bounded-cols 0.004; all 146 tests of the file passed -- subnormal
inputs and outputs are kept by the device as the oracle's numpy rounding keeps them -- and the whole file took 2.3 s."""
import collections

import numpy as np
import pytest

import half_ref as HR
from accel_amd import runtime
from plan_helpers import Builder, half_words, pair, r4
from test_conv_views_gpu import input_canvas, poisoned

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)      # family -> largest ratio of this session
IS_HALF = lambda hc, which: {"x": hc.xh, "y": hc.yh, "r": hc.res == "h"}[which]
CANVAS = {"x": "X", "y": "Y", "r": "R"}


def build(hc, poison=False):
    """(builder, params, views, producers): the plan of a case.  views: which -> the view of the layer under test; producers: which ->
    (canvas name, the half buffer's whole-width view, canvas values) of the half buffers"""
    c, lay = hc.case, HR.layout(hc)
    b = Builder(c.N)
    b.options.append("dtype=f16")
    o = HR.operands(hc)
    params = {"c_w": o["w"], "c_b": o["bias"]}
    params.update(o.get("bn", {}))
    views, producers = {}, {}
    for which in ("x", "r", "y"):
        if which not in lay:
            continue
        Cs, c0, C, H, W = lay[which]
        if IS_HALF(hc, which):
            name, Cc = "P" + which, HR.r16(Cs)
            src = b.canvas(name, Cc, H, W, N=c.N + 1)
            buf = b.hbuf(Cs, H, W, N=c.N + 1)
            values, bias = HR.half_buffer(hc, which, poison)
            params[name + "_w"] = np.eye(Cs, Cc, dtype=np.float32).reshape(Cs, Cc, 1, 1)
            params[name + "_b"] = bias
            b.lines.append("conv name=%s in=%s out=%s w=%s_w bias=%s_b act=0 cin=%d cout=%d mode=conv k=1,1 s=1,1 p=0,0 d=1,1 nosplit=1" % (
                name, src.ref(), buf.ref(), name, name, Cc, Cs))
            views[which], producers[which] = buf.sub(c0, C, N=c.N), (name, buf, values)
        elif which == "y":
            views[which] = b.canvas("Y", Cs, H, W, N=c.N + 1).sub(c0, C, N=c.N)
        else:
            views[which] = b.canvas(CANVAS[which], Cs, H, W).sub(c0, C)
    t = ["conv name=c in=%s out=%s w=c_w act=%d slope=%r cin=%d cout=%d mode=%s" % (views["x"].ref(), views["y"].ref(), hc.act, hc.slope, c.Cin, c.Cout, c.mode)]
    if c.mode == "conv":
        t.append("k=%d,%d s=%d,%d p=%d,%d d=%d,%d" % (pair(c.k) + pair(c.s) + pair(c.p) + pair(c.d)))
    elif c.mode == "cols":
        t.append("wk=3,3")
    if hc.tile is not None:
        t.append("tile=%d" % hc.tile)
    if not c.ksplit and not c.auto:
        t.append("nosplit=1")
    if "bias" in c.epi:
        t.append("bias=c_b")
    if "bn" in c.epi:
        t.append("bn=bn fixg=0 eps=1e-5")
    if "r" in views:
        t.append("res=%s" % views["r"].ref())
    b.lines.append(" ".join(t))
    return b, params, views, producers


def bind(ctx, b, params):
    m = runtime.Model(ctx)
    try:
        m.set_params(params)
        plan = m.add_plan("p", b.text())
        plan.finalize()
    except Exception:
        m.close()
        raise
    return m, plan


def issue(hc, m, plan, b, views, producers, fp32_in, run, poison=False):
    """write every canvas, run, read everything back: ({canvas name: (words, tail)}, arena bytes)"""
    for name, buf, values in producers.values():
        b.write_canvas(m, name, values)
    for name, (view, canvas) in fp32_in.items():
        if poison:
            m.write(name, poisoned(b, name, view, canvas))
        else:
            b.write_canvas(m, name, canvas)
    if not hc.yh:
        b.write_canvas(m, "Y")
    run()
    return {name: b.read_canvas(m, name) for name in b.canvases}, plan.arena()


def first_difference(got, want):
    d = np.argwhere(got != want)
    return "%d of %d differ, first at %s: got 0x%x, want 0x%x" % (len(d), got.size, tuple(d[0]), got[tuple(d[0])], want[tuple(d[0])])


def output_bits(hc, b, producers, canvases, arena):
    """(the whole output buffer (N + 1, Ho, Wo, Cs) as bits, what it held before the run, the tail pair of an fp32 canvas or None)"""
    if hc.yh:
        return half_words(arena, producers["y"][1]), HR.half_buffer_bits(hc, "y"), None
    words, tail = canvases["Y"]
    want = b.canary("Y")
    return words, want[:words.size].reshape(words.shape), (tail, want[words.size:])


def check_placement(hc, b, views, producers, canvases, arena, what=""):
    """assertions 2 and 3; returns the view's bits (N, Ho, Wo, r4(Cout))"""
    y, N = views["y"], hc.case.N
    buf, before, tails = output_bits(hc, b, producers, canvases, arena)
    sl = slice(y.c0, y.c0 + hc.C4)
    outside = np.ones(buf.shape, bool)
    outside[:N, :, :, sl] = False
    assert np.array_equal(buf[outside], before[outside]), "elements outside the output view were written%s: %s" % (
        what, first_difference(np.where(outside, buf, 0), np.where(outside, before, 0)))
    if tails is not None:
        assert np.array_equal(*tails), "the tail behind the output canvas was written" + what
    got = np.ascontiguousarray(buf[:N, :, :, sl])
    assert not got[..., hc.Cout:].any(), "pad channels of the output are not +0%s: %s" % (what, sorted(set(got[..., hc.Cout:].reshape(-1).tolist()))[:4])
    return got


def on_half_views(ctx, hc):
    """the seven assertions of the module docstring on one case"""
    c = hc.case
    o = HR.operands(hc)
    b, params, views, producers = build(hc)
    m, plan = bind(ctx, b, params)
    try:
        op = [q for q in plan.ops() if q["name"] == "c"][0]      # 7
        assert op["mode"] == 1 and op["narrow"] == 0, op
        if c.auto:
            assert op["tile"] in HR.TILES and op["ksplit"] >= 1, op
        else:
            assert op["tile"] == hc.tile and (op["ksplit"] > 1) == c.ksplit, op
        fp32_in = {}
        if not hc.xh:
            fp32_in["X"] = (views["x"], input_canvas(b, "X", views["x"], o["x"], 11))
        if hc.res == "f":
            fp32_in["R"] = (views["r"], input_canvas(b, "R", views["r"], o["res"], 12))
        (g1, a1), (g2, a2) = (issue(hc, m, plan, b, views, producers, fp32_in, run) for run in (plan.run, plan.run_serial))
        assert np.array_equal(a1, a2), "graph replay and eager issue leave different bytes in the arena"      # 1
        for name in g1:
            assert np.array_equal(g1[name][0], g2[name][0]) and np.array_equal(g1[name][1], g2[name][1]), "graph replay and eager issue differ in " + name
        # 4: the producers first -- every half buffer the layer under test does not write holds the half bits of its canvas
        for which, (name, buf, values) in producers.items():
            if which != "y":
                got, want = half_words(a1, buf), HR.half_buffer_bits(hc, which)
                assert np.array_equal(got, want), "the producer of half %s did not store its canvas exactly: %s" % (which, first_difference(got, want))
            assert np.array_equal(g1[name][0], values.view(np.uint32)) and np.array_equal(g1[name][1], b.canary(name)[values.size:]), name + " was written"
        for name, (view, canvas) in fp32_in.items():
            assert np.array_equal(g1[name][0], canvas.view(np.uint32)) and np.array_equal(g1[name][1], b.canary(name)[canvas.size:]), name + " was written"
        got = check_placement(hc, b, views, producers, g1, a1)      # 2, 3
        if hc.kind == "exact":      # 5
            want = HR.expected(hc)
            assert np.array_equal(got, want), "%s: %s" % (hc.id, first_difference(got, want))
        else:
            ref = HR.reference(hc)
            if hc.yh:
                lo, hi = HR.interval(hc)
                h = got[..., :hc.Cout].view(np.float16)
                inside = (lo <= h) & (h <= hi)
                assert inside.all(), "%s: %d of %d elements outside [h(ref - b), h(ref + b)], first at %s" % (
                    hc.id, (~inside).sum(), inside.size, tuple(np.argwhere(~inside)[0]))
            else:
                y = got[..., :hc.Cout].view(np.float32).astype(np.float64)
                assert np.isfinite(y).all()
                ratio = np.abs(y - HR.nhwc(ref.y)) / HR.nhwc(ref.bound)
                WORST[hc.fam] = max(WORST[hc.fam], float(ratio.max()))
                print("%s: at %.3f of the bound" % (hc.id, ratio.max()))
                assert ratio.max() <= 1.0, "%s: at %s the error is %.3f of its bound" % (hc.id, np.unravel_index(np.argmax(ratio), ratio.shape), ratio.max())
    finally:
        m.close()
    # 6: the same plan with everything outside the input views poisoned
    b, params, views, producers = build(hc, poison=True)
    m, plan = bind(ctx, b, params)
    try:
        g3, a3 = issue(hc, m, plan, b, views, producers, fp32_in, plan.run, poison=True)
        for which, (name, buf, values) in producers.items():
            if which != "y":
                v = views[which]
                h = half_words(a3, buf).view(np.float16)
                inside = np.zeros(h.shape, bool)
                inside[:c.N, :, :, v.c0:v.c0 + r4(v.C)] = True
                assert np.isnan(h[~inside]).all() and not np.isnan(h[inside]).any(), "the poison did not reach half " + which
        again = check_placement(hc, b, views, producers, g3, a3, " (poisoned plan)")
        assert np.array_equal(again, got), "the output depends on what lies outside the input views: " + first_difference(again, got)
    finally:
        m.close()


@pytest.mark.parametrize("hc", HR.CASES, ids=lambda c: c.id)
def test_conv_on_half_views(ctx, monkeypatch, hc):
    monkeypatch.setenv("ACCEL_SPLIT", "b3")
    on_half_views(ctx, hc)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _refusal_plan(kind):
    """a 3x3 layer from an fp32 canvas to a half arena view (Cin 32, Cout 40, 5x7), with the one thing wrong `kind` names"""
    Cin, Cout, H, W = (24 if kind == "cin24" else 32), 40, 5, 7
    b = Builder(1)
    b.options.append("dtype=f16")
    x = b.canvas("X", Cin + 8, H, W).sub(4, Cin)
    Cs = 60 if kind == "cs" else 64
    buf = b.hbuf(64, H, W)
    y = buf.sub(4 if kind == "offset" else 8, Cout)
    y.Cs = Cs
    if kind == "pbuf":
        y = b.canvas("Y", 32, H, W).sub(8, Cout)      # 32 words = 64 halves per pixel
        y.half, y.Cs = True, 64
    rng = np.random.default_rng(3)
    params = {"c_w": rng.standard_normal((Cout, Cin, 3, 3)).astype(np.float32), "c_b": rng.standard_normal(Cout).astype(np.float32)}
    extra = ""
    if kind == "out2":
        extra = " out2=%s bias2=c_b" % b.canvas("Y2", Cout + 8, H, W).sub(4, Cout).ref()
    if kind.startswith("tile"):
        extra = " tile=%s" % kind[4:]
    b.lines.append("conv name=c in=%s out=%s w=c_w bias=c_b act=1 cin=%d cout=%d mode=conv k=3,3 s=1,1 p=1,1 d=1,1 nosplit=1%s" % (
        x.ref(), y.ref(), Cin, Cout, extra))
    return b, params


def test_the_refusal_plan_runs_when_nothing_is_wrong(ctx):
    """(so that each refusal below is a refusal of the one thing it changes)"""
    b, params = _refusal_plan("tile84")
    m, plan = bind(ctx, b, params)
    try:
        plan.run()
        assert [q["tile"] for q in plan.ops()] == [84]
    finally:
        m.close()


@pytest.mark.parametrize("kind", ["cs", "offset", "pbuf", "cin24", "out2", "tile76", "tile0", "tile86"])
def test_half_views_the_library_cannot_serve_are_refused(ctx, kind):
    """resolve(): Cs % 8, 16-byte offsets, the arena only; finalize_conv: Cin % 16, a single output; launch_conv_igemm /
    launch_conv_b3d: no kernel outside conv_b3d.hip's six reads or writes half views (86 is a retired id)"""
    b, params = _refusal_plan(kind)
    with pytest.raises(runtime.AccelError):
        m, plan = bind(ctx, b, params)
        try:
            plan.run()
        finally:
            m.close()


def test_zz_report_the_ratios():
    """(last in the file) the largest error-to-bound ratio per family of this session (bounded cases with an fp32 output)"""
    for fam in sorted(WORST):
        print("%-14s %.3f" % (fam, WORST[fam]))
