"""Every convolution kernel on channel sub-views, against float64 (conv_ref.py): one hand-written plan per case of conv_ref.CASES with
`option tune=0`, the launch geometry forced with tile= (the narrow kernels take none) and asserted through plan.ops().

Every operand is a sub-view of a canvas of its own the host writes and reads raw; all channel strides differ and no offset is 0:
X Cs = r4(Cin) + 8 at channel 4, Y r4(Cout) + 12 at 8, the residual R r4(Cout) + 8 at 4, the second output Y2 r4(Cout) + 16 at 12
(narrow kernels: Y is the LAST slice of its canvas, the FlowNet concat layout; column GEMM: a dense column buffer, as dcn_cols
writes it).  Input canvases are random everywhere, the view's own pad channels zero.  Each plan runs as a graph and eagerly:

 1. both issues leave identical bits in every canvas;
 2. every word of Y and Y2 outside channels [c0, c0 + r4(Cout)) still holds its canary, the tail behind the canvas included (odd
    deconvolution: a tail of more than one output row, where a cropped row of the last image would land);
 3. the pad channels [Cout, r4(Cout)) of y and y2 hold +0.0;
 4. X and R read back as written;
 5. y and y2 are inside the bound and the bar of conv_ref.py;
 6. with every word of X and R outside the views (tails included) replaced by quiet NaNs, y and y2 keep their bits; under the
    fp16x2 form the measured range and its source stay as they were and nothing non-finite is reported.

Where a kernel's eligibility rules out an epilogue the forced geometry raises AccelError (conv_ref.REFUSED).

Every test prints its largest error-to-bound ratio (Winograd: error to bar; run with -s), the last test of the file the largest per
family.  One run on an MI355X: igemm 0-4 / 5-9 / 31-35 0.100, 10-12 + 14 0.078, 13 / 15 0.083, 16-19 0.078; bf16x3 and fp16x2 forms
0.014; Winograd fp32 0.077, bf16x3 0.066, fp16x2 0.073, split over K 0.081, behind the deep-K reduce 0.092; weight-stationary 0.065;
halo 0.002; narrow 0.036; split-K reduce below 0.001; deconvolution 0.034; column GEMM 0.009; f16 mode 0.054 (the stem cases of that
run failed: see conv_stem.hip's output stores; 0.027 in the run of the sweeps below).  The whole file took 3 s.

The geometry sweep (test_conv_geometry_on_sub_views) runs the same six assertions on conv_ref.GEOMETRY_RUN: 26 small shapes -- kernel
size, stride, padding and dilation with unequal height and width members (each pair on its own, and all four on a non-square map),
the networks' geometries, maps smaller than the filter, one / two / three / odd K steps and K far below K_pad, Cin % 8 == 4, M below,
at and one above the pixel tiles, Cout 5 / 33 / 129 / 260 -- crossed with one launch geometry per kernel template and loader path
(fp32 MFMA 0, 5, 10, 13, 31 and the DMA ring 16; conv_igemm_b3 70, 75; conv_b3r 76, 77, 80 as bf16x3 and as fp16x2; f16 mode on
conv_igemm_f16 0, 10, conv_b3r 76 and conv_b3d 82, 84, 88) and with no tile= at all under both split settings (the id conv_pick_tile
reports must be part of the build), plus the narrow pixel kernel on the anisotropic shapes and the split-K reduce behind 0 and 76
on one deep anisotropic K: 524 cases.  57 more must be refused (conv_ref.RULES and the kernels that demand square geometry), and 15
f16-mode requests on layers with a padded Cin off a multiple of 8 must report an fp32 layer.  One run on an MI355X, largest
error-to-bound ratio per family: geo-igemm 0.195, geo-b3 0.221, geo-b3r-b3 0.221, geo-b3r-h2 0.297, geo-f16 / geo-f16-b3r /
geo-f16-b3d 0.034, geo-auto 0.195, geo-narrow 0.223, geo-splitk 0.001.

The Winograd block sweep (test_winograd_blocks_on_sub_views) runs them on conv_ref.WINO_RUN: the 13 shapes of WINO_GEOMETRY -- every
block class of 42 (8x8, 4x16, 2x32) and 43 (4x8, 2x16) on a map it fits, on maps ragged in the tile rows, in the tile columns and in
both with a one-tile corner block; linear blocks of 40 / 41 below, at and above 64 tiles, across rows and images; K loops of 1, 2, 3,
4, 5 and 32 steps (2 to 64 on 40); splits over K with equal slices and with a short last one; nblk below 8, a multiple of 8 and
neither; Cout_store 8, 64, 68 and 132 -- crossed with 40 in fp32 and 41-43 as bf16x3 and as fp16x2, on Gaussian operands (assertion 5
against conv_ref.bar) and on dyadic ones, where assertion 5 is equality of every word of y with the float64 reference rounded once:
182 cases, 7 more refused.  ops() must report the forced id and the ksplit of conv_ref.wino_split.  The same run, error to bar:
wino-geo-fp32 0.171, wino-geo-b3 0.171, wino-geo-h2 0.081, wino-geo-splitk 0.100; all 91 dyadic cases bit for bit.  The whole file
(1010 tests) took 9 s; the 182 cases of this sweep with the 71 refusals, in a process of their own, 6 s."""
import collections

import numpy as np
import pytest

import conv_ref as R
import h2_model as H2
from accel_amd import runtime
from plan_helpers import Builder, pair, r4

pytestmark = pytest.mark.gpu

QNAN = 0x7FC00000
WORST = collections.defaultdict(float)      # family -> largest ratio of this session


def layout(case):
    """(builder, x, y, res, y2): the views of a case in their canvases"""
    b = Builder(case.N)
    if case.f16:
        b.options.append("dtype=f16")
    if case.mode == "cols":
        x = b.canvas("X", 9 * case.Cin, case.H, case.W).sub(0, 9 * case.Cin)
    else:
        x = b.canvas("X", r4(case.Cin) + 8, case.H, case.W).sub(4, case.Cin)
    Cs = r4(case.Cout) + 12
    # a cropped deconvolution must not write the rows it drops: behind the last image they would land in the tail
    tail = 64 + ((case.Wo + 2) * Cs if case.odd else 0)
    y = b.canvas("Y", Cs, case.Ho, case.Wo, tail=tail).sub(Cs - 4 if case.narrow else 8, case.Cout)
    res = b.canvas("R", r4(case.Cout) + 8, case.Ho, case.Wo).sub(4, case.Cout) if "res" in case.epi else None
    y2 = b.canvas("Y2", r4(case.Cout) + 16, case.Ho, case.Wo).sub(12, case.Cout) if "dual" in case.epi else None
    return b, x, y, res, y2


def conv_line(case, x, y, res, y2):
    t = ["conv name=c in=%s out=%s w=c_w act=%d slope=%r cin=%d cout=%d mode=%s" % (x.ref(), y.ref(), case.act, R.SLOPE, case.Cin, case.Cout, case.mode)]
    if case.mode == "conv":
        t.append("k=%d,%d s=%d,%d p=%d,%d d=%d,%d" % (pair(case.k) + pair(case.s) + pair(case.p) + pair(case.d)))
    elif case.mode == "cols":
        t.append("wk=3,3")
    if case.tile is not None:
        t.append("tile=%d" % case.tile)
    if not case.ksplit and not case.auto:
        t.append("nosplit=1")
    if "bias" in case.epi:
        t.append("bias=c_b")
    if "bn" in case.epi:
        t.append("bn=bn fixg=0 eps=1e-5")
    if res is not None:
        t.append("res=%s" % res.ref())
    if y2 is not None:
        t.append("out2=%s bn2=bn2 fixg2=0 eps2=1e-5" % y2.ref())
    return " ".join(t)


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def input_canvas(b, name, view, values, seed):
    """(N, H, W, Cs) fp32: random everywhere, the view's channels = values (NCHW), its pad channels zero"""
    N, H, W, Cs, _ = b.canvases[name]
    c = np.random.default_rng(seed).standard_normal((N, H, W, Cs)).astype(np.float32)
    c[..., view.c0:view.c0 + r4(view.C)] = 0.0
    c[..., view.c0:view.c0 + view.C] = nhwc(values)
    return c


def poisoned(b, name, view, canvas):
    """the canvas as words, every word outside the view (and the whole tail) a distinct quiet NaN"""
    N, H, W, Cs, tail = b.canvases[name]
    words = (np.uint32(QNAN) + np.arange(1, N * H * W * Cs + tail + 1, dtype=np.uint32) % np.uint32(1 << 22)).astype(np.uint32)
    body = words[:N * H * W * Cs].reshape(N, H, W, Cs)
    body[..., view.c0:view.c0 + r4(view.C)] = canvas.view(np.uint32)[..., view.c0:view.c0 + r4(view.C)]
    assert np.isnan(words[N * H * W * Cs:].view(np.float32)).all()
    return words


def bind(ctx, case, b, params):
    m = runtime.Model(ctx)
    try:
        m.set_params(params)
        plan = m.add_plan("p", b.text())
        plan.finalize()
    except Exception:
        m.close()
        raise
    return m, plan


def params_of(case, o):
    p = {"c_w": o["w"], "c_b": o["bias"]}
    p.update(o["bn"])
    p.update(o["bn2"])
    return p


def on_sub_views(ctx, monkeypatch, case):
    """the six assertions of the module docstring on one case"""
    monkeypatch.setenv("ACCEL_SPLIT", case.split)
    o = R.operands(case)
    b, x, y, res, y2 = layout(case)
    b.lines.append(conv_line(case, x, y, res, y2))
    m, plan = bind(ctx, case, b, params_of(case, o))
    try:
        # ---- what runs: the forced geometry, split over K or not, the narrow kernel the shape selects (misc.hip launch_conv_narrow)
        (op,) = plan.ops()
        assert op["narrow"] == (1 if case.narrow else 0), op
        if case.auto:      # no tile=: whatever conv_pick_tile chose is part of the build, split over K or not as conv_plan_split likes
            assert op["tile"] in R.VALID_TILES and op["ksplit"] >= 1, op
        else:
            assert (case.tile is None) == bool(case.narrow)
            if case.tile is not None:
                assert op["tile"] == case.tile, op
            assert (op["ksplit"] > 1) == case.ksplit, op
            if case.fam.startswith("wino-geo"):      # the K split is the one conv_ref restates: its slices are what the table is built on
                assert op["ksplit"] == R.wino_split(case.tile, case)[0], (op, R.wino_split(case.tile, case))
        if case.narrow:
            M = case.N * case.Ho * case.Wo
            strip = (pair(case.k), pair(case.s), pair(case.d), pair(case.p)) == ((3, 3), (1, 1), (1, 1), (1, 1)) and case.Cout <= 2
            want = "strip8" if strip and M >= 8 * 4 * 1024 else "strip4" if strip and M >= 4 * 4 * 512 else "pixel"
            assert want == case.narrow and (want == "pixel" or case.Wo % int(want[-1])), (M, case.Wo)
        form = R.form_of(case)
        assert op["mode"] == (1 if case.f16 else 3 if case.split == "h2" else 0), op

        inputs = {"X": (x, input_canvas(b, "X", x, o["x"], 11))}
        if res is not None:
            inputs["R"] = (res, input_canvas(b, "R", res, o["res"], 12))
        outputs = {"Y": y}
        if y2 is not None:
            outputs["Y2"] = y2

        def issue(run, poison=False):
            for name, (view, canvas) in inputs.items():
                if poison:
                    m.write(name, poisoned(b, name, view, canvas))
                else:
                    b.write_canvas(m, name, canvas)
            for name in outputs:
                b.write_canvas(m, name)
            run()
            got = {name: b.read_canvas(m, name) for name in list(inputs) + list(outputs)}
            return got, (plan.ranges() if form == "h2" else None)

        (g1, r1), (g2, r2) = issue(plan.run), issue(plan.run_serial)
        for name in g1:      # 1
            assert np.array_equal(g1[name][0], g2[name][0]) and np.array_equal(g1[name][1], g2[name][1]), "graph replay and eager issue differ in " + name
        assert r1 == r2
        for name, (view, canvas) in inputs.items():      # 4
            assert np.array_equal(g1[name][0], canvas.view(np.uint32)) and np.array_equal(g1[name][1], b.canary(name)[canvas.size:]), name + " was written"
        got = {}
        for name, view in outputs.items():
            words, tail = g1[name]
            assert b.untouched(name, words, tail, view.c0, view.C), "words outside the view of %s were written" % name      # 2
            assert not words[..., view.c0 + view.C:view.c0 + r4(view.C)].any(), "pad channels of %s are not +0.0" % name      # 3
            got[name] = np.transpose(np.ascontiguousarray(words[..., view.c0:view.c0 + view.C]).view(np.float32), (0, 3, 1, 2))
        if form == "h2":      # the range comes from the measuring launch over the sub-view
            s, src = r1["c"]
            assert src == 2 and s == H2.range_scale(H2.float_bits(np.abs(o["x"]).max())), (s, src)
        ratio = R.check(case, got["Y"], got.get("Y2"))      # 5
        if case.dyadic:      # integers in every intermediate of every form: no tolerance, the float64 reference rounded once
            want = R.reference(case).y.astype(np.float32)
            wrong = np.argwhere(got["Y"].view(np.uint32) != want.view(np.uint32))
            assert not len(wrong), "%s: %d words differ from the exact result, the first at (n, c, y, x) = %s: %r for %r" % (
                case.id, len(wrong), tuple(wrong[0]), got["Y"][tuple(wrong[0])], want[tuple(wrong[0])])
        WORST[case.fam] = max(WORST[case.fam], ratio)
        print("%s: at %.3f of the %s" % (case.id, ratio, "bar" if case.wino else "bound"))

        g3, r3 = issue(plan.run, poison=True)      # 6
        for name, view in outputs.items():
            sl = (Ellipsis, slice(view.c0, view.c0 + r4(view.C)))
            assert np.array_equal(g3[name][0][sl], g1[name][0][sl]), "%s depends on what lies outside the input views" % name
            assert b.untouched(name, g3[name][0], g3[name][1], view.c0, view.C), name
        assert r3 == r1, "the measured range depends on what lies outside the input view"
        plan.run()      # (a non-finite range of the run before is reported by the next one)
    finally:
        m.close()


@pytest.mark.parametrize("case", R.RUN_CASES, ids=lambda c: c.id)
def test_conv_on_sub_views(ctx, monkeypatch, case):
    on_sub_views(ctx, monkeypatch, case)


@pytest.mark.parametrize("case", R.GEOMETRY_RUN, ids=lambda c: c.id)
def test_conv_geometry_on_sub_views(ctx, monkeypatch, case):
    """the geometry sweep (conv_ref.GEOMETRY x GEOMETRY_KERNELS): unequal height and width members of every pair, the networks'
    geometries at small size, maps smaller than the filter, the edges of the K loop and of both tiles"""
    on_sub_views(ctx, monkeypatch, case)


@pytest.mark.parametrize("case", R.WINO_RUN, ids=lambda c: c.id)
def test_winograd_blocks_on_sub_views(ctx, monkeypatch, case):
    """the Winograd block sweep (conv_ref.WINO_GEOMETRY x WINO_KERNELS, on Gaussian and on dyadic operands): every block class of 42
    and 43 fitting and ragged, linear blocks across rows and images, K loops of one step to 64, short last slices of a split over K,
    every branch of the XCD swizzle; the dyadic cases bit for bit"""
    on_sub_views(ctx, monkeypatch, case)


@pytest.mark.parametrize("case", R.REFUSED + R.GEOMETRY_REFUSED + R.WINO_REFUSED, ids=lambda c: c.id)
def test_forced_geometry_refuses_what_it_cannot_run(ctx, monkeypatch, case):
    """an epilogue, a retired id or a geometry the kernel's eligibility rules out is an error, not something ignored: conv_*_eligible
    and the checks of accel_hip.cpp / launch_conv_igemm (conv_ref.RULES restates those of the geometry sweep)"""
    monkeypatch.setenv("ACCEL_SPLIT", case.split)
    b, x, y, res, y2 = layout(case)
    b.lines.append(conv_line(case, x, y, res, y2))
    with pytest.raises(runtime.AccelError):
        m, plan = bind(ctx, case, b, params_of(case, R.operands(case)))
        try:
            plan.run()
        finally:
            m.close()


@pytest.mark.parametrize("case", R.GEOMETRY_DEMOTED, ids=lambda c: c.id)
def test_f16_mode_leaves_layers_it_cannot_take_in_fp32(ctx, monkeypatch, case):
    """dtype=f16 on a layer whose padded Cin is no multiple of 8 (a K chunk of 8 would straddle two taps): the layer stays an fp32
    layer and says so through ops() -- those pairs are the fp32 rows of the sweep, nothing is refused and nothing runs in half"""
    monkeypatch.setenv("ACCEL_SPLIT", case.split)
    b, x, y, res, y2 = layout(case)
    b.lines.append(conv_line(case, x, y, res, y2))
    m, plan = bind(ctx, case, b, params_of(case, R.operands(case)))
    try:
        (op,) = plan.ops()
        assert op["mode"] == 0 and op["tile"] == case.tile, op
    finally:
        m.close()


def test_zz_report_the_ratios():
    """(last in the file) the largest ratio per family of this session"""
    for fam in sorted(WORST):
        print("%-14s %.3f" % (fam, WORST[fam]))

