"""Range slots of the fp16x2 form (csrc/range.h), writer by writer.

An fp16x2-form convolution takes its pixel scale from the range slot of its input tensor, and that slot is right only if every kernel
that stored into the tensor raised it to the largest |value| it stored.  Each case here is a hand-written plan
import_nchw -> WRITER UNDER TEST -> fp16x2 reader(s) -> export_nchw with every launch geometry forced, run several times on one bound
plan: bulk data at scale 1; the bulk at 2^-20 with one extreme 2^12 above it planted through the writer's input at a row of a full
tile; the bulk at 2^20 with the extreme NEGATIVE, planted at the last stored element (ragged tile, last image, last real channel);
(convolutions: a negative extreme at a row of a full tile as well); the first input again (the slots are cleared per run).  Every
run, graph replay and eager issue alike (bit-identical), asserts for every reader: the planted extreme is the unique maximum where it
was placed; word 0 of its slot is >= the largest |value| M of the tensor T the writer stored (read back) and bit-equal to it (readers
that can only be bounded -- channel sub-views, a fold before a later write, the cropped deconvolution -- are checked against an upper
bound instead); the scale puts M into [2^13, 2^14) with the expected source; the reader is at fp32 accuracy against float64 on T."""
import numpy as np
import pytest

from accel_amd import runtime
from plan_helpers import Builder, V, al, bits, bn_params, conv64, deconv64, r4  # noqa: F401

pytestmark = pytest.mark.gpu

BIG = 2.0 ** 12


def run_case(ctx, monkeypatch, b, feeds, expect, sources=None, locate=None, ulps=0, upper=None):
    """Bind b's plan once; for every input set of `feeds` (a list of {input name: array}) run it as a graph and eagerly and check
    every reader.  expect: {op name: {"tile": t, "ksplit>1": bool, "narrow": 0/1}} -- what must have run.  locate(run, reader) ->
    (n, c, y, x) of the planted unique maximum of that reader's T, or None.  upper(run, reader, outputs) -> an upper bound of word 0 (the
    deconvolution's cropped rows), None: word 0 must be bit-equal to M (within `ulps`)."""
    monkeypatch.setenv("ACCEL_SPLIT", "h2")
    m = runtime.Model(ctx)
    try:
        m.set_params(b.params)
        plan = m.add_plan("p", b.text())
        plan.finalize()
        ops = plan.ops()
        idx = {o["name"]: i for i, o in enumerate(ops)}
        for name, e in expect.items():
            o = ops[idx[name]]
            if "tile" in e:
                assert o["tile"] == e["tile"], (name, o)
            if "ksplit>1" in e:
                assert (o["ksplit"] > 1) == e["ksplit>1"], (name, o)
            if "narrow" in e:
                assert o["narrow"] == e["narrow"], (name, o)
        for name, _, _, tile in b.readers:
            assert ops[idx[name]]["mode"] == 3 and ops[idx[name]]["tile"] == tile, ops[idx[name]]
        for run, feed in enumerate(feeds):
            for k, v in feed.items():
                m.write(k, np.ascontiguousarray(v, np.float32))
            got = []
            for issue in (plan.run, plan.run_serial):
                issue()
                outs = {k: m.read(k, shape).copy() for k, shape in b.outputs.items()}
                words = {name: plan.range_words(idx[name]).copy() for name, _, _, _ in b.readers}
                got.append((outs, words, plan.ranges()))
            (outs, words, ranges), (outs2, words2, ranges2) = got
            for k in outs:
                assert np.array_equal(outs[k], outs2[k]), (run, k)
            for k in words:
                assert np.array_equal(words[k][0:1], words2[k][0:1]), (run, k)
            assert ranges == ranges2
            for name, _, w, tile in b.readers:
                t, y = outs[name + "_t"], outs[name + "_y"]
                M = float(np.abs(t).max())
                w0 = int(words[name][0])
                assert np.isfinite(t).all() and M > 0, (run, name)
                assert w0 >= bits(M), (run, name, "slot below the tensor's maximum", w0, bits(M))
                up = upper(run, name, outs) if upper else None
                if up is None:
                    assert abs(w0 - bits(M)) <= ulps, (run, name, "slot is not the tensor's maximum", w0, bits(M), M)
                else:
                    assert w0 <= bits(up), (run, name, "slot above the bound", w0, bits(up))
                s, src = ranges[name]
                want = (sources or {}).get(name, 1)
                assert src == want, (run, name, src)
                assert 2.0 ** 13 <= s * np.float32(np.uint32(w0).view(np.float32)) < 2.0 ** 14
                if up is None:
                    assert 2.0 ** 13 <= s * M < 2.0 ** 14, (run, name, s, M)
                pos = locate(run, name) if locate else None
                if pos is not None:
                    a = np.abs(t)
                    assert a[pos] == M and (a == M).sum() == 1, (run, name, pos, np.unravel_index(np.argmax(a), a.shape))
                k = w.shape[-1]
                ref = conv64(t.astype(np.float64), w, 1, k // 2)
                err = float(np.abs(y - ref).max() / np.abs(ref).max())
                assert err <= (3e-6 if tile in (40, 41, 42, 43) else 1e-6), (run, name, err)
    finally:
        m.close()


def planted(rng, shape, scale, at=None, sign=1.0, pattern=None):
    """bulk N(0, 1) * scale; at = (n, y, x): every channel of that pixel set to sign * 2^12 * scale * pattern"""
    x = rng.standard_normal(shape) * scale
    if at is not None:
        n, y, xx = at
        x[n, :, y, xx] = sign * BIG * scale * (pattern if pattern is not None else 1.0)
    return x.astype(np.float32)


# ---- convolution writers: (tile, N, Cin, Cout, H, W, k, s, p, d, act, epilogue, split[, options]) --------------------------------
# epilogue: "" | "bn" (mixed-sign scale / shift) | "res" | "dual" (out2 / bn2 behind a residual: the pre-activation trunk line)
# options: {"reader": geometry of the fp16x2 reader (3x3 for 41 / 43 / 78; default a 1x1 b3r one), "narrow": which narrow kernel}
CONV = [
    (0, 3, 32, 136, 13, 19, 3, 1, 1, 1, 0, "", False),
    (3, 3, 32, 136, 13, 19, 3, 1, 1, 1, 1, "bn", False),
    (4, 3, 32, 136, 13, 19, 3, 1, 1, 1, 2, "bn", False),
    (10, 3, 32, 136, 13, 19, 3, 1, 1, 1, 0, "res", False),
    (13, 3, 64, 136, 13, 19, 1, 1, 0, 1, 0, "dual", False),       # (geometry 13: K steps of 64)
    (16, 3, 32, 18, 13, 19, 3, 1, 1, 1, 2, "", False),
    (31, 3, 32, 136, 13, 19, 3, 1, 1, 1, 1, "res", False),
    (70, 3, 32, 136, 13, 19, 3, 1, 1, 1, 2, "bn", False),
    (73, 3, 32, 136, 13, 19, 3, 1, 1, 1, 0, "dual", False),
    (74, 3, 32, 18, 13, 19, 3, 1, 1, 1, 1, "", False),
    (75, 3, 32, 136, 13, 19, 3, 1, 1, 1, 0, "res", False),
    (76, 3, 32, 136, 13, 19, 3, 1, 1, 1, 2, "bn", False),
    (77, 3, 32, 136, 13, 19, 3, 1, 1, 1, 0, "res", False),
    (79, 3, 32, 136, 13, 19, 1, 1, 0, 1, 0, "dual", False),
    (80, 3, 32, 136, 13, 19, 3, 1, 1, 1, 1, "bn", False),
    (81, 3, 32, 18, 13, 19, 3, 2, 1, 1, 0, "", False),
    (76, 3, 32, 64, 12, 18, 3, 1, 1, 1, 2, "bn", False, {"reader": 41}),     # Winograd readers spend the slot's 4x of headroom
    (0, 3, 32, 64, 12, 18, 3, 1, 1, 1, 0, "res", False, {"reader": 43}),
    (81, 3, 32, 64, 13, 19, 3, 1, 1, 1, 2, "", False, {"reader": 78}),      # the halo geometry as the reader
    (40, 3, 32, 72, 12, 18, 3, 1, 1, 1, 0, "bn", False),
    (41, 3, 32, 72, 12, 18, 3, 1, 1, 1, 2, "", False),
    (42, 3, 32, 72, 12, 18, 3, 1, 1, 1, 0, "dual", False),
    (43, 3, 32, 72, 12, 18, 3, 1, 1, 1, 1, "res", False),
    (41, 1, 256, 72, 8, 8, 3, 1, 1, 1, 0, "dual", True),        # K split over blockIdx.y, finished by the split-K reduce
    (51, 3, 3, 64, 26, 38, 7, 2, 3, 1, 0, "", False),
    (50, 3, 3, 64, 26, 38, 7, 2, 3, 1, 1, "bn", False),
    (60, 3, 64, 256, 13, 19, 1, 1, 0, 1, 1, "", False),
    (78, 3, 64, 18, 13, 19, 3, 1, 1, 1, 2, "", False),
    (78, 3, 64, 18, 13, 19, 3, 1, 2, 2, 0, "bn", False),
    (0, 1, 256, 136, 6, 7, 3, 1, 1, 1, 0, "dual", True),        # the split-K reduce: low resolution, deep K
    (76, 1, 256, 136, 6, 7, 3, 1, 1, 1, 2, "bn", True),
    (-1, 3, 32, 3, 13, 19, 1, 2, 0, 1, 0, "bn", False, {"narrow": "pixel"}),     # conv_narrow_kernel (one pixel per wavefront)
    (-1, 3, 32, 2, 13, 19, 3, 1, 1, 1, 2, "", False, {"narrow": "pixel"}),       # 3x3 with M < 8192: conv_narrow_kernel as well
    (-1, 3, 32, 2, 48, 62, 3, 1, 1, 1, 2, "", False, {"narrow": "strip4"}),      # conv_narrow3x3_kernel<4>, the last strip ragged
]


def _conv_id(c):
    opt = c[13] if len(c) > 13 else {}
    return "t%d-n%d-%dx%d-%dx%d-k%ds%dd%d-act%d-%s%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[9], c[10], c[11] or "plain",
                                                         "-splitk" if c[12] else "", "".join("-%s%s" % kv for kv in sorted(opt.items())))


@pytest.mark.parametrize("case", CONV, ids=_conv_id)
def test_conv_epilogue_raises_the_slot_of_what_it_stored(ctx, monkeypatch, case):
    tile, N, Cin, Cout, H, W, k, s, p, d, act, epi, split = case[:13]
    opt = case[13] if len(case) > 13 else {}
    rng = np.random.default_rng(abs(tile) * 1000 + Cout + 7 * k + act)
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    tc = Cout - 1                                                   # the last real output channel
    pat = np.where(rng.random(Cin) < 0.5, -1.0, 1.0)                # the planted input pixel's channel pattern
    w = rng.standard_normal((Cout, Cin, k, k)) * 0.5 / np.sqrt(Cin * k * k)
    w[tc, :, k // 2, k // 2] = pat * 16.0 / Cin                     # channel tc sees the planted pixel 16x, the others about 1x
    b = Builder(N)
    x = b.inp("x", Cin, H, W)
    y = b.buf(Cout, Ho, Wo)
    extra = [] if split else ["nosplit=1"]
    if epi in ("bn", "dual"):
        b.params.update(bn_params(rng, "bn", Cout, tc, negative=(act == 0)))
        if epi == "bn":
            extra.append("bn=bn fixg=0")
    if epi in ("res", "dual"):
        r = b.inp("r", Cout, Ho, Wo)
        extra.append("res=%s" % r.ref())
    y2 = None
    if epi == "dual":
        y2 = b.buf(Cout, Ho, Wo)
        b.params.update(bn_params(rng, "bn2", Cout, tc, negative=True))       # scale2 < 0 in channel tc: y2's maximum comes from vmin
        extra.append("out2=%s bn2=bn2 fixg2=0 y2r=8" % y2.ref())
    b.conv("w", x, y, w.astype(np.float32), tile, k, s, p, d, act, yr=7, extra=" ".join(extra))
    if tile == -1:      # the narrow kernels take no forced geometry
        b.lines[-1] = b.lines[-1].replace(" tile=-1", "")
    rt = opt.get("reader", 81 if Cout % 8 else 77)
    b.reader("r1", y, 7, rng, tile=rt, k=3 if rt in (41, 43, 78) else 1)
    if y2 is not None:
        b.reader("r2", y2, 8, rng)
    sign3 = 1.0 if act == 1 else -1.0                               # behind a ReLU the extreme is positive
    last, inner = (N - 1, Ho - 1, Wo - 1), (0, 1, 2)
    at = lambda o: (o[0], o[1] * s - p + (k // 2) * d, o[2] * s - p + (k // 2) * d)
    feeds = []
    # runs: bulk; extreme at a row of a full tile (note_tile); NEGATIVE extreme at the last element (note_general); negative extreme at
    # a row of a full tile (note_tile's minimum: c * vmin, and the dual output through scale2 < 0); the first input again
    plan_runs = ((1.0, None, 1.0), (2.0 ** -20, inner, 1.0), (2.0 ** 20, last, sign3), (2.0 ** 10, inner, sign3), (1.0, None, 1.0))
    for sc, o, sg in plan_runs:
        f = {"x": planted(rng, (N, Cin, H, W), sc, None if o is None else at(o), sg, pat)}
        if "r" in b.inputs:
            f["r"] = planted(rng, (N, Cout, Ho, Wo), sc)
        feeds.append(f)
    feeds[-1] = feeds[0]
    where = {1: inner, 2: last, 3: inner}
    # (y2 in the negative runs: relu(-big * scale2 + shift2) with scale2 < 0 at the same pixel)
    locate = lambda run, name: None if run not in where or (name == "r2" and run not in (2, 3)) else (where[run][0], tc) + where[run][1:]
    if "narrow" in opt:      # ops() cannot tell the two narrow kernels apart: the shape must select the one named (misc.hip launch_conv_narrow)
        M = N * Ho * Wo
        strip = k == 3 and s == 1 and d == 1 and p == 1 and Cout <= 2
        if opt["narrow"] == "strip4":
            assert strip and 4 * 4 * 512 <= M < 8 * 4 * 1024 and Wo % 4, (M, Wo)
        else:
            assert not strip or M < 4 * 4 * 512, M
    expect = {"w": {"ksplit>1": split}}
    if tile >= 0:
        expect["w"]["tile"] = tile
    else:
        expect["w"]["narrow"] = 1
    run_case(ctx, monkeypatch, b, feeds, expect, locate=locate)


@pytest.mark.parametrize("odd", [False, True])
def test_deconv2x_epilogue_raises_the_slot(ctx, monkeypatch, odd):
    """mode=deconv2x: even sizes (exact), odd sizes (cropped rows and columns: the epilogue counts them on purpose, conv_epilogue.h --
    word 0 >= M and <= the float64 maximum of the UNCROPPED output)"""
    rng = np.random.default_rng(31 + odd)
    N, Cin, Cout, h, w_ = 3, 32, 18, 6, 9
    H2, W2 = 2 * h - odd, 2 * w_ - odd
    tc = Cout - 1
    pat = np.where(rng.random(Cin) < 0.5, -1.0, 1.0)
    w = rng.standard_normal((Cin, Cout, 4, 4)) * 0.5 / np.sqrt(Cin * 4)
    tap = 1 if odd else 2                                          # the tap that maps input (i, j) onto output (2i + tap - 1, 2j + tap - 1)
    w[:, tc, tap, tap] = pat * 16.0 / Cin
    b = Builder(N)
    x = b.inp("x", Cin, h, w_)
    y = b.buf(Cout, H2, W2)
    b.params["bias"] = (rng.standard_normal(Cout) * 2.0 ** -24).astype(np.float32)
    b.params["w_w"] = w.astype(np.float32)
    b.lines.append("conv name=w in=%s out=%s w=w_w bias=bias act=0 cin=%d cout=%d mode=deconv2x tile=76 nosplit=1 yr=7" % (x.ref(), y.ref(), Cin, Cout))
    b.reader("r1", y, 7, rng)
    o_last = (N - 1, H2 - 1, W2 - 1)
    i_last = (N - 1, h - 1, w_ - 1)
    feeds = [{"x": planted(rng, (N, Cin, h, w_), 1.0)},
             {"x": planted(rng, (N, Cin, h, w_), 2.0 ** -20, (0, 1, 2), 1.0, pat)},
             {"x": planted(rng, (N, Cin, h, w_), 2.0 ** 20, i_last, -1.0, pat)}]
    feeds.append(feeds[0])

    def full64(xx):
        return deconv64(xx, b.params["w_w"]) + b.params["bias"][None, :, None, None]
    inner = (0, 2 * 1 + tap - 1, 2 * 2 + tap - 1)
    locate = lambda run, name: {1: (0, tc) + inner[1:], 2: (N - 1, tc) + o_last[1:]}.get(run)
    upper = None
    if odd:
        upper = lambda run, name, outs: float(np.abs(full64(feeds[run]["x"].astype(np.float64))).max()) * (1 + 1e-6)
    run_case(ctx, monkeypatch, b, feeds, {"w": {"tile": 76, "ksplit>1": False}}, locate=locate, upper=upper)


def test_cols_gemm_and_dcn_cols_raise_their_slots(ctx, monkeypatch):
    """dcn_cols (dg 1 and 4, zero offsets: the columns are the input's 3x3 patches) writes a column buffer the fp16x2 GEMM
    (mode=cols, geometry 81) reads; that GEMM's output is read by a second reader"""
    rng = np.random.default_rng(41)
    N, C, H, W = 3, 32, 9, 13
    b = Builder(N)
    x = b.inp("x", C, H, W)
    outs = []
    for dg, rid in ((1, 7), (4, 9)):
        off = b.inp("off%d" % dg, 18 * dg, H, W)
        cols = b.buf(9 * C, H, W)
        b.lines.append("dcn_cols name=d%d in=%s off=%s out=%s k=3,3 s=1,1 p=1,1 d=1,1 dg=%d yr=%d" % (dg, x.ref(), off.ref(), cols.ref(), dg, rid))
        outs.append((cols, rid))
    cols, rid = outs[0]
    wc = (rng.standard_normal((40, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    b.params["g_w"] = wc
    y = b.buf(40, H, W)
    b.lines.append("conv name=g in=%s out=%s w=g_w act=2 slope=0.1 cin=%d cout=40 mode=cols wk=3,3 tile=81 nosplit=1 xr=%d yr=8" % (cols.ref(), y.ref(), C, rid))
    b.reader("r1", y, 8, rng)
    b.reader("r2", outs[1][0], outs[1][1], rng, K=64)
    b.reader("r0", cols, rid, rng, K=64)
    feeds = []
    for sc, at, sg in ((1.0, None, 1.0), (2.0 ** -20, (0, 2, 3), 1.0), (2.0 ** 20, (N - 1, H - 1, W - 1), -1.0)):
        f = {"x": planted(rng, (N, C, H, W), sc)}
        if at is not None:
            f["x"][at[0], C - 1, at[1], at[2]] = sg * BIG * sc
        f["off1"] = np.zeros((N, 18, H, W), np.float32)
        f["off4"] = np.zeros((N, 72, H, W), np.float32)
        feeds.append(f)
    feeds.append(feeds[0])
    run_case(ctx, monkeypatch, b, feeds, {"g": {"tile": 81, "ksplit>1": False}})


@pytest.mark.parametrize("kind", ["avg2x2-full", "max3x3s2-valid-bn-relu", "max2x2-bn"])
def test_pool_raises_the_slot(ctx, monkeypatch, kind):
    """the generic pool kernel (avg 2x2 'full' -- the last window a single pixel --, max 2x2 with BatchNorm) and pool_max3x3s2_kernel
    behind BatchNorm + ReLU.  The extreme is planted over a WHOLE window in the last channel, whose BatchNorm scale is -1: the pooled
    maximum is then the planted value itself, and behind the negative scale a negative plant becomes the largest output (a positive
    one the most negative: max2x2-bn has no ReLU).  Runs: a window of a full block, then the last window (the ragged block)."""
    rng = np.random.default_rng(51 + len(kind))
    N, C, H, W = 3, 20, 13, 19
    k, st = (3, 2) if kind.startswith("max3") else (2, 2)
    full = kind.endswith("full")
    po = lambda n: (1 + -(-(n - k) // st)) if full else (1 + (n - k) // st)
    Ho, Wo = po(H), po(W)
    b = Builder(N)
    x = b.inp("x", C, H, W)
    y = b.buf(C, Ho, Wo)
    extra = ""
    if "bn" in kind:
        b.params.update(bn_params(rng, "bn", C, C - 1, negative=True))
        extra = " bn=bn fixg=0 act=%d" % (1 if "relu" in kind else 0)
    b.lines.append("pool name=q kind=%s k=%d,%d s=%d,%d p=0,0 in=%s out=%s yr=7%s" % (kind[:3], k, k, st, st, x.ref(), y.ref(), extra))
    b.reader("r1", y, 7, rng)
    sign_in = -1.0 if "relu" in kind else 1.0      # behind the ReLU only a negative pooled maximum survives the scale -1
    runs = ((1.0, None, 1.0), (2.0 ** -20, (0, 1, 2), sign_in), (2.0 ** 20, (N - 1, Ho - 1, Wo - 1), sign_in),
            (2.0 ** 10, (1, 2, 3), -sign_in if "relu" not in kind else sign_in), (1.0, None, 1.0))
    feeds, where = [], {}
    for run, (sc, o, sg) in enumerate(runs):
        f = planted(rng, (N, C, H, W), sc)
        if o is not None:
            n, oy, ox = o
            f[n, C - 1, oy * st:min(oy * st + k, H), ox * st:min(ox * st + k, W)] = sg * BIG * sc      # the whole window
            where[run] = (n, C - 1, oy, ox)
        feeds.append({"x": f})
    feeds[-1] = feeds[0]
    run_case(ctx, monkeypatch, b, feeds, {}, locate=lambda run, name: where.get(run))


def test_copy_and_warp_raise_their_slots(ctx, monkeypatch):
    """copy_view, and flow_warp's two outputs (`out`, and `out2` = relu(out + bias): the warping_feat*fc6 line) at a zero flow"""
    rng = np.random.default_rng(61)
    N, C, H, W = 3, 24, 9, 13
    b = Builder(N)
    f = b.inp("f", C, H, W)
    fl = b.inp("fl", 2, H, W)
    big = b.buf(C + 8, H, W)
    cp = big.sub(8, C)
    b.lines.append("copy name=c src=%s dst=%s yr=7" % (f.ref(), cp.ref()))
    wo, wo2 = b.buf(C, H, W), b.buf(C, H, W)
    b.params["wbias"] = (rng.standard_normal(C) * 2.0 ** -24).astype(np.float32)
    b.lines.append("warp name=wp feat=%s flow=%s out=%s out2=%s bias=wbias yr=8 y2r=9" % (f.ref(), fl.ref(), wo.ref(), wo2.ref()))
    b.reader("rc", cp, 7, rng)
    b.reader("rw", wo, 8, rng)
    b.reader("rw2", wo2, 9, rng)
    feeds = []
    for sc, at, sg in ((1.0, None, 1.0), (2.0 ** -20, (0, 2, 3), 1.0), (2.0 ** 20, (N - 1, H - 1, W - 1), -1.0)):
        x = planted(rng, (N, C, H, W), sc)
        if at is not None:
            x[at[0], C - 1, at[1], at[2]] = sg * BIG * sc
        feeds.append({"f": x, "fl": np.zeros((N, 2, H, W), np.float32)})
    feeds.append(feeds[0])
    pos = {1: (0, C - 1, 2, 3), 2: (N - 1, C - 1, H - 1, W - 1)}
    locate = lambda run, name: pos.get(run) if name != "rw2" or run == 1 else None
    run_case(ctx, monkeypatch, b, feeds, {}, locate=locate)


def test_concat_of_three_writer_kinds(ctx, monkeypatch):
    """One buffer written by a convolution, a deconv2x and a narrow 3x3 flow predictor (the FlowNet decoder's concats; at this size
    conv_narrow_kernel), the extreme planted in each writer's part in turn and asserted there; its reader's slot exact.  Two readers
    of channel sub-views behind it: each slot >= its own view's maximum and <= the whole buffer's.  Second fold: another buffer
    written in channels [0, 32), read through that sub-view, written in [32, 64), read whole -- that fold sees both writes (exact).
    (A fold takes the maximum of word 0 and of partial words that are not cleared within a run: a write that OVERWRITES channels
    leaves their old maximum in the slot, a bound -- csrc/range.h; the lowering never overwrites a buffer it has read.)"""
    rng = np.random.default_rng(71)
    N, C, H, W = 3, 32, 12, 18
    b = Builder(N)
    x = b.inp("x", C, H, W)
    xs = b.inp("xs", C, H // 2, W // 2)
    cat = b.buf(32 + 16 + 2, H, W)                                   # [0, 32): conv, [32, 48): deconv2x, [48, 50): narrow
    pa, pn = np.where(rng.random(C) < 0.5, -1.0, 1.0), np.where(rng.random(C) < 0.5, -1.0, 1.0)
    wa = rng.standard_normal((32, C, 3, 3)) * 0.5 / np.sqrt(9 * C)
    wa[31, :, 1, 1] = pa * 16.0 / C                                   # channel 31 of the conv part sees pattern pa 16x
    wb = (rng.standard_normal((C, 16, 4, 4)) * 0.5 / np.sqrt(4 * C)).astype(np.float32)
    wn = rng.standard_normal((2, C, 3, 3)) * 0.5 / np.sqrt(9 * C)
    wn[1, :, 1, 1] = pn * 16.0 / C                                    # channel 49 (the predictor's second) sees pattern pn 16x
    b.conv("a", x, cat.sub(0, 32), wa.astype(np.float32), 76, 3, 1, 1, yr=7, extra="nosplit=1")
    b.params["b_w"] = wb
    b.lines.append("conv name=b in=%s out=%s w=b_w act=0 cin=%d cout=16 mode=deconv2x tile=0 nosplit=1 yr=7" % (xs.ref(), cat.sub(32, 16).ref(), C))
    b.conv("n", x, cat.sub(48, 2), wn.astype(np.float32), -1, 3, 1, 1, act=2, yr=7)
    b.lines[-1] = b.lines[-1].replace(" tile=-1", "")
    b.reader("r1", cat, 7, rng)
    b.reader("rs1", cat.sub(0, 32), 7, rng)
    b.reader("rs2", cat.sub(32, 16), 7, rng)
    sf = b.buf(64, H, W)
    b.conv("p1", x, sf.sub(0, 32), (rng.standard_normal((32, C, 1, 1)) * 0.3).astype(np.float32), 81, yr=9, extra="nosplit=1")
    b.reader("q1", sf.sub(0, 32), 9, rng)
    b.conv("p2", x, sf.sub(32, 32), (rng.standard_normal((32, C, 1, 1)) * 0.6).astype(np.float32), 0, yr=9, extra="nosplit=1")
    b.reader("q2", sf, 9, rng)
    feeds, where = [{"x": planted(rng, (N, C, H, W), 1.0), "xs": planted(rng, (N, C, H // 2, W // 2), 1.0)}], {}
    for sc, part in ((2.0 ** -20, "a"), (2.0 ** 20, "b"), (2.0 ** 10, "n")):
        f = {"x": planted(rng, (N, C, H, W), sc), "xs": planted(rng, (N, C, H // 2, W // 2), sc)}
        if part == "a":
            f["x"][0, :, 3, 4] = BIG * sc * pa
            where[len(feeds)] = (0, 31, 3, 4)
        elif part == "b":
            f["xs"][N - 1, :, H // 2 - 1, W // 2 - 1] = -BIG * sc      # (the deconvolution's four taps: no single pixel planned)
        else:
            f["x"][N - 1, :, H - 1, W - 1] = BIG * sc * pn
            where[len(feeds)] = (N - 1, 49, H - 1, W - 1)
        feeds.append(f)
    feeds.append(feeds[0])
    upper = lambda run, name, outs: {"rs1": outs["r1_t"], "rs2": outs["r1_t"], "q1": outs["q2_t"]}.get(name)
    upper_max = lambda run, name, outs: None if upper(run, name, outs) is None else float(np.abs(upper(run, name, outs)).max())

    def locate(run, name):
        if name != "r1" or run not in where:
            return None
        return where[run]
    expect = {"a": {"tile": 76}, "b": {"tile": 0}, "n": {"narrow": 1}, "p1": {"tile": 81}, "p2": {"tile": 0}}
    run_case(ctx, monkeypatch, b, feeds, expect, upper=upper_max, locate=locate)


def test_measured_inputs_source_2(ctx, monkeypatch):
    """measured paths (source 2): an import_nchw input whose C is not a multiple of 4 (maximum in the last real channel); a
    persistent buffer the host writes, read directly; a buffer with one writer without an epilogue (import_nchw) and one with"""
    rng = np.random.default_rng(81)
    N, C, H, W = 3, 18, 9, 13
    b = Builder(N)
    x = b.inp("x", C, H, W, yr=7)
    b.reader("r1", x, 7, rng)
    hb = b.pbuf("hb", 24, H, W)
    b.reader("rh", hb, 10, rng)
    mix = b.buf(40, H, W)
    xi = b.inp("xi", 20, H, W)
    b.lines.append("import_nchw src=xm:0:20:20:%d:%d:%d dst=%s yr=8" % (H, W, N, mix.sub(0, 20).ref()))
    b.head.append("pbuf name=xm bytes=%d" % (N * 20 * H * W * 4))
    b.inputs["xm"] = (N, 20, H, W)
    b.conv("c", xi, mix.sub(20, 20), (rng.standard_normal((20, 20, 1, 1)) * 0.2).astype(np.float32), 81, yr=8, extra="nosplit=1")
    b.reader("r2", mix, 8, rng)
    feeds = []
    for sc, at, sg in ((1.0, None, 1.0), (2.0 ** -20, (0, 2, 3), 1.0), (2.0 ** 20, (N - 1, H - 1, W - 1), -1.0)):
        f = {"x": planted(rng, (N, C, H, W), sc), "xi": planted(rng, (N, 20, H, W), sc), "xm": planted(rng, (N, 20, H, W), sc),
             "hb": planted(rng, (N, H, W, 24), sc)}
        if at is not None:
            f["x"][at[0], C - 1, at[1], at[2]] = sg * BIG * sc
            f["xm"][at[0], 19, at[1], at[2]] = sg * BIG * sc
            f["hb"][at[0], at[1], at[2], 23] = sg * BIG * sc
        feeds.append(f)
    feeds.append(feeds[0])
    pos = {1: (0, 2, 3), 2: (N - 1, H - 1, W - 1)}
    ch = {"r1": C - 1, "rh": 23, "r2": 19}
    run_case(ctx, monkeypatch, b, feeds, {"c": {"tile": 81}}, sources={"r1": 2, "r2": 2, "rh": 2},
             locate=lambda run, name: (pos[run][0], ch[name]) + pos[run][1:] if run in pos else None)


def test_prep_rgb_and_prep_flow_raise_their_slots(ctx, monkeypatch):
    """the image-boundary writers: prep_rgb (NCHW image -> NHWC4, with its BatchNorm of the pixel means) and prep_flow
    (Concat(cur / 255, prev / 255) -> avg pool 2x2 / 2 -> NHWC8), the extreme planted in the last real channel"""
    rng = np.random.default_rng(101)
    N, H, W = 3, 26, 38
    b = Builder(N)
    for name in ("img", "cur", "prev"):
        b.head.append("pbuf name=%s bytes=%d" % (name, N * 3 * H * W * 4))
        b.inputs[name] = (N, 3, H, W)
    b.params.update({"pbn_beta": np.array([-1.0, -2.0, -3.0], np.float32) * 2.0 ** -24, "pbn_moving_mean": np.zeros(3, np.float32),
                     "pbn_moving_var": np.full(3, 1.0 - 2e-5, np.float32)})
    rgb = b.buf(3, H, W)
    b.lines.append("prep_rgb name=pr src=img:0:3:3:%d:%d:%d dst=%s H=%d W=%d bn=pbn yr=7" % (H, W, N, rgb.ref(), H, W))
    fl = b.buf(6, H // 2, W // 2)
    b.lines.append("prep_flow name=pf cur=cur:0:3:3:%d:%d:%d prev=prev:0:3:3:%d:%d:%d dst=%s H=%d W=%d yr=8" % (H, W, N, H, W, N, fl.ref(), H, W))
    b.reader("r1", rgb, 7, rng)
    b.reader("r2", fl, 8, rng)
    feeds, where = [], {}
    for run, (sc, at, sg) in enumerate(((1.0, None, 1.0), (2.0 ** -20, (0, 1, 2), 1.0), (2.0 ** 20, (N - 1, H // 2 - 1, W // 2 - 1), -1.0))):
        f = {k: planted(rng, (N, 3, H, W), sc) for k in ("img", "cur", "prev")}
        if at is not None:
            n, oy, ox = at
            f["img"][n, 2, 2 * oy + 1, 2 * ox + 1] = sg * BIG * sc
            f["prev"][n, 2, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2] = sg * BIG * sc
            where[run] = {"r1": (n, 2, 2 * oy + 1, 2 * ox + 1), "r2": (n, 5, oy, ox)}
        feeds.append(f)
    feeds.append(feeds[0])
    run_case(ctx, monkeypatch, b, feeds, {}, locate=lambda run, name: where[run][name] if run in where else None)


@pytest.mark.parametrize("tile", [13, 79])
def test_dual_output_slot_does_not_count_rows_past_m(ctx, monkeypatch, tile):
    """conv_epilogue.h note_general (a wavefront with rows past M): a row past M stores nothing, so it must not raise y2's slot.
    Channel tc of y2 is relu(2 - v) with v = 1 + small everywhere (a residual of 1, scale2 = -1, shift2 = 2): its real maximum is
    about 1, while a row past M counted as v = 0 would put relu(shift2) = 2 into the slot -- twice the tensor's maximum"""
    rng = np.random.default_rng(91 + tile)
    N, Cin, Cout, H, W = 1, 64, 136, 13, 19                           # M = 247: the last wavefronts of a 128- or 64-row tile are ragged
    tc = Cout - 1
    b = Builder(N)
    x = b.inp("x", Cin, H, W)
    r = b.inp("r", Cout, H, W)
    y, y2 = b.buf(Cout, H, W), b.buf(Cout, H, W)
    g = np.ones(Cout, np.float32); g[tc] = -1.0
    beta = np.zeros(Cout, np.float32); beta[tc] = 2.0
    b.params.update({"bn2_gamma": g, "bn2_beta": beta, "bn2_moving_mean": np.zeros(Cout, np.float32),
                     "bn2_moving_var": np.full(Cout, 1.0 - 2e-5, np.float32)})
    w = (rng.standard_normal((Cout, Cin, 1, 1)) * 0.01 / np.sqrt(Cin)).astype(np.float32)
    b.conv("w", x, y, w, tile, yr=7, extra="nosplit=1 res=%s out2=%s bn2=bn2 fixg2=0 y2r=8" % (r.ref(), y2.ref()))
    b.reader("r2", y2, 8, rng)
    res = np.zeros((N, Cout, H, W), np.float32); res[:, tc] = 1.0
    feeds = [{"x": planted(rng, (N, Cin, H, W), 1.0), "r": res}]
    feeds.append(feeds[0])
    run_case(ctx, monkeypatch, b, feeds, {"w": {"tile": tile, "ksplit>1": False}})
