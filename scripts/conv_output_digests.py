#!/usr/bin/env python
"""One sha256 per convolution output, to compare two builds of the library bit for bit (ACCEL_LIB_PATH selects the build): run it on the
MI355X once per build -- twice on the old one, to learn which rows repeat -- and diff the files.  Rows:
  ref|<case id>          every runnable case of tests/conv_ref.py (RUN_CASES, GEOMETRY_RUN, WINO_RUN) on the sub-view layout of
                         tests/test_conv_views_gpu.py: the bytes of the Y canvas, and of Y2 where the case has a second output
  grid|<layer>|<mode>|<id>   the layers x plan modes of tests/conv_geometry.py at the default split setting, every launch geometry id
                         (and no tile= at all) that finalizes: the output in NCHW (f16-half: the half words of the output view, behind a
                         1x1 layer that writes the half input); an id that finalizes and is refused at launch records that text;
                         id 15 is left out in the f16 modes (grid_rows says why)
  deform|dg<n>           accel_deform_conv2d (the column GEMM, mode=cols)
  deconv|bias            accel_deconv2d_4x4s2 with a bias
A device fault ends the script at once.
    conv_output_digests.py --out FILE [--only ref,grid,ops]"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

import conv_geometry as G      # noqa: E402
import conv_ref as R      # noqa: E402
import test_conv_views_gpu as T      # noqa: E402
from accel_amd import runtime      # noqa: E402
from plan_helpers import Builder, half_words, pair      # noqa: E402

sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
r8 = lambda c: (c + 7) // 8 * 8


def fatal(e):
    return any(s in str(e) for s in ("illegal memory access", "hipErrorLaunchFailure", "unspecified launch failure"))


def ref_rows(ctx):
    for case in R.RUN_CASES + R.GEOMETRY_RUN + R.WINO_RUN:
        os.environ["ACCEL_SPLIT"] = case.split
        o = R.operands(case)
        b, x, y, res, y2 = T.layout(case)
        b.lines.append(T.conv_line(case, x, y, res, y2))
        m, plan = T.bind(ctx, case, b, T.params_of(case, o))
        try:
            b.write_canvas(m, "X", T.input_canvas(b, "X", x, o["x"], 11))
            if res is not None:
                b.write_canvas(m, "R", T.input_canvas(b, "R", res, o["res"], 12))
            for name in ["Y"] + (["Y2"] if y2 is not None else []):
                b.write_canvas(m, name)
            plan.run()
            yield "ref|" + case.id, " ".join(sha(np.concatenate([a.reshape(-1) for a in b.read_canvas(m, name)]))
                                            for name in ["Y"] + (["Y2"] if y2 is not None else []))
        finally:
            m.close()
    os.environ.pop("ACCEL_SPLIT", None)


def grid_plan(layer, mode, tile):
    """(builder, output view) of a grid layer between buffers the host can fill and read"""
    g = G.LAYERS[layer]
    b = Builder(g["N"])
    b.options += ["graph=0", G.MODES[mode]]
    if g["mode"] == "deconv2x":
        Ho, Wo = 2 * g["H"], 2 * g["W"]
    else:
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(g["k"]), pair(g["s"]), pair(g["p"]), pair(g["d"])
        Ho, Wo = (g["H"] + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (g["W"] + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if mode == "f16-half":
        x16 = b.inp("X", 16, g["H"], g["W"])
        xh = b.hbuf(r8(g["Cin"]), g["H"], g["W"])
        wpre = (np.random.default_rng(1).standard_normal((xh.C, 16, 1, 1)) / 4).astype(np.float32)
        b.conv("pre", x16, xh, wpre, -1)
        x, y = xh.sub(0, g["Cin"]), b.hbuf(r8(g["Cout"]), Ho, Wo).sub(0, g["Cout"])
    else:
        x, y = b.inp("X", g["Cin"], g["H"], g["W"]), b.buf(g["Cout"], Ho, Wo)
    t = ["conv name=c in=%s out=%s w=c_w act=0 slope=0.1 cin=%d cout=%d mode=%s" % (x.ref(), y.ref(), g["Cin"], g["Cout"], g["mode"])]
    if g["mode"] == "conv":
        t.append("k=%d,%d s=%d,%d p=%d,%d d=%d,%d" % (pair(g["k"]) + pair(g["s"]) + pair(g["p"]) + pair(g["d"])))
    if tile is not None:
        t.append("tile=%d" % tile)
    b.lines.append(" ".join(t))
    if mode != "f16-half":
        b.out("Y", y)
    b.params["c_w"] = G.weights(layer)
    return b, y


def grid_rows(ctx):
    for k in ("ACCEL_SPLIT", "ACCEL_WITHHOLD", "ACCEL_WB3_FORCE"):
        os.environ.pop(k, None)
    for layer, g in G.LAYERS.items():
        for mode in G.MODES:
            N, C = g["N"], 16 if mode == "f16-half" else g["Cin"]
            xin = np.random.default_rng(7).standard_normal((N, C, g["H"], g["W"])).astype(np.float32)
            for tile in g["ids"]:
                if tile == 15 and mode.startswith("f16"):
                    # not run: conv_plan_split counts this id's K steps in its own 16, the f16 kernel the layer runs on steps by 32
                    # (conv_igemm_f16_kernel), so the upper slices start past K and index the tap table beyond its end
                    continue
                b, y = grid_plan(layer, mode, tile)
                m = runtime.Model(ctx)
                try:
                    m.set_params(b.params)
                    try:
                        plan = m.add_plan("p", b.text())
                        plan.finalize()
                    except runtime.AccelError:
                        continue      # (what finalize refuses: tests/golden/conv_geometry.json)
                    m.write("X", xin)
                    key = "grid|%s|%s|%s" % (layer, mode, "none" if tile is None else tile)
                    try:
                        plan.run()
                    except runtime.AccelError as e:
                        if fatal(e):
                            raise
                        yield key, "refused at launch: %s" % e
                        continue
                    if mode == "f16-half":
                        yield key, sha(half_words(plan.arena(), y)[..., :y.C])
                    else:
                        yield key, sha(m.read("Y", b.outputs["Y"]))
                finally:
                    m.close()


def op_rows(ctx):
    rnd = lambda seed, *shape, **kw: (np.random.default_rng(seed).standard_normal(shape) * kw.get("scale", 1.0)).astype(np.float32)
    C, K, H, W = 32, 48, 12, 20
    x, w = rnd(15, 1, C, H, W), rnd(16, K, C, 3, 3, scale=0.06)
    for dg in (1, 4):
        yield "deform|dg%d" % dg, sha(ctx.deform_conv2d(x, rnd(17, 1, 18 * dg, H, W), w, 1, 2, 2, dg))
    x, w, bias = rnd(12, 2, 24, 9, 13), rnd(13, 24, 10, 4, 4, scale=0.1), rnd(14, 10)
    yield "deconv|bias", sha(ctx.deconv2d_4x4s2(x, w, bias, act=2, slope=0.1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="ref,grid,ops")
    a = ap.parse_args()
    os.environ["ACCEL_AUTOTUNE"] = "0"
    ctx = runtime.Context(0)
    t0, n = time.time(), 0
    try:
        with open(a.out, "w") as f:
            for what, rows in (("ref", ref_rows), ("grid", grid_rows), ("ops", op_rows)):
                if what not in a.only.split(","):
                    continue
                for key, digest in rows(ctx):
                    f.write("%s %s\n" % (key, digest))
                    n += 1
                    if n % 200 == 0:
                        f.flush()
                        print("%d rows, %.0f s" % (n, time.time() - t0), flush=True)
    finally:
        ctx.close()
    print("%d rows in %.0f s from %s -> %s" % (n, time.time() - t0, runtime.LIB_PATH, a.out))


if __name__ == "__main__":
    main()
