"""What finalize_conv (csrc/accel_hip.cpp) refuses on its own account, one case per refusal: a one-conv plan with tune=0 graph=0 that is
finalized and never run, on the smallest shapes that trigger it (a 4x6 map, 8 channels).  Every case breaks exactly ONE rule, so the
text it records does not depend on the order of the checks.  scripts/record_conv_refusals.py writes tests/golden/conv_refusals.json,
test_conv_finalize_gpu.py replays the cases against it.  No tests in here."""
import collections
import os

import numpy as np

from plan_helpers import Builder, V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_refusals.json")

H, W, C = 4, 6, 8
GEOMETRY_1X1 = "mode=conv k=1,1 s=1,1 p=0,0 d=1,1"


def _w(*shape):
    return np.random.default_rng(0).standard_normal(shape).astype(np.float32)


def _line(x, y, cin=C, cout=C, geometry=GEOMETRY_1X1, extra=""):
    return "conv name=c in=%s out=%s w=c_w act=0 slope=0.1 cin=%d cout=%d %s%s" % (x.ref(), y.ref(), cin, cout, geometry, (" " + extra) if extra else "")


def _plain(extra="", params=None, **kw):
    """the layer nothing is wrong with (8 -> 8 channels, 1x1, on a 4x6 map) with more keys on its line and other parameters"""
    def make(b):
        x, y = b.buf(C, H, W), b.buf(C, H, W)
        y2 = b.buf(C, H, W)
        return _line(x, y, extra=extra.replace("OUT2", y2.ref()), **kw), dict({"c_w": _w(C, C, 1, 1)}, **(params or {}))
    return make


def _too_narrow(b):
    x, y = b.buf(C, H, W), b.buf(4, H, W)      # Cout 8 into a Cs 4 view
    return _line(x, y), {"c_w": _w(C, C, 1, 1)}


def _deconv_size(b):
    x, y = b.buf(C, H, W), b.buf(C, 2 * H + 1, 2 * W)
    return _line(x, y, geometry="mode=deconv2x"), {"c_w": _w(C, C, 4, 4)}


def _deconv_weight(b):
    x, y = b.buf(C, H, W), b.buf(C, 2 * H, 2 * W)
    return _line(x, y, geometry="mode=deconv2x"), {"c_w": _w(C, C, 3, 3)}


def _geometry(b):
    x, y = b.buf(C, H, W), b.buf(C, H, W - 1)      # 3x3 / 1 / pad 1 keeps 4x6
    return _line(x, y, geometry="mode=conv k=3,3 s=1,1 p=1,1 d=1,1"), {"c_w": _w(C, C, 3, 3)}


def _input_narrow(b):
    x, y = b.buf(4, H, W), b.buf(C, H, W)      # Cin 8 from a Cs 4 view
    return _line(x, y), {"c_w": _w(C, C, 1, 1)}


def _batch(b):
    x, y = b.buf(C, H, W), b.buf(C, H, W)      # the builder's views hold 3 images: the input claims 2 of them
    return _line(x.sub(0, C, N=2), y), {"c_w": _w(C, C, 1, 1)}


def _four_gib(b):
    # views of persistent buffers are not held to the buffer's size when they are resolved: 16384 x 16384 pixels of 4 floats are 4 GiB.
    # Nothing that large is allocated, and nothing is launched
    b.head += ["pbuf name=X bytes=256", "pbuf name=Y bytes=256"]
    x, y = V(0, 4, 4, 16384, 16384, 1, space="X"), V(0, 4, 4, 16384, 16384, 1, space="Y")
    return _line(x, y, cin=4, cout=4), {"c_w": _w(4, 4, 1, 1)}


def _half_views(b):
    x, y = b.hbuf(C, H, W), b.hbuf(C, H, W)      # Cin 8: no multiple of 16
    return _line(x, y), {"c_w": _w(C, C, 1, 1)}


# name -> (images, plan options, builder of (conv line, parameters))
CASES = collections.OrderedDict([
    ("output-too-narrow", (1, [], _too_narrow)),
    ("weight-missing", (1, [], _plain(params={"c_w": None}))),
    ("weight-not-4d", (1, [], _plain(params={"c_w": _w(C, C)}))),
    ("weight-shape", (1, [], _plain(params={"c_w": _w(C, C, 3, 3)}))),
    ("deconv-weight-shape", (1, [], _deconv_weight)),
    ("deconv-output-size", (1, [], _deconv_size)),
    ("geometry-mismatch", (1, [], _geometry)),
    ("input-narrower-than-cin", (1, [], _input_narrow)),
    ("bias-missing", (1, [], _plain("bias=c_b"))),
    ("bias-size", (1, [], _plain("bias=c_b", {"c_b": _w(C - 1)}))),
    ("out2-needs-bn2-or-bias2", (1, [], _plain("out2=OUT2"))),
    ("bias2-missing", (1, [], _plain("out2=OUT2 bias2=c_b2"))),
    ("bias2-size", (1, [], _plain("out2=OUT2 bias2=c_b2", {"c_b2": _w(C + 1)}))),
    ("batch-sizes-differ", (3, [], _batch)),
    ("half-views", (1, ["dtype=f16"], _half_views)),
    ("view-exceeds-4gib", (1, [], _four_gib)),
])


def plan(name):
    """(plan text, parameters) of a case"""
    N, options, make = CASES[name]
    b = Builder(N)
    b.options += ["graph=0"] + options
    line, params = make(b)
    b.lines.append(line)
    return b.text(), {k: v for k, v in params.items() if v is not None}


def answer(ctx, name):
    """the text finalize refuses the case with; None if it takes the plan"""
    from accel_amd import runtime
    saved = {k: os.environ.pop(k, None) for k in ("ACCEL_SPLIT", "ACCEL_WITHHOLD", "ACCEL_CONV_DTYPE")}
    saved["ACCEL_AUTOTUNE"] = os.environ.get("ACCEL_AUTOTUNE")
    os.environ["ACCEL_AUTOTUNE"] = "0"
    text, params = plan(name)
    m = runtime.Model(ctx)
    try:
        m.set_params(params)
        try:
            m.add_plan("p", text).finalize()
        except runtime.AccelError as e:
            return str(e)
        return None
    finally:
        m.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
