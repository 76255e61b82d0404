"""What the overlay in the frame's own format (csrc/overlay_yuv.hip) costs, on frames resident in HBM, beside what a user had to run for a blended
picture before it existed -- the byte converter followed by the BGR blend (accel_yuv_to_bgr / accel_nv12_to_bgr, then accel_model_labels_colour
with that BGR frame), two kernels this feature did not touch:

    python scripts/microbench/overlay_yuv.py [--size 1024x2048] [--source 2160x3840] [--frames 8] [--train 200] [--rounds 5] [--repeats 3] [--out FILE]

Per format (NV12, I420, YUY2, P010), in ONE process with the kernels alternating, for label maps of --size:
  (i)  frames of --size: the identity geometry
  (s)  frames of --source: every source pixel gathers its label from the valid region of the map
each as  `out`  the overlay into a separate buffer,  `in`  the overlay in place, and  `bgr`  the two-kernel BGR path.
Measured as scripts/microbench/yuv.py measures (its trains()): device-event time around a train of --train back-to-back launches, divided by the
train, --repeats times --rounds trains per kernel, beside the host time it took to ENQUEUE a launch (where the two are about equal, the train
measured this process's enqueue rate, not the kernel).  Bytes moved, from the shapes: the overlay reads the valid region of the label map and the
frame and writes the frame; the BGR path reads the frame and writes 3 bytes per pixel, then reads the labels and those 3 bytes and writes 3 more.
For NV12 that is about 4 bytes per pixel against about 11.5."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from yuv import BYTES_IN, KINDS, trains      # noqa: E402


def labels_model(ctx, n, H, W):
    """a model that owns a `labels` buffer of n x H x W (no op: nothing is ever run)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=labels bytes=%d\nmeta labels_n=%d labels_h=%d labels_w=%d\n"
                     % ((n * H * W + 255) // 256 * 256, n, H, W))
    return m


def launches(model, image, n, h, w, out_h, out_w, palette, keep):
    """{(kind, what): launch()} for n resident h x w frames of random bytes against the model's label maps"""
    import torch
    from accel_amd import runtime
    ctx = model.ctx
    bgr = torch.zeros(n * h * w * 3, dtype=torch.uint8, device="cuda")
    blended = torch.zeros(n * h * w * 3, dtype=torch.uint8, device="cuda")
    keep += [bgr, blended]
    out = {}
    for kind in KINDS:
        size = int(n * h * w * BYTES_IN[kind])
        src = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
        dst = torch.zeros(size, dtype=torch.uint8, device="cuda")
        work = src.clone()
        keep += [src, dst, work]
        lay = image.overlay_layout(kind, h, w)
        table = image.palette_ycbcr(palette, 2, bits=10 if kind == "p010" else 8)
        struct = runtime.yuv_struct(lay, 2)
        out[kind, "out"] = lambda s=src.data_ptr(), d=dst.data_ptr(), y=struct, t=table: model.labels_overlay_yuv_device(s, d, n, out_h, out_w, y, t, alpha=128)
        out[kind, "in"] = lambda p=work.data_ptr(), y=struct, t=table: model.labels_overlay_yuv_device(p, p, n, out_h, out_w, y, t, alpha=128)
        if kind == "nv12":
            convert = lambda p=src.data_ptr(): ctx.nv12_to_bgr_device(p, bgr.data_ptr(), n, h, w, w, h * w, h * w * 3 // 2, 2, 3 * w)
        else:
            convert = lambda p=src.data_ptr(), y=runtime.yuv_struct(image.yuv_layout(kind, h, w), 2): ctx.yuv_to_bgr_device(p, bgr.data_ptr(), n, y, 3 * w)

        def two(convert=convert):
            convert()
            model.labels_colour_device(blended.data_ptr(), n, out_h, out_w, h, w, 3 * w, palette, frame_ptr=bgr.data_ptr(), frame_pitch=3 * w, alpha=128,
                                       rgb=False)
        out[kind, "bgr"] = two
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x2048")
    ap.add_argument("--source", default="2160x3840")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import runtime
    from accel_amd.dataset.cityscape import getpallete
    from accel_amd.utils import image
    H, W = [int(v) for v in a.size.split("x")]
    sh, sw = [int(v) for v in a.source.split("x")]
    n, stride = a.frames, 16
    lines, record = [], {"size": a.size, "source": a.source, "frames": n, "train": a.train, "rounds": a.rounds, "repeats": a.repeats, "ms": {}, "ratio": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown (not a git checkout)"
    say("box: %s, torch %s; tree: %s; command: python %s" % (torch.cuda.get_device_name(0), torch.__version__, commit, " ".join(sys.argv)))
    ctx = runtime.Context(0)
    palette = getpallete(256)
    model = labels_model(ctx, n, H, W)
    model.write("labels", np.random.default_rng(1).integers(0, 19, (n, H, W), dtype=np.uint8))
    out_h, out_w = image.resize_geometry(sh, sw, H, W, stride)[1:3]
    sets = {"i": ("identity, %d x %s" % (n, a.size), H, W, H, W), "s": ("%d x %s from the %d x %d region of %s maps" % (n, a.source, out_h, out_w, a.size),
                                                                         sh, sw, out_h, out_w)}
    for tag, (what, h, w, oh, ow) in sets.items():
        keep = []
        fns = launches(model, image, n, h, w, oh, ow, palette, keep)
        torch.cuda.synchronize()
        for fn in fns.values():         # warm every kernel
            for _ in range(5):
                fn()
        ctx.sync()
        ms, host = {k: [] for k in fns}, {k: [] for k in fns}
        for _ in range(a.repeats):      # alternate the kernels
            for key, fn in fns.items():
                dev, enq = trains(model, fn, a.rounds, a.train)
                ms[key] += dev
                host[key] += enq
        ctx.sync()
        px = n * h * w
        for kind in KINDS:
            moved = {"out": n * oh * ow + 2 * px * BYTES_IN[kind], "bgr": n * oh * ow + px * (BYTES_IN[kind] + 9)}
            moved["in"] = moved["out"]
            base = float(np.median(ms[kind, "bgr"]))
            for name in ("out", "in", "bgr"):
                v = np.asarray(ms[kind, name]) * 1e3
                med = float(np.median(v))
                ratio = base / float(np.median(ms[kind, name]))
                # the spread of the ratio: the slowest of these trains against the fastest of the BGR path's, and the other way round
                lo = float(np.min(ms[kind, "bgr"])) / float(np.max(ms[kind, name]))
                hi = float(np.max(ms[kind, "bgr"])) / float(np.min(ms[kind, name]))
                record["ms"]["%s %s %s" % (tag, kind, name)] = ms[kind, name]
                record["ratio"]["%s %s %s" % (tag, kind, name)] = [ratio, lo, hi]
                say("(%s) %s, %s %s: min %.2f us, median %.2f us per launch (%d trains of %d; max %.2f, spread %.1f %% of the median; host enqueue "
                    "%.2f us per launch), %.0f GB/s over %.1f MB (%.2f bytes per pixel); the BGR path takes %.2f times as long (%.2f .. %.2f over the "
                    "trains; from bytes alone %.2f)"
                    % (tag, what, kind, name, v.min(), med, len(v), a.train, v.max(), 100.0 * (v.max() - v.min()) / med,
                       float(np.median(host[kind, name])) * 1e3, moved[name] / med / 1e3, moved[name] / 1e6, moved[name] / px, ratio, lo, hi,
                       moved["bgr"] / moved[name]))
        ctx.sync()
        del keep, fns
    model.close()
    say("json " + json.dumps(record))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
