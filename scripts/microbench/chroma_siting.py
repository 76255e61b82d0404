"""What interpolated chroma siting (csrc/frames_sited.hip) costs beside the replicated kernels of the same format
(csrc/frames_yuv.hip), on frames resident in HBM:

    python scripts/microbench/chroma_siting.py [--size 1024x2048] [--source 720x1280] [--frames 1 8] [--train 200] [--rounds 5] [--repeats 3] [--out FILE]

Three things per format (NV12, I420, YUY2, P010) and siting (replicate, left, centre, topleft), in ONE process with the kernels alternating:
  (c) the step-1 kernel: a --size frame copied into the `data` input of that size (Model.write_yuv_device / write_nv12_device, siting = s)
  (r) the resample kernel: a --source frame resampled into the same input
  (b) the byte converter: a --size frame to packed BGR bytes (Context.yuv_to_bgr_device / nv12_to_bgr_device, siting = s)
Measured as scripts/microbench/yuv.py measures (its trains()): device-event time around a train of --train back-to-back launches, divided by the
train, --repeats times --rounds trains per kernel, beside the host time it took to ENQUEUE a launch (where the two are about equal, the train
measured this process's enqueue rate; that is why every set also runs at 8 frames per launch).  Every sited figure is held against the replicated
kernel of the SAME format in the SAME run -- siting 0 calls the entry points and kernels this feature did not touch.  From bytes alone the ratio
is 1: the same bytes cross HBM, the extra chroma taps are re-reads of lines a neighbouring thread brought in."""
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

from yuv import BYTES_IN, KINDS, input_model, trains      # noqa: E402

SITINGS = ("replicate", "left", "centre", "topleft")


def frame_launches(model, image, n, h, w, g, means, keep):
    """{(kind, siting): launch()} converting n resident h x w frames of random bytes into `data` with the geometry g"""
    import torch
    from accel_amd import runtime
    geo = (g["out_h"], g["out_w"], g["step"], g["H"], g["W"])
    out = {}
    for kind in KINDS:
        src = torch.randint(0, 256, (int(n * h * w * BYTES_IN[kind]),), dtype=torch.uint8, device="cuda")
        keep.append(src)
        for s, _ in enumerate(SITINGS):
            if kind == "nv12":
                out[kind, s] = lambda p=src.data_ptr(), s=s: model.write_nv12_device("data", p, n, h, w, w, h * w, h * w * 3 // 2, 2, means, *geo, siting=s)
            else:
                lay = runtime.yuv_struct(image.yuv_layout(kind, h, w), 2)
                out[kind, s] = lambda p=src.data_ptr(), lay=lay, s=s: model.write_yuv_device("data", p, n, lay, means, *geo, siting=s)
    return out


def bgr_launches(ctx, image, n, h, w, keep):
    import torch
    from accel_amd import runtime
    dst = torch.zeros(n * h * w * 3, dtype=torch.uint8, device="cuda")
    keep.append(dst)
    out = {}
    for kind in KINDS:
        src = torch.randint(0, 256, (int(n * h * w * BYTES_IN[kind]),), dtype=torch.uint8, device="cuda")
        keep.append(src)
        for s, _ in enumerate(SITINGS):
            if kind == "nv12":
                out[kind, s] = lambda p=src.data_ptr(), s=s: ctx.nv12_to_bgr_device(p, dst.data_ptr(), n, h, w, w, h * w, h * w * 3 // 2, 2, 3 * w, siting=s)
            else:
                lay = runtime.yuv_struct(image.yuv_layout(kind, h, w), 2)
                out[kind, s] = lambda p=src.data_ptr(), lay=lay, s=s: ctx.yuv_to_bgr_device(p, dst.data_ptr(), n, lay, 3 * w, siting=s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x2048")
    ap.add_argument("--source", default="720x1280")
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import runtime
    from accel_amd.utils import image
    H, W = [int(v) for v in a.size.split("x")]
    sh, sw = [int(v) for v in a.source.split("x")]
    means, stride = (103.06, 115.9, 123.15), 16
    lines, record = [], {"size": a.size, "source": a.source, "train": a.train, "rounds": a.rounds, "repeats": a.repeats, "ms": {}, "ratio": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown (not a git checkout)"
    say("box: %s, torch %s; tree: %s; command: python %s" % (torch.cuda.get_device_name(0), torch.__version__, commit, " ".join(sys.argv)))
    ctx = runtime.Context(0)
    scale, out_h, out_w, PH, PW = image.resize_geometry(H, W, H, W, stride)
    gc = dict(out_h=out_h, out_w=out_w, step=image.resample_step(H, W, scale, out_h, out_w), H=PH, W=PW)
    assert gc["step"] == 1.0 and (PH, PW) == (H, W), gc
    scale, out_h, out_w, PH, PW = image.resize_geometry(sh, sw, H, W, stride)
    gr = dict(out_h=out_h, out_w=out_w, step=image.resample_step(sh, sw, scale, out_h, out_w), H=PH, W=PW)
    assert gr["step"] != 1.0, gr
    for n in a.frames:
        keep, sets = [], {}
        models = [input_model(ctx, gc["H"], gc["W"], n), input_model(ctx, gr["H"], gr["W"], n)]
        sets["c"] = ("step-1 kernel, %d x %s" % (n, a.size), models[0], frame_launches(models[0], image, n, H, W, gc, means, keep))
        sets["r"] = ("resample kernel, %d x %s -> %d x %d in %d x %d" % (n, a.source, gr["out_h"], gr["out_w"], gr["H"], gr["W"]), models[1],
                     frame_launches(models[1], image, n, sh, sw, gr, means, keep))
        sets["b"] = ("byte converter, %d x %s" % (n, a.size), models[0], bgr_launches(ctx, image, n, H, W, keep))
        torch.cuda.synchronize()
        for tag, (what, model, launches) in sets.items():
            for fn in launches.values():         # warm every kernel
                for _ in range(5):
                    fn()
            ctx.sync()
            ms, host = {k: [] for k in launches}, {k: [] for k in launches}
            for _ in range(a.repeats):           # alternate the kernels
                for key, fn in launches.items():
                    dev, enq = trains(model, fn, a.rounds, a.train)
                    ms[key] += dev
                    host[key] += enq
            ctx.sync()
            for kind in KINDS:
                base = float(np.median(ms[kind, 0]))
                for s, name in enumerate(SITINGS):
                    v = np.asarray(ms[kind, s]) * 1e3
                    ratio = float(np.median(ms[kind, s])) / base
                    record["ms"]["%s%d %s %s" % (tag, n, kind, name)] = ms[kind, s]
                    record["ratio"]["%s%d %s %s" % (tag, n, kind, name)] = ratio
                    tail = ""
                    if tag == "c":
                        moved = n * H * W * (12 + BYTES_IN[kind])
                        tail = ", %.0f GB/s over %.1f MB" % (moved / float(np.median(v)) / 1e3, moved / 1e6)
                    say("(%s) %s, %s %s: min %.2f us, median %.2f us per launch (%d trains of %d; max %.2f, spread %.1f %% of the median; host "
                        "enqueue %.2f us per launch)%s; %.3f of the replicated kernel's time"
                        % (tag, what, kind, name, v.min(), float(np.median(v)), len(v), a.train, v.max(),
                           100.0 * (v.max() - v.min()) / float(np.median(v)), float(np.median(host[kind, s])) * 1e3, tail, ratio))
        ctx.sync()
        del keep, sets
        for m in models:
            m.close()
    say("json " + json.dumps(record))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
