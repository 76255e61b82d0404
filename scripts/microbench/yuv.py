"""What the I420, P010 and YUY2 kernels cost beside the NV12 kernels (all in csrc/frames_yuv.hip), on frames resident in HBM:

    python scripts/microbench/yuv.py [--size 1024x2048] [--source 720x1280] [--frames 1 8] [--train 200] [--rounds 5] [--repeats 3] [--out FILE]

Three things per format, NV12 among them, in ONE process with the formats alternating:
  (c) the step-1 kernel: a --size frame copied into the `data` input of that size (accel_model_write_yuv / _nv12, source on the device)
  (r) the resample kernel: a --source frame resampled into the same input
  (b) the byte converter: a --size frame to packed BGR bytes (accel_yuv_to_bgr / accel_nv12_to_bgr, device to device)
Every figure is device-event time around a train of --train back-to-back launches on the library's compute stream, divided by the train; every
kernel is warmed first; --repeats times --rounds trains per kernel; the minimum and the median are printed, and the spread.  Beside it stands the
host time it took to ENQUEUE a launch of that train: where the two are about equal the train measured the enqueue rate of this Python process, not
the kernel.  That is why every set also runs with --frames frames per launch (8 by default): the kernel then takes 8 times as long and the host
keeps ahead of it.  (c) is priced over the bytes the algorithm moves, n h w (12 + bytes in per pixel), and held against NV12's time in the same
run: from bytes alone format f should take (12 + bytes_in_f) / 13.5 of it; more than 15 % above that ratio says its load side does not coalesce."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

BYTES_IN = {"nv12": 1.5, "i420": 1.5, "yuy2": 2.0, "p010": 3.0}      # per pixel
KINDS = ("nv12", "i420", "yuy2", "p010")


def trains(model, launch, rounds, train):
    """(ms per launch, host ms to enqueue a launch) of `launch()` over `rounds` trains of back-to-back launches between one event pair"""
    import torch
    stream = torch.cuda.ExternalStream(model.ctx.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out, host = [], []
    for _ in range(rounds):
        e0.record(stream)
        t0 = time.perf_counter()
        for _ in range(train):
            launch()
        host.append((time.perf_counter() - t0) * 1e3 / train)
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / train)
    return out, host


def input_model(ctx, H, W, n=1):
    """a model with the image inputs `data` / `data_key` of n H x W frames (the one-op plan of accel_flow_input; never finalized or run)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    ib, h2, w2 = n * 3 * H * W * 4, H // 2, W // 2
    arena = (h2 * w2 * 32 + 255) // 256 * 256
    m.add_plan("op", "option graph=0 tune=0\narena bytes=%d\npbuf name=data bytes=%d\npbuf name=data_key bytes=%d\npbuf name=y bytes=%d\n"
                     "prep_flow cur=data:0:3:4:%d:%d prev=data_key:0:3:4:%d:%d dst=A:0:6:8:%d:%d H=%d W=%d\n"
                     "export_nchw src=A:0:6:8:%d:%d dst=y:0:6:8:%d:%d\n"
               % (arena, ib, ib, 6 * h2 * w2 * 4, H, W, H, W, h2, w2, H, W, h2, w2, h2, w2))
    return m


def frame_launches(model, image, n, h, w, g, means, keep):
    """{kind: launch()} converting n resident h x w frames of random bytes into `data` with the geometry g"""
    import torch
    from accel_amd import runtime
    geo = (g["out_h"], g["out_w"], g["step"], g["H"], g["W"])
    out = {}
    for kind in KINDS:
        src = torch.randint(0, 256, (int(n * h * w * BYTES_IN[kind]),), dtype=torch.uint8, device="cuda")
        keep.append(src)
        if kind == "nv12":
            out[kind] = lambda p=src.data_ptr(): model.write_nv12_device("data", p, n, h, w, w, h * w, h * w * 3 // 2, 2, means, *geo)
        else:
            lay = runtime.yuv_struct(image.yuv_layout(kind, h, w), 2)
            out[kind] = lambda p=src.data_ptr(), lay=lay: model.write_yuv_device("data", p, n, lay, means, *geo)
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
        if kind == "nv12":
            out[kind] = lambda p=src.data_ptr(): ctx.nv12_to_bgr_device(p, dst.data_ptr(), n, h, w, w, h * w, h * w * 3 // 2, 2, 3 * w)
        else:
            lay = runtime.yuv_struct(image.yuv_layout(kind, h, w), 2)
            out[kind] = lambda p=src.data_ptr(), lay=lay: ctx.yuv_to_bgr_device(p, dst.data_ptr(), n, lay, 3 * w)
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
    lines, record = [], {"size": a.size, "source": a.source, "train": a.train, "rounds": a.rounds, "repeats": a.repeats, "ms": {}}

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
            ms, host = {k: [] for k in KINDS}, {k: [] for k in KINDS}
            for _ in range(a.repeats):           # alternate the formats
                for kind in KINDS:
                    dev, enq = trains(model, launches[kind], a.rounds, a.train)
                    ms[kind] += dev
                    host[kind] += enq
            ctx.sync()
            record["ms"]["%s%d" % (tag, n)] = ms
            base = float(np.median(ms["nv12"]))
            for kind in KINDS:
                v = np.asarray(ms[kind]) * 1e3
                ratio = float(np.median(ms[kind])) / base
                tail = ", %.3f of NV12's time" % ratio
                if tag == "c":
                    moved = n * H * W * (12 + BYTES_IN[kind])
                    want = (12 + BYTES_IN[kind]) / 13.5
                    tail = ", %.0f GB/s over %.1f MB; %.3f of NV12's time, %.3f from bytes alone (%+.1f %%)" \
                           % (moved / float(np.median(v)) / 1e3, moved / 1e6, ratio, want, 100.0 * (ratio / want - 1.0))
                say("(%s) %s, %s: min %.2f us, median %.2f us per launch (%d trains of %d; max %.2f, spread %.1f %% of the median; host enqueue "
                    "%.2f us per launch)%s" % (tag, what, kind, v.min(), float(np.median(v)), len(v), a.train, v.max(),
                                               100.0 * (v.max() - v.min()) / float(np.median(v)), float(np.median(host[kind])) * 1e3, tail))
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
