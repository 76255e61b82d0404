"""What NV12 frames cost and save against raw BGR frames (accel_model_prefetch_u8 / _commit_nv12, csrc/frames_yuv.hip): Accel-18, kf=5, at 1024x2048
(step 1: the frame is copied) and 720x1280 (resampled to 1024x1820, padded to 1024x1824), one clip per call and 8 clips per call.

    python scripts/microbench/nv12.py [--sizes 1024x2048 720x1280] [--batches 1 8] [--seconds 1.0] [--repeats 3] [--out profiles/nv12.md]

  (k) the conversion kernel alone, frames_nv12 against frames_u8 on frames resident in HBM: device-event time around trains of 20 launches on
      the library's compute stream, the two kernels alternating, --repeats rounds; GB/s over the bytes the algorithm moves at step 1
      (n * (1.5 hw + 12 HW) against n * (3 hw + 12 HW))
  (e) frames/s of the loop of bench.py's timed_pcie (step, prefetch of the next frame, asnumpy of the labels) fed with page-locked NV12 bytes
      against page-locked BGR bytes of the same pictures, alternating in one process, both warmed, each timed for at least --seconds,
      --repeats times; the spread is printed beside them."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

from frames_u8 import pcie_loop      # noqa: E402  (the same loop for both feeds)


def kernel_trains(model, launch, rounds, train=20):
    """ms per launch of `launch()` over `rounds` trains of back-to-back launches between one event pair (a 10 us kernel alone is launch-bound)"""
    import torch
    stream = torch.cuda.ExternalStream(model.ctx.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(rounds):
        e0.record(stream)
        for _ in range(train):
            launch()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / train)
    return out


def kernels_alone(model, n, h, w, g, means, repeats):
    """{"u8": [ms per launch, ...], "nv12": [...]} for n resident h x w frames converted into `data`"""
    import torch
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    nv = torch.randint(0, 256, (n, h * w * 3 // 2), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    geo = (g["out_h"], g["out_w"], g["step"], g["H"], g["W"])
    launches = {"u8": lambda: model.write_u8_device("data", bgr.data_ptr(), n, h, w, 3 * w, means, *geo),
                "nv12": lambda: model.write_nv12_device("data", nv.data_ptr(), n, h, w, w, h * w, h * w * 3 // 2, 0, means, *geo)}
    for fn in launches.values():
        for _ in range(3):
            fn()
    model.ctx.sync()
    ms = {"u8": [], "nv12": []}
    for _ in range(repeats):            # alternate
        for kind in ("u8", "nv12"):
            ms[kind] += kernel_trains(model, launches[kind], 5)
    model.ctx.sync()
    del bgr, nv
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["1024x2048", "720x1280"])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--interval", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from accel_amd import demo, mx, runtime
    from accel_amd.config.config import config, update_config
    from accel_amd.utils import image, synth
    update_config(os.path.join(ROOT, "tests", "golden", "dff_deeplab_vid_demo.yaml"))
    config.SCALES[0] = (1024, 2048)
    means = config.network.PIXEL_MEANS
    stride = config.network.IMAGE_STRIDE = config.network.IMAGE_STRIDE or 16      # the graphs want multiples of 16: 1820 columns are padded to 1824
    lines, record = [], {"interval": a.interval, "seconds": a.seconds, "repeats": a.repeats, "sizes": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown (not a git checkout)"
    import torch
    say("box: %s, torch %s; tree: %s; command: python %s" % (torch.cuda.get_device_name(0), torch.__version__, commit, " ".join(sys.argv)))

    for size in a.sizes:
        h, w = [int(v) for v in size.split("x")]
        scale, out_h, out_w, H, W = image.resize_geometry(h, w, config.SCALES[0][0], config.SCALES[0][1], stride)
        g = dict(out_h=out_h, out_w=out_w, step=image.resample_step(h, w, scale, out_h, out_w), H=H, W=W)
        say("== %s -> %d x %d in %d x %d, step %.6g (%s)" % (size, out_h, out_w, H, W, g["step"], "copy" if g["step"] == 1.0 else "resample"))
        arg, aux = synth.model_params("18", H, W, config)
        record["sizes"][size] = {"geometry": g, "batches": {}}
        for B in a.batches:
            model = runtime.Model(runtime.Context(0))
            runner = demo.ClipRunner("18", config, arg, aux, (H, W), model=model, batch=B)
            clips = [synth.make_clip(h, w, a.interval, seed=20260929 + b) for b in range(B)]
            pinned = mx.cpu_pinned()
            nv_bytes = [image.bgr_to_nv12_host(np.stack([c[t] for c in clips]), 0) for t in range(a.interval)]
            # the BGR feed shows the same pictures: the host conversion of the NV12 bytes
            bgr = [mx.nd.raw_frames(image.nv12_to_bgr_host(nv_bytes[t], h, w), config, ctx=pinned) for t in range(a.interval)]
            nv = [mx.nd.nv12_frames(nv_bytes[t], h, w, config, ctx=pinned) for t in range(a.interval)]
            zero = mx.nd.array(np.zeros((B, 2048, 1, 1), np.float32))
            batches = {"bgr": [[bgr[t], bgr[t - 1] if t else bgr[0], zero] for t in range(a.interval)],
                       "nv12": [[nv[t], nv[t - 1] if t else nv[0], zero] for t in range(a.interval)]}
            sync = model.ctx.sync
            for kind in ("bgr", "nv12"):      # warm both
                pcie_loop(runner, batches[kind], 0.0, sync)
                pcie_loop(runner, batches[kind], 0.0, sync)
            rates = {"bgr": [], "nv12": []}
            for _ in range(a.repeats):          # alternate
                for kind in ("bgr", "nv12"):
                    rates[kind].append(pcie_loop(runner, batches[kind], a.seconds, sync))
            assert all(r._host is None and r._frames is None for r in nv), "the NV12 route converted a frame on the host"
            for kind in ("bgr", "nv12"):
                v = rates[kind]
                say("(e) %s, %d clip(s) per call, page-locked %s bytes: %.1f frames/s (median of %d; %.1f .. %.1f, spread %.1f)"
                    % (size, B, kind.upper(), float(np.median(v)), len(v), min(v), max(v), max(v) - min(v)))
            ms = kernels_alone(model, B, h, w, g, means, a.repeats)
            moved = {"u8": B * (3 * h * w + 12 * H * W), "nv12": B * (h * w * 3 // 2 + 12 * H * W)}
            for kind in ("u8", "nv12"):
                v = ms[kind]
                say("(k) %s, %d frame(s), frames_%s: %.1f us per launch (median of %d trains; %.1f .. %.1f, spread %.1f)%s"
                    % (size, B, kind, float(np.median(v)) * 1e3, len(v), min(v) * 1e3, max(v) * 1e3, (max(v) - min(v)) * 1e3,
                       ", %.0f GB/s over %.1f MB" % (moved[kind] / float(np.median(v)) / 1e6, moved[kind] / 1e6) if g["step"] == 1.0 else ""))
            record["sizes"][size]["batches"][str(B)] = {"bgr_fps": rates["bgr"], "nv12_fps": rates["nv12"], "kernel_ms": ms, "bytes": moved}
            del bgr, nv, batches
            model.ctx.sync()
            model.close()
            model.ctx.close()
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
