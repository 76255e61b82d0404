"""What raw uint8 frames cost and save (accel_model_prefetch_u8 / _commit_u8, csrc/frames_u8.hip): Accel-18 at 1024x2048, kf=5, one clip per call
and 8 clips per call, through the loop of bench.py's timed_pcie (step, prefetch of the next frame, asnumpy of the labels).

    python scripts/microbench/frames_u8.py [--batches 1 8] [--seconds 1.0] [--repeats 3] [--out profiles/frames_u8.md]

  (a) frames/s with fp32 page-locked frames (the path every release so far has had)
  (b) frames/s with raw uint8 page-locked frames
  (c) host milliseconds per frame of transform(resize(frame)) -> fp32: what (b) removes from a live pipeline and (a) hides before its loop
  (d) the conversion kernel alone at step == 1: device-event time and achieved GB/s over n * (3hw + 12HW) bytes
(a) and (b) alternate in one process, both warmed, each timed for at least --seconds, --repeats times; the spread is printed beside them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)


def pcie_loop(runner, batches, seconds, sync):
    """bench.py timed_pcie, run for at least `seconds`: frames per second of the loop"""
    n = len(batches)
    B = batches[0][0].shape[0]

    def clip():
        for t in range(n):
            _, lab = runner.step(t, batches[t], n)
            runner.prefetch(batches[(t + 1) % n])
            host = lab.asnumpy()
        return host
    sync()
    t0 = time.perf_counter()
    clips = 0
    while True:
        last = clip()
        clips += 1
        if time.perf_counter() - t0 >= seconds:
            break
    sync()
    el = time.perf_counter() - t0
    assert last.shape[0] == B
    return clips * n * B / el


def kernel_alone(model, n, H, W, means, iters=40):
    """device-event time of the conversion of n resident H x W frames into `data` at step == 1, through the library's compute stream"""
    import torch
    dev = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(model.ctx.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    args = (n, H, W, 3 * W, means, H, W, 1.0, H, W)
    for _ in range(3):
        model.write_u8_device("data", dev.data_ptr(), *args)
    model.ctx.sync()
    best, total, train = None, 0.0, 20
    for _ in range(iters // train * 5):      # trains of back-to-back launches between one event pair (a 10 us kernel is launch-bound alone)
        e0.record(stream)
        for _ in range(train):
            model.write_u8_device("data", dev.data_ptr(), *args)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / train
        total += ms
        best = ms if best is None else min(best, ms)
    iters = iters // train * 5
    nbytes = n * (3 * H * W + 12 * H * W)
    return {"n": n, "ms_mean": total / iters, "ms_best": best, "bytes": nbytes, "GBps_mean": nbytes / (total / iters) / 1e6, "GBps_best": nbytes / best / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--interval", type=int, default=5)
    ap.add_argument("--size", default="1024x2048")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from accel_amd import demo, mx, runtime
    from accel_amd.config.config import config, update_config
    from accel_amd.utils import image, synth
    update_config(os.path.join(ROOT, "tests", "golden", "dff_deeplab_vid_demo.yaml"))
    H, W = [int(v) for v in a.size.split("x")]
    config.SCALES[0] = (H, W)
    means = config.network.PIXEL_MEANS
    arg, aux = synth.model_params("18", H, W, config)
    lines, record = [], {"size": a.size, "interval": a.interval, "seconds": a.seconds, "repeats": a.repeats, "batches": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # (c) the host path, one frame at a time on one thread (what a live pipeline would run per frame)
    frame = synth.make_clip(H, W, 1)[0]
    host_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        tensor = image.transform(image.resize(frame, H, W, stride=config.network.IMAGE_STRIDE)[0], means).astype(np.float32)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert tensor.shape == (1, 3, H, W)
    record["host_ms_per_frame"] = host_ms
    say("(c) host transform(resize(frame)) -> fp32, %s: %.2f ms per frame (median of 5; %.2f .. %.2f)"
        % (a.size, float(np.median(host_ms)), min(host_ms), max(host_ms)))

    for B in a.batches:
        model = runtime.Model(runtime.Context(0))
        runner = demo.ClipRunner("18", config, arg, aux, (H, W), model=model, batch=B)
        clips = [synth.make_clip(H, W, a.interval, seed=20260929 + b) for b in range(B)]
        u8 = [np.stack([c[t] for c in clips]) for t in range(a.interval)]
        pinned = mx.cpu_pinned()
        f32 = [mx.nd.array(np.concatenate([image.transform(f, means) for f in u8[t]]).astype(np.float32), ctx=pinned) for t in range(a.interval)]
        raw = [mx.nd.raw_frames(u8[t], config, ctx=pinned) for t in range(a.interval)]
        zero = mx.nd.array(np.zeros((B, 2048, 1, 1), np.float32))
        batches = {"fp32": [[f32[t], f32[t - 1] if t else f32[0], zero] for t in range(a.interval)],
                   "uint8": [[raw[t], raw[t - 1] if t else raw[0], zero] for t in range(a.interval)]}
        sync = model.ctx.sync
        for kind in ("fp32", "uint8"):      # warm both
            pcie_loop(runner, batches[kind], 0.0, sync)
            pcie_loop(runner, batches[kind], 0.0, sync)
        rates = {"fp32": [], "uint8": []}
        for _ in range(a.repeats):          # alternate
            for kind in ("fp32", "uint8"):
                rates[kind].append(pcie_loop(runner, batches[kind], a.seconds, sync))
        assert all(r._host is None for r in raw), "the uint8 route built an fp32 image on the host"
        for tag, kind in (("(a)", "fp32"), ("(b)", "uint8")):
            v = rates[kind]
            say("%s %d clip(s) per call, %s page-locked frames: %.1f frames/s (median of %d; %.1f .. %.1f, spread %.1f)"
                % (tag, B, kind, float(np.median(v)), len(v), min(v), max(v), max(v) - min(v)))
        k = kernel_alone(model, B, H, W, means)
        say("(d) kernel alone, %d frame(s) of %s at step 1: %.1f us mean / %.1f us best per launch, %.0f / %.0f GB/s over %.1f MB"
            % (B, a.size, k["ms_mean"] * 1e3, k["ms_best"] * 1e3, k["GBps_mean"], k["GBps_best"], k["bytes"] / 1e6))
        record["batches"][str(B)] = {"fp32_fps": rates["fp32"], "uint8_fps": rates["uint8"], "kernel": k}
        del f32, raw, batches
        model.ctx.sync()
        model.close()
        model.ctx.close()
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
