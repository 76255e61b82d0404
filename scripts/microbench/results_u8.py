"""What finishing a frame on the GPU costs and saves (accel_model_hist_add / _hist_read / _labels_to_source / _labels_colour,
csrc/results_u8.hip): Accel-18 at 1024x2048, kf=5, one clip per call and 8 clips per call, through the loop of bench.py's timed_pcie
(step, prefetch of the next frame, label fetch) with the evaluation of the frame behind it.

    python scripts/microbench/results_u8.py [--batches 1 8] [--seconds 1.0] [--repeats 3] [--out profiles/results_u8.md]

  (a)  frames/s of the present host route: asnumpy of the labels, then demo.fast_hist against host ground truth
  (b)  frames/s with hist_add per call (host ground truth through the staging buffer) and one hist_read at the end
  (b') the same with the ground truth resident in HBM (hist_add_device): nothing but the launch per call
  (k)  each kernel alone: device-event time over trains of 20 launches and GB/s over its algorithmic bytes, against the 6.3 TB/s achievable
       HBM rate of DESIGN.md section 3 -- hist n*(HW + hw), source n*(hw + hw), colour n*(hw + 3hw [+ 3hw frame]) -- at the identity and
       for a 720 x 1280 source; the histogram on a uniform-random map and on the single-pair (worst-contention) map
(a), (b), (b') alternate in one process, all warmed, each timed for at least --seconds, --repeats times; the spread is printed beside them.
The matrices of (a) and (b) are compared at the end: they must be equal."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12


def loop(runner, batches, seconds, sync, finish):
    """bench.py timed_pcie with `finish(labels handle, frame index)` in the place of the label fetch: (frames per second, frames run)"""
    n = len(batches)
    B = batches[0][0].shape[0]
    sync()
    t0 = time.perf_counter()
    clips = 0
    while True:
        for t in range(n):
            _, lab = runner.step(t, batches[t], n)
            runner.prefetch(batches[(t + 1) % n])
            finish(lab, t)
        clips += 1
        if time.perf_counter() - t0 >= seconds:
            break
    sync()
    return clips * n * B / (time.perf_counter() - t0), clips


def train_ms(ctx, launch, trains=10, train=20):
    """device-event milliseconds per launch: trains of back-to-back launches between one event pair on the library's compute stream"""
    import torch
    stream = torch.cuda.ExternalStream(ctx.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        launch()
    ctx.sync()
    ms = []
    for _ in range(trains):
        e0.record(stream)
        for _ in range(train):
            launch()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / train)
    return float(np.mean(ms)), float(min(ms))


def kernels_alone(ctx, n, H, W, say):
    import torch
    from accel_amd import runtime
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=labels bytes=%d\nmeta labels_n=%d labels_h=%d labels_w=%d\n" % (n * H * W, n, H, W))
    pal = np.random.default_rng(0).integers(0, 256, 768, dtype=np.uint8)
    out = {}
    maps = {"random": np.random.default_rng(1).integers(0, 19, (n, H, W), dtype=np.uint8), "single pair": np.full((n, H, W), 5, np.uint8)}
    for (h, w, out_h, out_w) in ((H, W, H, W), (720, 1280, 1024, 1820)):
        if out_h > H or out_w > W:
            continue
        gts = {"random": torch.randint(0, 19, (n, h, w), dtype=torch.uint8, device="cuda"), "single pair": torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")}
        dst = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        dst3 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
        frame = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        tag = "%dx%d -> %dx%d" % (out_h, out_w, h, w)
        for kind in ("random", "single pair"):
            m.write("labels", maps[kind])
            mean, best = train_ms(ctx, lambda: m.hist_add_device(gts[kind].data_ptr(), n, h, w, w, out_h, out_w, 19))
            m.hist_read(19, clear=True)
            nbytes = n * (out_h * out_w + h * w)
            out["hist %s %s" % (kind, tag)] = (mean, best, nbytes)
        m.write("labels", maps["random"])
        out["source %s" % tag] = train_ms(ctx, lambda: m.labels_to_source_device(dst.data_ptr(), n, out_h, out_w, h, w, w)) + (n * 2 * h * w,)
        out["colour %s" % tag] = train_ms(ctx, lambda: m.labels_colour_device(dst3.data_ptr(), n, out_h, out_w, h, w, 3 * w, pal)) + (n * 4 * h * w,)
        out["colour + frame %s" % tag] = train_ms(ctx, lambda: m.labels_colour_device(dst3.data_ptr(), n, out_h, out_w, h, w, 3 * w, pal, frame.data_ptr(),
                                                                                       3 * w, 128)) + (n * 7 * h * w,)
        ctx.sync()
    for name, (mean, best, nbytes) in out.items():
        say("(k) %d map(s), %s: %.1f us mean / %.1f us best per launch, %.0f / %.0f GB/s over %.1f MB = %.2f of the achievable HBM rate"
            % (n, name, mean * 1e3, best * 1e3, nbytes / mean / 1e6, nbytes / best / 1e6, nbytes / 1e6, nbytes / (best * 1e-3) / HBM_ACHIEVABLE))
    m.close()
    return {k: {"ms_mean": v[0], "ms_best": v[1], "bytes": v[2]} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--interval", type=int, default=5)
    ap.add_argument("--size", default="1024x2048")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import demo, mx, runtime
    from accel_amd.config.config import config, update_config
    from accel_amd.utils import synth
    update_config(os.path.join(ROOT, "tests", "golden", "dff_deeplab_vid_demo.yaml"))
    H, W = [int(v) for v in a.size.split("x")]
    config.SCALES[0] = (H, W)
    arg, aux = synth.model_params("18", H, W, config)
    lines, record = [], {"size": a.size, "interval": a.interval, "seconds": a.seconds, "repeats": a.repeats, "batches": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B in a.batches:
        ctx = runtime.Context(0)
        model = runtime.Model(ctx)
        runner = demo.ClipRunner("18", config, arg, aux, (H, W), model=model, batch=B)
        clips = [synth.make_clip(H, W, a.interval, seed=20260929 + b) for b in range(B)]
        pinned = mx.cpu_pinned()
        raw = [mx.nd.raw_frames(np.stack([c[t] for c in clips]), config, ctx=pinned) for t in range(a.interval)]
        zero = mx.nd.array(np.zeros((B, 2048, 1, 1), np.float32))
        batches = [[raw[t], raw[t - 1] if t else raw[0], zero] for t in range(a.interval)]
        rng = np.random.default_rng(B)
        gt = [rng.integers(0, 19, (B, H, W), dtype=np.uint8) for _ in range(a.interval)]
        gt_dev = [torch.from_numpy(g).cuda() for g in gt]
        torch.cuda.synchronize()
        host_hist = np.zeros((19, 19), np.int64)
        calls = {"a": 0, "b": 0}

        def host_route(lab, t):
            host_hist[...] += demo.fast_hist(lab.asnumpy().reshape(-1), gt[t].reshape(-1), 19)
            calls["a"] += 1

        def gpu_route(lab, t):
            model.hist_add(gt[t], H, W, 19)
            calls["b"] += 1

        def gpu_route_resident(lab, t):
            model.hist_add_device(gt_dev[t].data_ptr(), B, H, W, W, H, W, 19)

        routes = (("(a)", "host: asnumpy + fast_hist", host_route), ("(b)", "GPU: hist_add, host ground truth", gpu_route),
                  ("(b')", "GPU: hist_add, ground truth in HBM", gpu_route_resident))
        for _, _, fn in routes:             # warm all
            loop(runner, batches, 0.0, ctx.sync, fn)
        model.hist_read(19, clear=True)
        host_hist[...] = 0
        calls.update(a=0, b=0)
        rates = {tag: [] for tag, _, _ in routes}
        gpu_hist = np.zeros((19, 19), np.int64)
        for _ in range(a.repeats):          # alternate
            for tag, _, fn in routes:
                rates[tag].append(loop(runner, batches, a.seconds, ctx.sync, fn)[0])
                if tag == "(b)":
                    gpu_hist += model.hist_read(19, clear=True).astype(np.int64)      # the one read at the end of the route
                elif tag == "(b')":
                    model.hist_read(19, clear=True)
        # every call of a route sees the same frames: the two matrices are equal per call
        same = calls["a"] and calls["b"] and np.array_equal(host_hist * calls["b"], gpu_hist * calls["a"])
        for tag, what, _ in routes:
            v = rates[tag]
            say("%s %d clip(s) per call, %s: %.1f frames/s (median of %d; %.1f .. %.1f, spread %.1f)"
                % (tag, B, what, float(np.median(v)), len(v), min(v), max(v), max(v) - min(v)))
        say("    confusion matrices of (a) and (b) per call: %s" % ("equal" if same else "DIFFERENT"))
        k = kernels_alone(ctx, B, H, W, say)
        record["batches"][str(B)] = {"fps": rates, "kernels": k, "matrices_equal": bool(same)}
        del raw, batches, gt_dev
        ctx.sync()
        model.close()
        ctx.close()
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
