"""What the per-pixel confidence of a finished frame costs (accel_model_confidence, csrc/confidence.hip) against the host route it replaces
(`logits.asnumpy()` plus utils.image.confidence_host), on a model that owns a `logits` buffer of n x 19 x 1024 x 2048 filled with seeded
scores -- no network is run: the kernel's time depends on the shape, and through the histogram on how the levels are spread, not on whose
logits they are.

    python scripts/microbench/confidence.py [--frames 8] [--size 1024x2048] [--host-frames 1] [--out profiles/confidence.md]

  (k) the kernel alone into HBM destinations: device-event time over trains of 20 launches, GB/s over the scores it reads (ncls * 4 bytes per
      map pixel touched: 159 MB per 1024x2048 frame) and over read + written bytes, against the 6.3 TB/s achievable HBM rate of DESIGN.md
      section 3 -- conf alone, conf + hist, all four outputs; at the identity geometry and for a 720 x 1280 source of a 1024 x 1820 region;
      on scores of standard deviation 1 (levels spread over the bins) and 30 (nearly every pixel saturated: one bin takes almost all)
  (m) the model-level call with host destinations (kernel + the copy of the results + the wait), wall clock
  (h) the host route on --host-frames frames: asnumpy of the logits, then confidence_host, wall clock per frame
The GPU results of (m) are compared with (h): they must be equal."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
NCLS = 19


def train_ms(ctx, launch, trains=5, train=20):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="1024x2048")
    ap.add_argument("--host-frames", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import runtime
    from accel_amd.utils import image
    H, W = [int(v) for v in a.size.split("x")]
    n = a.frames
    lines, record = [], {"size": a.size, "frames": n, "kernel": {}, "model": {}, "host": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = runtime.Context(0)
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=logits bytes=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d\n"
                     % (n * NCLS * H * W * 4, n, NCLS, H, W))
    geometries = [(H, W, H, W)]
    if H >= 1024 and W >= 1820:
        geometries.append((720, 1280, 1024, 1820))
    one = np.random.default_rng(1).standard_normal((1, NCLS, H, W)).astype(np.float32)
    equal = True
    for sigma in (1.0, 30.0):
        scores = np.ascontiguousarray(np.broadcast_to(one * np.float32(sigma), (n, NCLS, H, W)))      # the same frame n times: time does not care
        m.write("logits", scores)
        for (h, w, out_h, out_w) in geometries:
            tag = "sigma %g, %dx%d -> %dx%d" % (sigma, out_h, out_w, h, w)
            conf = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
            second = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
            margin = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
            hist = torch.empty((n, 256), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            touched = n * NCLS * 4 * (out_h * out_w if (h, w) == (out_h, out_w) else min(h, out_h) * min(w, out_w))
            variants = (("conf", dict(conf_ptr=conf.data_ptr(), conf_pitch=w), n * h * w),
                        ("conf + hist", dict(conf_ptr=conf.data_ptr(), conf_pitch=w, hist_ptr=hist.data_ptr()), n * h * w),
                        ("all four", dict(conf_ptr=conf.data_ptr(), conf_pitch=w, margin_ptr=margin.data_ptr(), margin_pitch=4 * w,
                                          second_ptr=second.data_ptr(), second_pitch=w, hist_ptr=hist.data_ptr()), n * 6 * h * w))
            for name, kw, written in variants:
                mean, best = train_ms(ctx, lambda: m.confidence_device(n, out_h, out_w, h, w, **kw))
                say("(k) %d frame(s), %s, %s: %.1f us mean / %.1f us best per launch; scores read %.1f MB = %.0f GB/s (%.2f of the achievable "
                    "HBM rate), read + written %.0f GB/s" % (n, tag, name, mean * 1e3, best * 1e3, touched / 1e6, touched / best / 1e6,
                                                             touched / (best * 1e-3) / HBM_ACHIEVABLE, (touched + written) / best / 1e6))
                record["kernel"]["%s, %s" % (tag, name)] = {"ms_mean": mean, "ms_best": best, "scores_bytes": touched, "written_bytes": written}
            ctx.sync()
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = m.confidence(n, out_h, out_w, h, w)
                t.append(time.perf_counter() - t0)
            say("(m) %d frame(s), %s, all four to the host: %.2f ms per call (best of 3), %.2f ms per frame" % (n, tag, min(t) * 1e3, min(t) * 1e3 / n))
            record["model"][tag] = {"ms_per_call": min(t) * 1e3}
            k = max(1, min(a.host_frames, n))
            t0 = time.perf_counter()
            lg = m.read("logits", (n, NCLS, H, W))[:k]
            t1 = time.perf_counter()
            want = image.confidence_host(lg, out_h, out_w, h, w)
            t2 = time.perf_counter()
            say("(h) %s, host route: asnumpy of %d frame(s) of logits %.1f ms (all %d frames are fetched: %.1f ms per frame), confidence_host %.1f ms per "
                "frame" % (tag, n, (t1 - t0) * 1e3, n, (t1 - t0) * 1e3 / n, (t2 - t1) * 1e3 / k))
            record["host"][tag] = {"asnumpy_ms_per_frame": (t1 - t0) * 1e3 / n, "confidence_host_ms_per_frame": (t2 - t1) * 1e3 / k}
            same = all(np.array_equal(g[:k].view(np.uint32) if g.dtype == np.float32 else g[:k], x.view(np.uint32) if x.dtype == np.float32 else x)
                       for g, x in zip(got, want))
            equal = equal and same
            say("    results of (m) and (h): %s" % ("equal" if same else "DIFFERENT"))
            del conf, second, margin, hist
    record["equal"] = bool(equal)
    ctx.sync()
    m.close()
    ctx.close()
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
