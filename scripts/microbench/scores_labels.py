"""What source-size labels from interpolated scores cost (accel_model_scores_labels, csrc/scores_labels.hip) against the nearest rule on the
finished label map (accel_model_labels_to_source, csrc/results_u8.hip) and against the host route it replaces (`logits.asnumpy()` plus
utils.image.labels_interpolated_host), on models that own a `logits` and a `labels` buffer of --frames frames filled with seeded scores -- no
network is run: the kernel's time depends on the shapes, not on whose logits they are.

    python scripts/microbench/scores_labels.py [--frames 4] [--host-frames 1] [--out profiles/scores_labels.md]

Three geometries: 1024 x 2048 at the identity; a 720 x 1280 source of a 1024 x 1820 region of a 1024 x 1824 map; a 2160 x 3840 source of a
1024 x 2048 map.  --frames frames are finished per launch (blockIdx.z), so that with the default 4 the scores (4 x 159 MB) do not fit the
256 MiB Infinity Cache and a rate above HBM's cannot be the cache's; times are reported per frame.

  (k) the kernel alone into HBM: device-event time over trains of 20 launches; bytes are counted from the shapes -- the scores of the valid
      region a launch has to read once (ncls * 4 bytes per map pixel of the region that any source pixel taps) plus the labels it writes --
      and the rate is set against the 6.3 TB/s achievable HBM rate of DESIGN.md section 3
  (n) labels_to_source at the same geometry, the same way
  (m) the model-level call with a host destination (kernel + the copy of the labels + the wait), wall clock
  (h) the host route on --host-frames frames: asnumpy of the logits, then labels_interpolated_host, wall clock per frame
The labels of (m) are compared with (h): they must be equal."""
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
# (H, W, out_h, out_w, h, w)
GEOMETRIES = [(1024, 2048, 1024, 2048, 1024, 2048), (1024, 2048, 1024, 2048, 2160, 3840), (1024, 1824, 1024, 1820, 720, 1280)]


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
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--host-frames", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import runtime
    from accel_amd.utils import image
    n = a.frames
    lines, record = [], {"frames": n, "kernel": {}, "nearest": {}, "model": {}, "host": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = runtime.Context(0)
    equal = True
    models = {}
    for (H, W, out_h, out_w, h, w) in GEOMETRIES:
        if (H, W) not in models:
            for old in models.values():
                old.close()
            models.clear()
            m = runtime.Model(ctx)
            m.add_plan("op", "option graph=0 tune=0\npbuf name=logits bytes=%d\npbuf name=labels bytes=%d\n"
                             "meta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d labels_n=%d labels_h=%d labels_w=%d\n"
                             % (n * NCLS * H * W * 4, (n * H * W + 255) // 256 * 256, n, NCLS, H, W, n, H, W))
            one = np.random.default_rng(H * 4096 + W).standard_normal((1, NCLS, H, W)).astype(np.float32)
            scores = np.ascontiguousarray(np.broadcast_to(one, (n, NCLS, H, W)))          # the same frame n times: time does not care
            m.write("logits", scores)
            m.write("labels", np.argmax(scores, axis=1).astype(np.uint8))
            del scores
            models[(H, W)] = m
        m = models[(H, W)]
        tag = "%dx%d of %dx%d -> %dx%d" % (out_h, out_w, H, W, h, w)
        dst = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        # every map pixel of the region is tapped when the source is at least as large; a smaller source skips none either (its taps are
        # two adjacent pixels at a step below 2), so the whole region counts
        read = n * NCLS * 4 * out_h * out_w
        written = n * h * w
        mean, best = train_ms(ctx, lambda: m.scores_labels_device(dst.data_ptr(), n, out_h, out_w, h, w, w))
        say("(k) %s, interpolated: %.1f us mean / %.1f us best per frame; scores read %.1f MB + labels written %.1f MB per frame = %.0f GB/s "
            "(%.2f of the achievable HBM rate)" % (tag, mean * 1e3 / n, best * 1e3 / n, read / n / 1e6, written / n / 1e6, (read + written) / best / 1e6,
                                                   (read + written) / (best * 1e-3) / HBM_ACHIEVABLE))
        record["kernel"][tag] = {"ms_mean_per_frame": mean / n, "ms_best_per_frame": best / n, "read_bytes_per_frame": read // n,
                                 "written_bytes_per_frame": written // n}
        nread = n * (out_h * out_w if (h, w) == (out_h, out_w) else min(h, out_h) * min(w, out_w))
        mean, best = train_ms(ctx, lambda: m.labels_to_source_device(dst.data_ptr(), n, out_h, out_w, h, w, w))
        say("(n) %s, nearest (labels_to_source): %.1f us mean / %.1f us best per frame; %.1f MB read + %.1f MB written per frame = %.0f GB/s"
            % (tag, mean * 1e3 / n, best * 1e3 / n, nread / n / 1e6, written / n / 1e6, (nread + written) / best / 1e6))
        record["nearest"][tag] = {"ms_mean_per_frame": mean / n, "ms_best_per_frame": best / n}
        ctx.sync()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = m.scores_labels(n, out_h, out_w, h, w)
            t.append(time.perf_counter() - t0)
        say("(m) %s, %d frame(s) to the host: %.2f ms per call (best of 3), %.2f ms per frame" % (tag, n, min(t) * 1e3, min(t) * 1e3 / n))
        record["model"][tag] = {"ms_per_call": min(t) * 1e3}
        k = max(1, min(a.host_frames, n))
        t0 = time.perf_counter()
        lg = m.read("logits", (n, NCLS, H, W))[:k]
        t1 = time.perf_counter()
        want = image.labels_interpolated_host(lg, out_h, out_w, h, w)
        t2 = time.perf_counter()
        say("(h) %s, host route: asnumpy of %d frame(s) of logits %.1f ms (%.1f ms per frame), labels_interpolated_host %.1f ms per frame"
            % (tag, n, (t1 - t0) * 1e3, (t1 - t0) * 1e3 / n, (t2 - t1) * 1e3 / k))
        record["host"][tag] = {"asnumpy_ms_per_frame": (t1 - t0) * 1e3 / n, "labels_interpolated_host_ms_per_frame": (t2 - t1) * 1e3 / k}
        same = bool(np.array_equal(got[:k], want))
        equal = equal and same
        say("    labels of (m) and (h): %s" % ("equal" if same else "DIFFERENT (%d)" % int(np.count_nonzero(got[:k] != want))))
        del dst, lg, want, got
    record["equal"] = bool(equal)
    ctx.sync()
    for m in models.values():
        m.close()
    ctx.close()
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
