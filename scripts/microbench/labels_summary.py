"""What the summary of finished frames (csrc/labels_summary.hip) costs, beside the two kernels of the same family that bracket it on bytes moved and
beside the route it replaces:

    python scripts/microbench/labels_summary.py [--frames 8 1] [--train 200] [--rounds 5] [--repeats 3] [--host 5] [--out FILE]

Label maps of 1024x2048 resident in HBM (`labels` of a model, written once), summarised at the identity (a 1024x2048 source) and for a 2160x3840
source, --frames frames per launch, for two kinds of content: `blocks` (32 x 32 blocks of one class: what a segmentation looks like to the kernel,
runs of equal pixels) and `noise` (independent classes per pixel: every pixel ends a run, the worst case).  In the same process, alternating:
    summary            accel_model_labels_summary, track = 0, stats and box into caller-owned HBM: 1 byte read per source pixel
    summary tracked    the same with track = 1 and trans: the kept map read and written in the same pass: 3 bytes per source pixel
    hist_add           accel_model_hist_add against ground truth resident in HBM: 2 bytes read per source pixel
    to_source          accel_model_labels_to_source into caller-owned HBM: 1 byte read and 1 written per source pixel
Device-event time around a train of --train back-to-back launches on the library's compute stream, divided by the train (`trains` of
scripts/microbench/yuv.py); --repeats times --rounds trains each.  The bytes are nominal: source pixels times the bytes per pixel above (an enlarged
map is re-read from cache).
The route the call replaces: accel_model_labels_to_source to the host, then np.bincount and the box search per class in numpy; host clock, --host
times, for one frame."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yuv import trains      # noqa: E402

NCLS = 19
BYTES = {"summary": 1, "summary tracked": 3, "hist_add": 2, "to_source": 2}


def labels_model(ctx, n, H, W):
    from accel_amd import runtime
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=labels bytes=%d\nmeta labels_n=%d labels_h=%d labels_w=%d\n"
                     % ((n * H * W + 255) // 256 * 256, n, H, W))
    return m


def content(kind, n, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, NCLS, (n, H, W), dtype=np.uint8)
    small = rng.integers(0, NCLS, (n, H // 32, W // 32), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, 32, axis=1), 32, axis=2))


def host_route(m, n, H, W, h, w):
    """labels at the source size on the host, then areas, coordinate sums and boxes in numpy"""
    src = m.labels_to_source(n, H, W, h, w)
    out = []
    xs, ys = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    for f in range(n):
        area = np.bincount(src[f].reshape(-1), minlength=256)[:NCLS]
        for k in np.nonzero(area)[0]:
            mask = src[f] == k
            cols, rows = mask.sum(axis=0), mask.sum(axis=1)
            cx, cy = np.nonzero(cols)[0], np.nonzero(rows)[0]
            out.append((int(area[k]), int((cols * xs).sum()), int((rows * ys).sum()), cx[0], cy[0], cx[-1], cy[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[8, 1])
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import runtime
    lines, record = [], {"train": a.train, "rounds": a.rounds, "repeats": a.repeats, "ms": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown (not a git checkout)"
    say("box: %s, torch %s; tree: %s; command: python %s" % (torch.cuda.get_device_name(0), torch.__version__, commit, " ".join(sys.argv)))
    ctx = runtime.Context(0)
    H, W = 1024, 2048
    for h, w in ((1024, 2048), (2160, 3840)):
        for n in a.frames:
            for kind in ("blocks", "noise"):
                m = labels_model(ctx, n, H, W)
                m.write("labels", content(kind, n, H, W, 1))
                gt = torch.from_numpy(content(kind, n, h // 8 * 8 + 32, w, 2)[:, :h]).contiguous().cuda()       # other blocks than the labels
                dst = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
                stats = torch.zeros(n * NCLS * 3, dtype=torch.int64, device="cuda")
                box = torch.zeros(n * NCLS * 4, dtype=torch.int32, device="cuda")
                trans = torch.zeros(n * NCLS * NCLS, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                launches = {
                    "summary": lambda: m.labels_summary_device(n, H, W, h, w, NCLS, False, stats.data_ptr(), box.data_ptr()),
                    "summary tracked": lambda: m.labels_summary_device(n, H, W, h, w, NCLS, True, stats.data_ptr(), box.data_ptr(), trans.data_ptr()),
                    "hist_add": lambda: m.hist_add_device(gt.data_ptr(), n, h, w, w, H, W, NCLS),
                    "to_source": lambda: m.labels_to_source_device(dst.data_ptr(), n, H, W, h, w, w),
                }
                for fn in launches.values():
                    for _ in range(5):
                        fn()
                ctx.sync()
                # the kernel under the clock computes what the specification says (one frame is enough here; the tests hold every case)
                from accel_amd.utils import image
                want = image.labels_summary_host(m.read("labels", (n, H, W), np.uint8)[:1], H, W, h, w, NCLS)
                assert np.array_equal(stats.cpu().numpy().view(np.uint64).reshape(n, NCLS, 3)[:1], want[0])
                assert np.array_equal(box.cpu().numpy().reshape(n, NCLS, 4)[:1], want[1])
                ms, host = {k: [] for k in launches}, {k: [] for k in launches}
                for _ in range(a.repeats):
                    for k, fn in launches.items():
                        dev, enq = trains(m, fn, a.rounds, a.train)
                        ms[k] += dev
                        host[k] += enq
                ctx.sync()
                tag = "%dx%d n%d %s" % (h, w, n, kind)
                record["ms"][tag] = ms
                med = {}
                for k in launches:
                    v = np.asarray(ms[k]) * 1e3
                    med[k] = float(np.median(v))
                    nbytes = n * h * w * BYTES[k]
                    say("%s, %s: min %.2f us, median %.2f us per launch = %.2f us per frame (%d trains of %d; max %.2f, spread %.1f %% of the median; "
                        "host enqueue %.2f us per launch); %.0f GB/s over %d nominal byte(s) per source pixel"
                        % (tag, k, v.min(), med[k], med[k] / n, len(v), a.train, v.max(), 100.0 * (v.max() - v.min()) / med[k],
                           float(np.median(host[k])) * 1e3, nbytes / med[k] / 1e3, BYTES[k]))
                say("%s: summary / hist_add = %.3f, summary tracked / hist_add = %.3f, summary / to_source = %.3f (medians)"
                    % (tag, med["summary"] / med["hist_add"], med["summary tracked"] / med["hist_add"], med["summary"] / med["to_source"]))
                if n == 1:
                    t = []
                    for _ in range(a.host):
                        t0 = time.perf_counter()
                        host_route(m, 1, H, W, h, w)
                        t.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    for _ in range(20):
                        m.labels_summary(1, H, W, h, w, NCLS)
                    call = (time.perf_counter() - t0) * 1e3 / 20
                    say("%s: the host route (labels to the host, bincount, box search) takes %.1f ms per frame (median of %d; min %.1f); "
                        "labels_summary with host destinations %.3f ms per call, wait included"
                        % (tag, float(np.median(t)), len(t), min(t), call))
                    record["ms"][tag + " host"] = t
                del gt, dst, stats, box, trans
                m.close()
    ctx.close()
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
