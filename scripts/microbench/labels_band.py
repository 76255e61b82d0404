"""What the trimap kernels (csrc/labels_band.hip) cost, beside the whole-frame confusion matrix they split and beside the route they replace:

    python scripts/microbench/labels_band.py [--frames 8 1] [--train 100] [--rounds 5] [--repeats 3] [--host 3] [--out FILE]

Label maps of 1024x2048 resident in HBM (`labels` of a model, written once) against ground truth of the same size resident in HBM, at the identity
geometry, --frames frames per launch.  Both hold 32 x 32 blocks of one class -- what a segmentation looks like to the kernels -- at other places.  In
the same process, alternating:
    hist_add                 accel_model_hist_add: 2 bytes read per source pixel
    band_hist_add 1,2,4,8    accel_model_band_hist_add with widths (1, 2, 4, 8): the same 2 bytes from HBM, the ground truth about 2.25 times from cache
    band_hist_add 16         the same with widths (16,): the largest halo, about 4.5 times from cache
Device-event time around a train of --train back-to-back launches on the library's compute stream, divided by the train (`trains` of
scripts/microbench/yuv.py); --repeats times --rounds trains each.
accel_boundary_distance takes and returns HOST arrays: it is timed with the host clock around the whole call, upload and download included (--host
times), at cap 8 and 16; the kernel alone, with the maps resident, is NOT measured here.
The route the band kernel replaces: the labels to the host (accel_model_labels_to_source), then utils.image.boundary_distance_host and the bincount of
band_hist_host in numpy; host clock, --host times, for one frame."""
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

from labels_summary import content, labels_model      # noqa: E402
from yuv import trains      # noqa: E402

NCLS = 19
WIDTHS = {"band_hist_add 1,2,4,8": (1, 2, 4, 8), "band_hist_add 16": (16,)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[8, 1])
    ap.add_argument("--train", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import runtime
    from accel_amd.utils import image
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
    for n in a.frames:
        m = labels_model(ctx, n, H, W)
        labels = content("blocks", n, H, W, 1)
        truth = np.ascontiguousarray(content("blocks", n, H + 32, W + 32, 2)[:, 13:13 + H, 7:7 + W])      # other blocks, at another phase
        m.write("labels", labels)
        gt = torch.from_numpy(truth).cuda()
        torch.cuda.synchronize()
        launches = {"hist_add": lambda: m.hist_add_device(gt.data_ptr(), n, H, W, W, H, W, NCLS)}
        # the kernels under the clock compute what the specification says (one frame is enough here; the tests hold every case)
        for name, widths in WIDTHS.items():
            one = labels_model(ctx, 1, H, W)
            one.write("labels", labels[:1])
            one.band_hist_add_device(gt.data_ptr(), 1, H, W, W, H, W, NCLS, widths)
            assert np.array_equal(one.band_hist_read(NCLS, len(widths)), image.band_hist_host(labels[:1], H, W, truth[:1], NCLS, widths)), name
            one.close()
        ms = {}
        for name in launches.keys() | WIDTHS.keys():
            ms[name] = []
        for _ in range(a.repeats):
            for name in ("hist_add",) + tuple(WIDTHS):
                if name in WIDTHS:      # one accumulator, one set of widths at a time: cleared between the two
                    m.band_hist_read(NCLS, len(WIDTHS[name]), clear=True)
                    widths = WIDTHS[name]
                    fn = lambda: m.band_hist_add_device(gt.data_ptr(), n, H, W, W, H, W, NCLS, widths)
                else:
                    fn = launches[name]
                for _ in range(3):
                    fn()
                ctx.sync()
                ms[name] += trains(m, fn, a.rounds, a.train)[0]
                if name in WIDTHS:
                    m.band_hist_read(NCLS, len(WIDTHS[name]), clear=True)
        m.hist_read(NCLS, clear=True)
        tag = "%dx%d n%d blocks" % (H, W, n)
        record["ms"][tag] = ms
        med = {}
        for name in ("hist_add",) + tuple(WIDTHS):
            v = np.asarray(ms[name]) * 1e3
            med[name] = float(np.median(v))
            say("%s, %s: min %.2f us, median %.2f us per launch = %.2f us per frame (%d trains of %d; max %.2f, spread %.1f %% of the median); "
                "%.0f GB/s over 2 nominal bytes per source pixel"
                % (tag, name, v.min(), med[name], med[name] / n, len(v), a.train, v.max(), 100.0 * (v.max() - v.min()) / med[name],
                   2.0 * n * H * W / med[name] / 1e3))
        for name in WIDTHS:
            r = np.asarray(ms[name]) / np.asarray(ms["hist_add"])
            say("%s: %s / hist_add = %.2f (medians); train by train %.2f .. %.2f" % (tag, name, med[name] / med["hist_add"], r.min(), r.max()))
        if n == 1:
            for cap in (8, 16):
                t = []
                for _ in range(a.host + 1):
                    t0 = time.perf_counter()
                    d = ctx.boundary_distance(truth, cap)
                    t.append((time.perf_counter() - t0) * 1e3)
                t = t[1:]
                assert np.array_equal(d, image.boundary_distance_host(truth, cap))
                say("%s: accel_boundary_distance at cap %d, host arrays in and out, takes %.2f ms per call (median of %d; min %.2f): allocation, upload, "
                    "kernel and download" % (tag, cap, float(np.median(t)), len(t), min(t)))
                record["ms"][tag + " distance cap %d" % cap] = t
            for name, widths in WIDTHS.items():
                t = []
                for _ in range(a.host):
                    t0 = time.perf_counter()
                    src = m.labels_to_source(1, H, W, H, W)
                    image.band_hist_host(src, H, W, truth, NCLS, widths)
                    t.append((time.perf_counter() - t0) * 1e3)
                say("%s: the host route for widths %s (labels to the host, boundary_distance_host, band_hist_host) takes %.1f ms per frame (median of "
                    "%d; min %.1f)" % (tag, widths, float(np.median(t)), len(t), min(t)))
                record["ms"][tag + " host " + name] = t
        del gt
        m.close()
    ctx.close()
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
