"""What the connected components of finished frames (csrc/labels_components.hip) cost, beside the summary of the same frames -- the yardstick every
result kernel here is given -- and beside the route they replace:

    python scripts/microbench/labels_components.py [--frames 8 1] [--train 50] [--rounds 5] [--repeats 3] [--host 3] [--kinds blocks one noise]
                                                   [--sources 1024x2048 2160x3840] [--no-summary] [--out FILE]

Label maps of 1024x2048 resident in HBM (`labels` of a model, written once), taken at the identity (a 1024x2048 source) and to a 2160x3840 source,
--frames frames per launch, for three kinds of content: `blocks` (32 x 32 blocks of one class: what a segmentation looks like to the kernels), `one`
(one class everywhere: every pixel ends up under ONE root, the contention case) and `noise` (an independent class per pixel: the worst case, with
count far above max_components).  In the same process, alternating:
    components         accel_model_labels_components, connectivity 8, min_area 1, max_components 1024, count / comp / sums into caller-owned HBM
    components + ids   the same with the per-pixel object index
    summary            accel_model_labels_summary, track = 0, stats and box into caller-owned HBM
Device-event time around a train of --train back-to-back launches on the library's compute stream, divided by the train (`trains` of
scripts/microbench/yuv.py); --repeats times --rounds trains each.  A launch of `components` is seven or eight kernels; their split comes from a run of
this script under `rocprofv3 --kernel-trace --stats` (with --no-summary --host 0), never from the figures of this run.
The route the call replaces: accel_model_labels_to_source to the host, then scipy.ndimage.label per present class and find_objects; host clock,
--host times (once for `noise`), for one frame."""
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
from labels_summary import labels_model      # noqa: E402

NCLS = 19
RECORDS = 1024


def content(kind, n, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, NCLS, (n, H, W), dtype=np.uint8)
    if kind == "one":
        return np.full((n, H, W), 7, np.uint8)
    small = rng.integers(0, NCLS, (n, H // 32, W // 32), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, 32, axis=1), 32, axis=2))


def host_route(m, H, W, h, w):
    """one frame's labels at the source size on the host, then scipy's labelling per present class and the boxes"""
    from scipy import ndimage
    src = m.labels_to_source(1, H, W, h, w)[0]
    eight = ndimage.generate_binary_structure(2, 2)
    found = 0
    for k in np.unique(src):
        if k >= NCLS:
            continue
        lab, count = ndimage.label(src == k, structure=eight)
        ndimage.find_objects(lab)
        found += count
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[8, 1])
    ap.add_argument("--kinds", nargs="*", default=["blocks", "one", "noise"])
    ap.add_argument("--sources", nargs="*", default=["1024x2048", "2160x3840"])
    ap.add_argument("--train", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host", type=int, default=3)
    ap.add_argument("--no-summary", dest="summary", action="store_false")
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
    for h, w in (tuple(int(v) for v in src.split("x")) for src in a.sources):
        for n in a.frames:
            for kind in a.kinds:
                m = labels_model(ctx, n, H, W)
                m.write("labels", content(kind, n, H, W, 1))
                count = torch.zeros(n, dtype=torch.int32, device="cuda")
                comp = torch.zeros(n * RECORDS * 8, dtype=torch.int32, device="cuda")
                sums = torch.zeros(n * RECORDS * 2, dtype=torch.int64, device="cuda")
                ids = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
                stats = torch.zeros(n * NCLS * 3, dtype=torch.int64, device="cuda")
                box = torch.zeros(n * NCLS * 4, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ptrs = dict(count_ptr=count.data_ptr(), comp_ptr=comp.data_ptr(), sums_ptr=sums.data_ptr())
                launches = {
                    "components": lambda: m.labels_components_device(n, H, W, h, w, NCLS, max_components=RECORDS, **ptrs),
                    "components + ids": lambda: m.labels_components_device(n, H, W, h, w, NCLS, max_components=RECORDS, ids_ptr=ids.data_ptr(), **ptrs),
                }
                if a.summary:
                    launches["summary"] = lambda: m.labels_summary_device(n, H, W, h, w, NCLS, False, stats.data_ptr(), box.data_ptr())
                for fn in launches.values():
                    for _ in range(3):
                        fn()
                ctx.sync()
                # the kernels under the clock compute what the specification says (one small frame is enough here; the tests hold every case)
                if (h, w) == (H, W) and n == 1 and kind != "noise":
                    want = image.labels_components_host(m.read("labels", (n, H, W), np.uint8)[:1], H, W, h, w, NCLS, max_components=RECORDS, ids=True)
                    assert np.array_equal(count.cpu().numpy()[:1], want[0])
                    assert np.array_equal(comp.cpu().numpy().reshape(n, RECORDS, 8)[:1], want[1])
                    assert np.array_equal(sums.cpu().numpy().view(np.uint64).reshape(n, RECORDS, 2)[:1], want[2])
                    assert np.array_equal(ids.cpu().numpy()[:1], want[3])
                found = int(count.cpu().numpy()[0])
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
                    say("%s, %s: min %.1f us, median %.1f us per launch = %.1f us per frame (%d trains of %d; max %.1f, spread %.1f %% of the median; "
                        "host enqueue %.1f us per launch); %d components in frame 0"
                        % (tag, k, v.min(), med[k], med[k] / n, len(v), a.train, v.max(), 100.0 * (v.max() - v.min()) / med[k],
                           float(np.median(host[k])) * 1e3, found))
                if a.summary:
                    say("%s: components / summary = %.2f, with ids %.2f (medians)" % (tag, med["components"] / med["summary"],
                                                                                      med["components + ids"] / med["summary"]))
                if n == 1 and a.host:
                    t = []
                    for _ in range(1 if kind == "noise" else a.host):
                        t0 = time.perf_counter()
                        objects = host_route(m, H, W, h, w)
                        t.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    for _ in range(10):
                        m.labels_components(1, H, W, h, w, NCLS, max_components=RECORDS)
                    call = (time.perf_counter() - t0) * 1e3 / 10
                    assert objects == found, (objects, found)
                    say("%s: the host route (labels to the host, scipy.ndimage.label per class, find_objects) takes %.1f ms per frame (median of %d; "
                        "min %.1f) for %d objects; labels_components with host destinations %.3f ms per call, wait included"
                        % (tag, float(np.median(t)), len(t), min(t), objects, call))
                    record["ms"][tag + " host"] = t
                del count, comp, sums, ids, stats, box
                m.close()
    ctx.close()
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
