"""What the frame-change measure (csrc/frame_change.hip) costs, and what the adaptive key-frame decision costs in the clip loop:

    python scripts/microbench/frame_change.py [--size 1024x2048] [--frames 1 8] [--train 200] [--rounds 5] [--repeats 3]
                                              [--clip 10] [--passes 9] [--skip-loop] [--out FILE]

(a) the kernel: accel_model_frame_change on the `data` input of --frames frames resident in HBM, compared with a kept signature, results into
    caller-owned HBM (no host wait) -- beside accel_model_write(src_on_device=1) of the same tensor in the same process, the two alternating: an
    HBM copy that READS the same bytes (and writes them once more).  Device-event time around a train of --train back-to-back launches on the
    library's compute stream, divided by the train (`trains` of scripts/microbench/yuv.py); --repeats times --rounds trains each; the bytes are
    n x 3 x H x W x 4, the bytes the kernel reads (the signature words are 1 / 3072 of them at cell 32).
(b) the decision in the loop: Accel-18 at --size, a clip of --clip raw BGR frames in pinned memory, the demo's loop (step, prefetch of the next
    frame, fetch of the label map) per frame under KeySchedule.adaptive(share=1.0, max_interval=5) -- a share no frame can exceed, so the key
    frames are those of fixed(5) and the plans run are the same -- and under KeySchedule.fixed(5), the two alternating pass by pass over the
    same clip.  Host clock around a frame that ends in the fetch of its labels; the difference is the kernel, a 12-byte read-back per frame
    and the host wait it forces before the predictor is chosen."""
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

from yuv import input_model, trains      # noqa: E402


def kernel_part(a, ctx, say, record):
    import torch
    H, W = [int(v) for v in a.size.split("x")]
    cell, level_q = 32, 1024
    for n in a.frames:
        m = input_model(ctx, H, W, n)
        m.plans["op"].finalize()
        nbytes = n * 3 * H * W * 4
        src = [torch.empty((n, 3, H, W), dtype=torch.float32, device="cuda").uniform_(-120.0, 130.0) for _ in range(2)]
        changed = torch.zeros(n, dtype=torch.int32, device="cuda")
        sad = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        m.write_device("data", src[0].data_ptr(), nbytes)
        assert m.frame_change_device("data", n, H, W, cell, level_q) is False
        m.frame_keep()
        m.write_device("data", src[1].data_ptr(), nbytes)
        launches = {
            "frame_change": lambda: m.frame_change_device("data", n, H, W, cell, level_q, changed.data_ptr(), sad.data_ptr()),
            "write": lambda: m.write_device("data_key", src[1].data_ptr(), nbytes),
        }
        for fn in launches.values():
            for _ in range(5):
                fn()
        ctx.sync()
        ms, host = {k: [] for k in launches}, {k: [] for k in launches}
        for _ in range(a.repeats):
            for k, fn in launches.items():
                dev, enq = trains(m, fn, a.rounds, a.train)
                ms[k] += dev
                host[k] += enq
        ctx.sync()
        record["kernel"]["n%d" % n] = ms
        for k in launches:
            v = np.asarray(ms[k]) * 1e3
            med = float(np.median(v))
            say("(a) %s, %d x %s: min %.2f us, median %.2f us per launch = %.2f us per frame (%d trains of %d; max %.2f, spread %.1f %% of the median; "
                "host enqueue %.2f us per launch); %.0f GB/s over the %.1f MB it reads"
                % (k, n, a.size, v.min(), med, med / n, len(v), a.train, v.max(), 100.0 * (v.max() - v.min()) / med,
                   float(np.median(host[k])) * 1e3, nbytes / med / 1e3, nbytes / 1e6))
        say("(a) %d x %s: frame_change takes %.3f of the copy's time (medians)"
            % (n, a.size, float(np.median(ms["frame_change"])) / float(np.median(ms["write"]))))
        del src, changed, sad
        m.close()


def loop_part(a, say, record):
    from accel_amd import demo
    from accel_amd.config.config import config, update_config
    from accel_amd.core import tester
    from accel_amd.core.schedule import KeySchedule
    from accel_amd.utils import synth
    H, W = [int(v) for v in a.size.split("x")]
    update_config(os.path.join(ROOT, "tests", "golden", "dff_deeplab_vid_demo.yaml"))
    config.SCALES[0] = (H, W)
    arg, aux = synth.model_params("18", H, W, config)
    frames = synth.make_clip(H, W, a.clip)
    data = demo.build_batches(frames, config, pinned=True, raw=True)
    runner = demo.ClipRunner("18", config, arg, aux, (H, W))
    kinds = {"fixed": lambda: KeySchedule.fixed(5), "adaptive": lambda: KeySchedule.adaptive(share=1.0, max_interval=5)}

    def one_pass(schedule):
        times, keys = [], []
        for idx, arrays in enumerate(data):
            t0 = time.perf_counter()
            _, lab = runner.step(idx, arrays, 5, schedule=schedule)
            if idx + 1 < len(data):
                runner.prefetch(data[idx + 1])
            lab.asnumpy()
            times.append((time.perf_counter() - t0) * 1e3)
            if runner.last_key:
                keys.append(idx)
        return times, keys

    try:
        for make in kinds.values():          # warm both paths
            one_pass(make())
        per = {k: [] for k in kinds}
        for _ in range(a.passes):            # alternate the schedules
            for k, make in kinds.items():
                times, keys = one_pass(make())
                assert keys == [i for i in range(a.clip) if i % 5 == 0], (k, keys)
                per[k].append(times)
        record["loop"] = per
        is_key = np.array([i % 5 == 0 for i in range(a.clip)])
        stats = {}
        for k in kinds:
            t = np.asarray(per[k])           # passes x frames
            mean = t.mean(axis=1)            # per pass
            stats[k] = mean
            say("(b) %s: %.3f ms per frame (median over %d passes of %d frames; min %.3f, max %.3f, spread %.1f %% of the median); key frames "
                "%.3f ms, non-key frames %.3f ms (medians)"
                % (k, float(np.median(mean)), a.passes, a.clip, mean.min(), mean.max(), 100.0 * (mean.max() - mean.min()) / float(np.median(mean)),
                   float(np.median(t[:, is_key])), float(np.median(t[:, ~is_key]))))
        diff = stats["adaptive"] - stats["fixed"]          # pass by pass: neighbours in time
        say("(b) adaptive - fixed: %.1f us per frame (median of the %d pass-by-pass differences; min %.1f, max %.1f)"
            % (float(np.median(diff)) * 1e3, len(diff), diff.min() * 1e3, diff.max() * 1e3))
    finally:
        tester.release_models()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x2048")
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clip", type=int, default=10)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--skip-loop", dest="skip_loop", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import runtime
    lines, record = [], {"size": a.size, "train": a.train, "rounds": a.rounds, "repeats": a.repeats, "kernel": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown (not a git checkout)"
    say("box: %s, torch %s; tree: %s; command: python %s" % (torch.cuda.get_device_name(0), torch.__version__, commit, " ".join(sys.argv)))
    ctx = runtime.Context(0)
    kernel_part(a, ctx, say, record)
    ctx.close()
    if not a.skip_loop:
        loop_part(a, say, record)
    say("json " + json.dumps(record))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
