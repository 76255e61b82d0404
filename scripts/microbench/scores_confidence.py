"""What the confidence of interpolated scores costs in one pass with their labels (accel_model_confidence_interp, the interpolated form of csrc/confidence.hip)
against the two-kernel route it replaces at the same geometry -- accel_model_scores_labels (csrc/scores_labels.hip) for the labels plus
accel_model_confidence (csrc/confidence.hip, the nearest rule) for conf and hist, each reading the logits once -- on models that own a `logits`
buffer of --frames frames filled with seeded scores.  No network is run: the kernels' time depends on the shapes, not on whose logits they are.

    python scripts/microbench/scores_confidence.py [--frames 4] [--out profiles/scores_confidence.txt]

The three geometries of scripts/microbench/scores_labels.py: 1024 x 2048 at the identity; a 720 x 1280 source of a 1024 x 1820 region of a
1024 x 1824 map; a 2160 x 3840 source of a 1024 x 2048 map.  --frames frames are finished per launch (blockIdx.z), so that with the default 4
the scores (4 x 159 MB) do not fit the 256 MiB Infinity Cache; times are reported per frame.

Device-event time over trains of 20 launches on the library's stream; the variants ALTERNATE train by train (f, l, c, a, f, l, c, a, ...) for
--rounds rounds, so that whatever else the box is doing falls on all of them alike; mean, best and worst train of each are reported:
  (f) fused: labels + conf + hist from one launch
  (l) the yardstick's labels: scores_labels           (c) the yardstick's confidence: nearest conf + hist          yardstick = (l) + (c)
  (a) fused, all five outputs (margin and second too)
  (m) the model-level fused call with host destinations (kernel + the copies of labels, conf, hist + the wait), wall clock, best of 3
The fused labels are compared with those of (l) at every geometry, and at the identity conf and hist with those of (c): they must be equal."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

NCLS = 19
# (H, W, out_h, out_w, h, w)
GEOMETRIES = [(1024, 2048, 1024, 2048, 1024, 2048), (1024, 2048, 1024, 2048, 2160, 3840), (1024, 1824, 1024, 1820, 720, 1280)]


def alternating_ms(ctx, launches, rounds, train=20):
    """{name: [device-event milliseconds per launch of every round]}: one train of each variant per round, in the order given"""
    import torch
    stream = torch.cuda.ExternalStream(ctx.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for launch in launches.values():
        for _ in range(3):
            launch()
    ctx.sync()
    ms = {name: [] for name in launches}
    for _ in range(rounds):
        for name, launch in launches.items():
            e0.record(stream)
            for _ in range(train):
                launch()
            e1.record(stream)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / train)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from accel_amd import runtime
    n = a.frames
    lines, record = [], {"frames": n, "rounds": a.rounds, "geometries": {}}

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
            m.add_plan("op", "option graph=0 tune=0\npbuf name=logits bytes=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d\n"
                             % (n * NCLS * H * W * 4, n, NCLS, H, W))
            one = np.random.default_rng(H * 4096 + W).standard_normal((1, NCLS, H, W)).astype(np.float32)
            m.write("logits", np.ascontiguousarray(np.broadcast_to(one, (n, NCLS, H, W))))         # the same frame n times: time does not care
            del one
            models[(H, W)] = m
        m = models[(H, W)]
        tag = "%dx%d of %dx%d -> %dx%d" % (out_h, out_w, H, W, h, w)
        u8 = lambda: torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        lab_f, conf_f, sec_f, lab_l, conf_c = u8(), u8(), u8(), u8(), u8()
        mar_f = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
        hist_f, hist_c = (torch.empty((n, 256), dtype=torch.int64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        geo = (n, out_h, out_w, h, w)
        launches = {
            "f": lambda: m.confidence_interp_device(*geo, labels_ptr=lab_f.data_ptr(), labels_pitch=w, conf_ptr=conf_f.data_ptr(), conf_pitch=w,
                                                    hist_ptr=hist_f.data_ptr()),
            "l": lambda: m.scores_labels_device(lab_l.data_ptr(), *geo, w),
            "c": lambda: m.confidence_device(*geo, conf_ptr=conf_c.data_ptr(), conf_pitch=w, hist_ptr=hist_c.data_ptr()),
            "a": lambda: m.confidence_interp_device(*geo, labels_ptr=lab_f.data_ptr(), labels_pitch=w, conf_ptr=conf_f.data_ptr(), conf_pitch=w,
                                                    margin_ptr=mar_f.data_ptr(), margin_pitch=4 * w, second_ptr=sec_f.data_ptr(), second_pitch=w,
                                                    hist_ptr=hist_f.data_ptr()),
        }
        ms = alternating_ms(ctx, launches, a.rounds)
        us = {k: (1e3 * float(np.mean(v)) / n, 1e3 * min(v) / n, 1e3 * max(v) / n) for k, v in ms.items()}
        names = {"f": "fused labels + conf + hist", "l": "scores_labels", "c": "nearest conf + hist", "a": "fused, all five outputs"}
        for k in ("f", "l", "c", "a"):
            say("(%s) %s, %s: %.1f us mean / %.1f best / %.1f worst per frame over %d trains" % ((k, tag, names[k]) + us[k] + (a.rounds,)))
        yard = tuple(us["l"][i] + us["c"][i] for i in range(3))
        say("    %s: yardstick (l) + (c) = %.1f us mean / %.1f best / %.1f worst per frame; fused / yardstick = %.2f (means), %.2f (bests)"
            % (tag, yard[0], yard[1], yard[2], us["f"][0] / yard[0], us["f"][1] / yard[1]))
        ctx.sync()
        same = bool(torch.equal(lab_f, lab_l))
        if (h, w) == (out_h, out_w):
            same = same and bool(torch.equal(conf_f, conf_c)) and bool(torch.equal(hist_f, hist_c))
        equal = equal and same
        say("    fused labels against scores_labels%s: %s" % (", conf and hist against the nearest rule's" if (h, w) == (out_h, out_w) else "",
                                                              "equal" if same else "DIFFERENT"))
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = m.confidence_interp(*geo, margin=False, second=False)
            t.append(time.perf_counter() - t0)
        same = bool(np.array_equal(got[0], lab_f.cpu().numpy()) and np.array_equal(got[1], conf_f.cpu().numpy())
                    and np.array_equal(got[4], hist_f.cpu().numpy().astype(np.uint64)))
        equal = equal and same
        say("(m) %s, %d frame(s) of labels + conf + hist to the host: %.2f ms per call (best of 3), %.2f ms per frame; against the device "
            "destinations: %s" % (tag, n, min(t) * 1e3, min(t) * 1e3 / n, "equal" if same else "DIFFERENT"))
        record["geometries"][tag] = {"us_per_frame_mean_best_worst": us, "yardstick_us_per_frame_mean_best_worst": yard,
                                     "model_ms_per_call": min(t) * 1e3}
        del lab_f, conf_f, sec_f, lab_l, conf_c, mar_f, hist_f, hist_c, got
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
