"""The calls the result half of the C ABI refuses (csrc/accel_io.cpp from accel_labels_to_source to accel_model_labels_forget), each with the
return code and the message it is refused with.  tests/golden/result_refusals.json holds what the library answered before the result half was
rewritten (scripts/record_result_refusals.py); test_result_refusals_gpu.py replays the cases against the library of the day.

Every case is (id, exported function, arguments) on raw ctypes: the Python wrappers refuse some of these themselves.  A refused call enqueues
nothing, so pointers only have to be non-NULL: host arguments point into one scratch array, "device" arguments into the `logits` buffer of the
model (so a case that were ever accepted by mistake would stay inside memory this file owns)."""
import ctypes
import re

import numpy as np

N, NCLS, H, W = 2, 19, 32, 64       # the model's `labels` (N x H x W) and `logits` (N x NCLS x H x W), as test_results_gpu.py builds them


def _model(runtime, ctx, ncls, labels=True):
    m = runtime.Model(ctx)
    text = "option graph=0 tune=0\n"
    if ncls:
        text += "pbuf name=logits bytes=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d\n" % (N * ncls * H * W * 4, N, ncls, H, W)
    if labels:
        text += "pbuf name=labels bytes=%d\nmeta labels_n=%d labels_h=%d labels_w=%d\n" % ((N * H * W + 255) // 256 * 256, N, H, W)
    if not ncls and not labels:
        text += "pbuf name=other bytes=256\n"
    m.add_plan("op", text)
    return m


class Env(object):
    """what the cases point at: a context, a model with `labels` and `logits` (m), one with neither (m0), one whose scores have 3 classes (m3)"""

    def __init__(self, runtime, ctx):
        from accel_amd.utils import image
        self.lib = runtime.lib()
        self.ctx = ctx.handle
        self.models = [_model(runtime, ctx, NCLS), _model(runtime, ctx, 0, labels=False), _model(runtime, ctx, 3, labels=False)]
        self.m, self.m0, self.m3 = (m.handle for m in self.models)
        self.host = np.zeros(1 << 20, np.uint8)
        self.P = self.host.ctypes.data
        self.D = self.models[0].buffer("logits")[0]
        self.ycc = np.zeros(768, np.uint16)
        self.ycc_300 = self.ycc.copy()
        self.ycc_300[4] = 300
        self.ycc_1024 = self.ycc.copy()
        self.ycc_1024[5] = 1024
        self.lay = runtime.yuv_struct(image.overlay_layout("i420", H, W), 0)
        self.lay10 = runtime.yuv_struct(image.overlay_layout("p010", H, W), 0)
        self.compared = ctypes.c_int(0)
        # the accumulator holds counts of 19 classes from here on: the one call of this file that is accepted
        gt = np.zeros((N, H, W), np.uint8)
        runtime.check(self.lib.accel_model_hist_add(self.m, gt.ctypes.data, N, H, W, W, H, W, 19, 0))

    def close(self):
        out = np.zeros(19 * 19, np.uint64)
        self.lib.accel_model_hist_read(self.m, out.ctypes.data, 19, 1)
        for m in self.models:
            m.close()


def cases(E):
    P, D, ctx, m, m0, m3 = E.P, E.D, E.ctx, E.m, E.m0, E.m3
    ycc, lay, lay10, cmp_ = E.ycc.ctypes.data, ctypes.byref(E.lay), ctypes.byref(E.lay10), ctypes.byref(E.compared)
    G = (N, H, W, H, W, H, W)       # n, H, W, out_h, out_w, h, w of an accepted ctx-level call
    c = []

    def add(name, fn, *args):
        c.append((name, fn, args))

    # ---- the geometry, the pitch, the class count and alpha, through the ctx-level calls ----
    fn = "accel_labels_to_source"
    add("to_source/ctx", fn, None, P, *G, P, W)
    add("to_source/labels", fn, ctx, None, *G, P, W)
    add("to_source/dst", fn, ctx, P, *G, None, W)
    add("to_source/n", fn, ctx, P, 0, H, W, H, W, H, W, P, W)
    add("to_source/H", fn, ctx, P, N, 0, W, H, W, H, W, P, W)
    add("to_source/W", fn, ctx, P, N, H, 32769, H, W, H, W, P, W)
    add("to_source/h", fn, ctx, P, N, H, W, H, W, 0, W, P, W)
    add("to_source/w", fn, ctx, P, N, H, W, H, W, H, 32769, P, 32769)
    add("to_source/out_h", fn, ctx, P, N, H, W, H + 1, W, H, W, P, W)
    add("to_source/out_w", fn, ctx, P, N, H, W, H, 0, H, W, P, W)
    add("to_source/dst_pitch", fn, ctx, P, *G, P, W - 1)
    fn = "accel_labels_hist"
    add("hist/ctx", fn, None, P, N, H, W, H, W, P, H, W, W, 19, P)
    add("hist/labels", fn, ctx, None, N, H, W, H, W, P, H, W, W, 19, P)
    add("hist/gt", fn, ctx, P, N, H, W, H, W, None, H, W, W, 19, P)
    add("hist/hist", fn, ctx, P, N, H, W, H, W, P, H, W, W, 19, None)
    add("hist/out_w", fn, ctx, P, N, H, W, H, W + 1, P, H, W, W, 19, P)
    add("hist/gt_pitch", fn, ctx, P, N, H, W, H, W, P, H, W, W - 1, 19, P)
    add("hist/ncls", fn, ctx, P, N, H, W, H, W, P, H, W, W, 33, P)
    fn = "accel_labels_colour"
    add("colour/ctx", fn, None, P, *G, P, 1, None, 0, 256, P, 3 * W)
    add("colour/labels", fn, ctx, None, *G, P, 1, None, 0, 256, P, 3 * W)
    add("colour/palette", fn, ctx, P, *G, None, 1, None, 0, 256, P, 3 * W)
    add("colour/dst", fn, ctx, P, *G, P, 1, None, 0, 256, None, 3 * W)
    add("colour/h", fn, ctx, P, N, H, W, H, W, 32769, W, P, 1, None, 0, 256, P, 3 * W)
    add("colour/dst_pitch", fn, ctx, P, *G, P, 1, None, 0, 256, P, 3 * W - 1)
    add("colour/frame_pitch", fn, ctx, P, *G, P, 1, P, 3 * W - 1, 128, P, 3 * W)
    add("colour/alpha", fn, ctx, P, *G, P, 1, None, 0, -1, P, 3 * W)

    # ---- the model-level forms of the label maps: each pair, labels form and scores form ----
    for form, fn, mm in (("labels", "accel_model_labels_to_source", m), ("scores", "accel_model_scores_labels", m)):
        t = "model_to_source/%s/" % form
        add(t + "m", fn, None, N, H, W, H, W, P, W, 0)
        add(t + "dst", fn, mm, N, H, W, H, W, None, W, 0)
        add(t + "no_buffer", fn, m0, N, H, W, H, W, P, W, 0)
        add(t + "n", fn, mm, 0, H, W, H, W, P, W, 0)
        add(t + "batch", fn, mm, N + 1, H, W, H, W, P, W, 0)
        add(t + "out_h", fn, mm, N, H + 1, W, H, W, P, W, 0)
        add(t + "w", fn, mm, N, H, W, H, 0, P, W, 0)
        add(t + "dst_pitch", fn, mm, N, H, W, H, W, P, W - 1, 0)
        add(t + "dst_pitch_device", fn, mm, N, H, W, H, W, D, W - 1, 1)
    add("model_to_source/scores/classes", "accel_model_scores_labels", m3, N, H, W, H, W, P, W, 0)
    add("model_to_source/scores/classes+out_h", "accel_model_scores_labels", m3, N, H + 1, W, H, W, P, W, 0)

    for form, fn in (("labels", "accel_model_hist_add"), ("scores", "accel_model_scores_hist_add")):
        t = "model_hist_add/%s/" % form
        add(t + "m", fn, None, P, N, H, W, W, H, W, 19, 0)
        add(t + "gt", fn, m, None, N, H, W, W, H, W, 19, 0)
        add(t + "no_buffer", fn, m0, P, N, H, W, W, H, W, 19, 0)
        add(t + "n", fn, m, P, -1, H, W, W, H, W, 19, 0)
        add(t + "batch", fn, m, P, N + 1, H, W, W, H, W, 19, 0)
        add(t + "batch+h", fn, m, P, N + 1, 0, W, W, H, W, 19, 0)
        add(t + "h", fn, m, P, N, 0, W, W, H, W, 19, 0)
        add(t + "out_w", fn, m, P, N, H, W, W, H, W + 1, 19, 0)
        add(t + "gt_pitch", fn, m, P, N, H, W, W - 1, H, W, 19, 0)
        add(t + "ncls", fn, m, P, N, H, W, W, H, W, 0, 0)
        add(t + "gt_pitch+ncls", fn, m, P, N, H, W, W - 1, H, W, 33, 0)
        add(t + "other_ncls", fn, m, P, N, H, W, W, H, W, 21, 0)
    add("model_hist_add/scores/classes", "accel_model_scores_hist_add", m3, P, N, H, W, W, H, W, 19, 0)
    add("model_hist_add/scores/classes+out_h", "accel_model_scores_hist_add", m3, P, N, H, W, W, H + 1, W, 19, 0)
    fn = "accel_model_hist_read"
    add("model_hist_read/m", fn, None, P, 19, 0)
    add("model_hist_read/out", fn, m, None, 19, 0)
    add("model_hist_read/ncls", fn, m, P, 33, 0)
    add("model_hist_read/other_ncls", fn, m, P, 21, 0)

    for form, fn in (("labels", "accel_model_labels_colour"), ("scores", "accel_model_scores_colour")):
        t = "model_colour/%s/" % form
        add(t + "m", fn, None, N, H, W, H, W, P, 1, None, 0, 256, 0, P, 3 * W, 0)
        add(t + "palette", fn, m, N, H, W, H, W, None, 1, None, 0, 256, 0, P, 3 * W, 0)
        add(t + "dst", fn, m, N, H, W, H, W, P, 1, None, 0, 256, 0, None, 3 * W, 0)
        add(t + "no_buffer", fn, m0, N, H, W, H, W, P, 1, None, 0, 256, 0, P, 3 * W, 0)
        add(t + "batch", fn, m, N + 1, H, W, H, W, P, 1, None, 0, 256, 0, P, 3 * W, 0)
        add(t + "out_h", fn, m, N, 0, W, H, W, P, 1, None, 0, 256, 0, P, 3 * W, 0)
        add(t + "dst_pitch", fn, m, N, H, W, H, W, P, 1, None, 0, 256, 0, P, 3 * W - 1, 0)
        add(t + "frame_pitch", fn, m, N, H, W, H, W, P, 1, P, 3 * W - 1, 128, 0, P, 3 * W, 0)
        add(t + "alpha", fn, m, N, H, W, H, W, P, 1, None, 0, 257, 0, P, 3 * W, 0)
        add(t + "dst_pitch+alpha", fn, m, N, H, W, H, W, P, 1, None, 0, 257, 0, P, 3 * W - 1, 0)
        add(t + "frame_pitch+alpha", fn, m, N, H, W, H, W, P, 1, P, 3 * W - 1, 257, 0, P, 3 * W, 0)
    add("model_colour/scores/classes", "accel_model_scores_colour", m3, N, H, W, H, W, P, 1, None, 0, 256, 0, P, 3 * W, 0)
    add("model_colour/scores/classes+out_h", "accel_model_scores_colour", m3, N, H + 1, W, H, W, P, 1, None, 0, 256, 0, P, 3 * W, 0)

    # ---- confidence: the nearest and the interpolated form (which has labels, labels_pitch in front of conf) ----
    for form, fn, lab in (("nearest", "accel_scores_confidence", ()), ("interp", "accel_scores_confidence_interp", (None, 0))):
        t = "confidence/%s/" % form
        head = (N, NCLS, H, W, H, W, H, W, 0)
        add(t + "ctx", fn, None, P, *head, *lab, P, W, None, 0, None, 0, None)
        add(t + "scores", fn, ctx, None, *head, *lab, P, W, None, 0, None, 0, None)
        add(t + "nothing", fn, ctx, P, *head, *lab, None, 0, None, 0, None, 0, None)
        add(t + "ncls", fn, ctx, P, N, 3, H, W, H, W, H, W, 0, *lab, P, W, None, 0, None, 0, None)
        add(t + "ncls+out_h", fn, ctx, P, N, 3, H, W, H + 1, W, H, W, 0, *lab, P, W, None, 0, None, 0, None)
        add(t + "out_h", fn, ctx, P, N, NCLS, H, W, H + 1, W, H, W, 0, *lab, P, W, None, 0, None, 0, None)
        add(t + "n", fn, ctx, P, 32769, NCLS, H, W, H, W, H, W, 0, *lab, P, W, None, 0, None, 0, None)
        add(t + "conf_pitch", fn, ctx, P, *head, *lab, P, W - 1, None, 0, None, 0, None)
        add(t + "margin_pitch", fn, ctx, P, *head, *lab, None, 0, P, 4 * W - 4, None, 0, None)
        add(t + "margin_pitch_4", fn, ctx, P, *head, *lab, None, 0, P, 4 * W + 2, None, 0, None)
        add(t + "second_pitch", fn, ctx, P, *head, *lab, None, 0, None, 0, P, W - 1, None)
        add(t + "conf_pitch+second_pitch", fn, ctx, P, *head, *lab, P, W - 1, None, 0, P, W - 2, None)
    add("confidence/interp/labels_pitch", "accel_scores_confidence_interp", ctx, P, N, NCLS, H, W, H, W, H, W, 0, P, W - 1, P, W - 2, None, 0, None, 0, None)
    for form, fn, lab in (("nearest", "accel_model_confidence", ()), ("interp", "accel_model_confidence_interp", (None, 0))):
        t = "model_confidence/%s/" % form
        head = (N, H, W, H, W, 0)
        add(t + "m", fn, None, *head, *lab, P, W, None, 0, None, 0, None, 0)
        add(t + "no_buffer", fn, m0, *head, *lab, P, W, None, 0, None, 0, None, 0)
        add(t + "n", fn, m, 0, H, W, H, W, 0, *lab, P, W, None, 0, None, 0, None, 0)
        add(t + "batch", fn, m, N + 1, H, W, H, W, 0, *lab, P, W, None, 0, None, 0, None, 0)
        add(t + "nothing", fn, m, *head, *lab, None, 0, None, 0, None, 0, None, 0)
        add(t + "classes", fn, m3, *head, *lab, P, W, None, 0, None, 0, None, 0)
        add(t + "out_w", fn, m, N, H, W + 1, H, W, 0, *lab, P, W, None, 0, None, 0, None, 0)
        add(t + "conf_pitch", fn, m, *head, *lab, P, W - 1, None, 0, None, 0, None, 0)
        add(t + "margin_pitch_4", fn, m, *head, *lab, None, 0, P, 4 * W + 1, None, 0, None, 0)
        add(t + "margin_device", fn, m, *head, *lab, None, 0, D + 2, 4 * W, None, 0, None, 1)
        add(t + "hist_device", fn, m, *head, *lab, None, 0, None, 0, None, 0, D + 4, 1)
        add(t + "margin_device+hist_device", fn, m, *head, *lab, None, 0, D + 1, 4 * W, None, 0, D + 4, 1)
        add(t + "conf_pitch+margin_device", fn, m, *head, *lab, D, W - 1, D + 1, 4 * W, None, 0, None, 1)
    add("model_confidence/interp/labels_pitch", "accel_model_confidence_interp", m, N, H, W, H, W, 0, P, W - 1, None, 0, None, 0, None, 0, None, 0)

    # ---- labels from interpolated scores, ctx level ----
    fn = "accel_scores_labels"
    add("scores_labels/ctx", fn, None, P, N, NCLS, H, W, H, W, H, W, P, W)
    add("scores_labels/scores", fn, ctx, None, N, NCLS, H, W, H, W, H, W, P, W)
    add("scores_labels/dst", fn, ctx, P, N, NCLS, H, W, H, W, H, W, None, W)
    add("scores_labels/ncls", fn, ctx, P, N, 20, H, W, H, W, H, W, P, W)
    add("scores_labels/ncls+out_h", fn, ctx, P, N, 20, H, W, H + 1, W, H, W, P, W)
    add("scores_labels/out_w", fn, ctx, P, N, NCLS, H, W, H, W + 1, H, W, P, W)
    add("scores_labels/n", fn, ctx, P, 32769, NCLS, H, W, H, W, H, W, P, W)
    add("scores_labels/dst_pitch", fn, ctx, P, N, NCLS, H, W, H, W, H, W, P, W - 1)

    # ---- the overlay in the frame's own format ----
    fn = "accel_labels_overlay_yuv"
    add("overlay/ctx", fn, None, P, N, H, W, H, W, lay, ycc, 128, P, P)
    add("overlay/labels", fn, ctx, None, N, H, W, H, W, lay, ycc, 128, P, P)
    add("overlay/frame", fn, ctx, P, N, H, W, H, W, lay, ycc, 128, None, P)
    add("overlay/dst", fn, ctx, P, N, H, W, H, W, lay, ycc, 128, P, None)
    add("overlay/palette", fn, ctx, P, N, H, W, H, W, lay, None, 128, P, P)
    add("overlay/layout", fn, ctx, P, N, H, W, H, W, None, ycc, 128, P, P)
    add("overlay/alpha", fn, ctx, P, N, H, W, H, W, lay, ycc, 257, P, P)
    add("overlay/palette_value", fn, ctx, P, N, H, W, H, W, lay, E.ycc_300.ctypes.data, 128, P, P)
    add("overlay/palette_value_p010", fn, ctx, P, N, H, W, H, W, lay10, E.ycc_1024.ctypes.data, 128, P, P)
    add("overlay/alpha+palette_value", fn, ctx, P, N, H, W, H, W, lay, E.ycc_300.ctypes.data, 257, P, P)
    add("overlay/out_h", fn, ctx, P, N, H, W, H + 1, W, lay, ycc, 128, P, P)
    add("overlay/n", fn, ctx, P, 0, H, W, H, W, lay, ycc, 128, P, P)
    for form, fn in (("labels", "accel_model_labels_overlay_yuv"), ("scores", "accel_model_scores_overlay_yuv")):
        t = "model_overlay/%s/" % form
        add(t + "m", fn, None, N, H, W, lay, ycc, 128, P, 0, P, 0)
        add(t + "no_buffer", fn, m0, N, H, W, lay, ycc, 128, P, 0, P, 0)
        add(t + "batch", fn, m, N + 1, H, W, lay, ycc, 128, P, 0, P, 0)
        add(t + "batch+frame", fn, m, N + 1, H, W, lay, ycc, 128, None, 0, P, 0)
        add(t + "frame", fn, m, N, H, W, lay, ycc, 128, None, 0, P, 0)
        add(t + "dst", fn, m, N, H, W, lay, ycc, 128, P, 0, None, 0)
        add(t + "palette", fn, m, N, H, W, lay, None, 128, P, 0, P, 0)
        add(t + "layout", fn, m, N, H, W, None, ycc, 128, P, 0, P, 0)
        add(t + "p010_frame_device", fn, m, N, H, W, lay10, ycc, 128, D + 1, 1, D + 65536, 1)
        add(t + "p010_dst_device", fn, m, N, H, W, lay10, ycc, 128, D, 1, D + 65537, 1)
        add(t + "alpha", fn, m, N, H, W, lay, ycc, -1, P, 0, P, 0)
        add(t + "palette_value", fn, m, N, H, W, lay, E.ycc_300.ctypes.data, 128, P, 0, P, 0)
        add(t + "overlap", fn, m, N, H, W, lay, ycc, 128, D, 1, D + 16, 1)
        add(t + "out_h", fn, m, N, H + 1, W, lay, ycc, 128, P, 0, P, 0)
        add(t + "alpha+out_h", fn, m, N, H + 1, W, lay, ycc, 257, P, 0, P, 0)
    add("model_overlay/scores/classes", "accel_model_scores_overlay_yuv", m3, N, H, W, lay, ycc, 128, P, 0, P, 0)
    add("model_overlay/scores/alpha+classes", "accel_model_scores_overlay_yuv", m3, N, H, W, lay, ycc, 257, P, 0, P, 0)
    add("model_overlay/scores/classes+out_h", "accel_model_scores_overlay_yuv", m3, N, H + 1, W, lay, ycc, 128, P, 0, P, 0)

    # ---- frame change ----
    fn = "accel_frame_change"
    tail = (P, P, None, 0)      # changed, sad, mask, mask_pitch
    add("frame_change/ctx", fn, None, P, P, N, H, W, H, W, 8, 64, P, *tail)
    add("frame_change/img", fn, ctx, None, P, N, H, W, H, W, 8, 64, P, *tail)
    add("frame_change/n", fn, ctx, P, P, 32769, H, W, H, W, 8, 64, P, *tail)
    add("frame_change/H", fn, ctx, P, P, N, 0, W, H, W, 8, 64, P, *tail)
    add("frame_change/out_h", fn, ctx, P, P, N, H, W, H + 1, W, 8, 64, P, *tail)
    add("frame_change/out_w", fn, ctx, P, P, N, H, W, H, 0, 8, 64, P, *tail)
    add("frame_change/cell", fn, ctx, P, P, N, H, W, H, W, 12, 64, P, *tail)
    add("frame_change/level_q", fn, ctx, P, P, N, H, W, H, W, 8, 32769, P, *tail)
    add("frame_change/nothing", fn, ctx, P, P, N, H, W, H, W, 8, 64, None, None, None, None, 0)
    add("frame_change/no_key", fn, ctx, P, None, N, H, W, H, W, 8, 64, P, None, P, None, 0)
    add("frame_change/mask_pitch", fn, ctx, P, P, N, H, W, H, W, 8, 64, P, None, None, P, W // 8 - 1)
    fn = "accel_model_frame_change"
    add("model_frame_change/m", fn, None, b"data", N, H, W, 8, 64, P, P, None, 0, 0, cmp_)
    add("model_frame_change/buf", fn, m, None, N, H, W, 8, 64, P, P, None, 0, 0, cmp_)
    add("model_frame_change/compared", fn, m, b"data", N, H, W, 8, 64, P, P, None, 0, 0, None)
    add("model_frame_change/unknown", fn, m, b"data", N, H, W, 8, 64, P, P, None, 0, 0, cmp_)
    add("model_frame_change/not_an_image", fn, m, b"labels", N, H, W, 8, 64, P, P, None, 0, 0, cmp_)
    add("model_frame_keep/m", "accel_model_frame_keep", None)
    add("model_frame_keep/no_signature", "accel_model_frame_keep", m)

    # ---- summary ----
    fn = "accel_labels_summary"
    outs = (P, P, None, None, 0)        # stats, box, trans, kept_out, kept_pitch
    add("summary/ctx", fn, None, P, *G, 19, None, 0, *outs)
    add("summary/labels", fn, ctx, None, *G, 19, None, 0, *outs)
    add("summary/out_h", fn, ctx, P, N, H, W, 0, W, H, W, 19, None, 0, *outs)
    add("summary/n", fn, ctx, P, 32769, H, W, H, W, H, W, 19, None, 0, *outs)
    add("summary/ncls", fn, ctx, P, *G, 33, None, 0, *outs)
    add("summary/n+ncls", fn, ctx, P, 32769, H, W, H, W, H, W, 33, None, 0, *outs)
    add("summary/nothing", fn, ctx, P, *G, 19, None, 0, None, None, None, None, 0)
    add("summary/trans_without_prev", fn, ctx, P, *G, 19, None, 0, P, P, P, None, 0)
    add("summary/prev_pitch", fn, ctx, P, *G, 19, P, W - 1, P, P, P, None, 0)
    add("summary/kept_pitch", fn, ctx, P, *G, 19, None, 0, P, P, None, P, W - 1)
    for form, fn in (("labels", "accel_model_labels_summary"), ("scores", "accel_model_scores_summary")):
        t = "model_summary/%s/" % form
        g = (N, H, W, H, W)
        add(t + "m", fn, None, *g, 19, 0, P, P, None, 0, cmp_)
        add(t + "no_buffer", fn, m0, *g, 19, 0, P, P, None, 0, cmp_)
        add(t + "batch", fn, m, N + 1, H, W, H, W, 19, 0, P, P, None, 0, cmp_)
        add(t + "batch+h", fn, m, N + 1, H, W, 0, W, 19, 0, P, P, None, 0, cmp_)
        add(t + "h", fn, m, N, H, W, 0, W, 19, 0, P, P, None, 0, cmp_)
        add(t + "ncls", fn, m, *g, 33, 0, P, P, None, 0, cmp_)
        add(t + "out_w+ncls", fn, m, N, H, W + 1, H, W, 33, 0, P, P, None, 0, cmp_)
        add(t + "compared", fn, m, *g, 19, 0, P, P, None, 0, None)
        add(t + "ncls+compared", fn, m, *g, 0, 0, P, P, None, 0, None)
        add(t + "nothing", fn, m, *g, 19, 0, None, None, None, 0, cmp_)
        add(t + "trans_without_track", fn, m, *g, 19, 0, P, P, P, 0, cmp_)
        add(t + "stats_device", fn, m, *g, 19, 1, D + 4, D, D + 65536, 1, cmp_)
        add(t + "trans_device", fn, m, *g, 19, 1, D, D, D + 65540, 1, cmp_)
        add(t + "box_device", fn, m, *g, 19, 1, D, D + 2, D + 65536, 1, cmp_)
    add("model_summary/scores/classes", "accel_model_scores_summary", m3, N, H, W, H, W, 19, 0, P, P, None, 0, cmp_)
    add("model_summary/scores/classes+out_h", "accel_model_scores_summary", m3, N, H + 1, W, H, W, 19, 0, P, P, None, 0, cmp_)
    add("model_labels_forget/m", "accel_model_labels_forget", None)
    return c


_ADDRESS = re.compile(r"0x[0-9a-fA-F]+|\(nil\)")


def replay(runtime, ctx):
    """{id: {"rc": return code, "message": accel_last_error() with every printed address replaced by a fixed token}} of every case, in order"""
    env = Env(runtime, ctx)
    try:
        out = {}
        for name, fn, args in cases(env):
            assert name not in out, name
            rc = getattr(env.lib, fn)(*args)
            out[name] = {"rc": int(rc), "message": _ADDRESS.sub("<address>", env.lib.accel_last_error().decode()) if rc else ""}
        return out
    finally:
        env.close()
