"""One sha256 per row over every output buffer of every result entry point, on seeded inputs: the A/B of two builds of the library.
    ACCEL_LIB_PATH=<library> python scripts/result_output_digests.py out.txt
Two runs with the same library must give the same file (the calls repeat); a library with a rewritten result half must give the same file as
its parent (profiles/results_refactor.md).  The conf bytes depend on the device's exp, so the file is compared on one machine and not committed.

Rows: ctx level and model level (host and device destinations), n = 2, ncls in {2, 19, 21}, is_prob 0 / 1, a row pitch equal to the row and one
3 bytes (margin: 3 floats) longer, and five geometries (H, W, out_h, out_w, h, w).  Padding bytes are part of the digest (they start as 7s)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N = 2
GEOMETRIES = [(32, 64, 32, 64, 32, 64),        # identity, every vector path
              (32, 64, 31, 52, 31, 52),        # cropped identity
              (32, 64, 31, 54, 29, 50),        # down, odd width
              (32, 64, 31, 54, 67, 131),       # up
              (8, 8, 1, 1, 5, 7)]              # a one-pixel region: both taps clamp to 0
# the overlay's frames: the formats and layouts of the smallest cases of tests/test_overlay_yuv_gpu.py, at an even size of their own
OVERLAYS = [("i420", {}), ("i420", {"pitch": 72, "pitch_c": 40}), ("p010", {}), ("yuy2", {}), ("nv12", {}), ("nv12", {"pitch": 80})]


def scores_of(rng, ncls, H, W, is_prob, identity):
    """finite scores with exact ties at the top and, on the identity rows, pairs more than 2^30 apart in magnitude"""
    s = rng.standard_normal((N, ncls, H, W)).astype(np.float32) * 4
    s[:, 1, ::3, ::5] = s[:, 0, ::3, ::5] = np.float32(9.0)                     # a tie at the top between classes 0 and 1
    s[:, :, 1::7, 2::7] = np.float32(1.5)                                       # a tie of everything
    if identity:
        s[:, 0, 2::5, 1::4] = np.float32(2.0 ** 31)                             # top1 - top2 loses the small operand in fp32 ...
        s[:, ncls - 1, 2::5, 1::4] = np.float32(-3.0 * 2.0 ** -2)               # ... and keeps another rounding in float64
        s[:, 0, 3::5, 3::4] = np.float32(1.0 + 2.0 ** -20)
        s[:, ncls - 1, 3::5, 3::4] = np.float32(2.0 ** -32 + 2.0 ** -50)
    if is_prob:
        e = np.exp(np.minimum(s, 30).astype(np.float64) - 30.0)
        s = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    return s


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b"<none>")
        else:
            a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
            h.update(str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    import torch
    from accel_amd import runtime
    from accel_amd.utils import image
    out_path = sys.argv[1]
    ctx = runtime.Context(0)
    rows = []

    def row(name, *arrays):
        rows.append("%s %s" % (sha(*arrays), name))

    def host(n, h, p, dtype=np.uint8):
        return np.full((n, h, p), 7, dtype)

    def dev(n, h, p, dtype=torch.uint8):
        return torch.full((n, h, p), 7, dtype=dtype, device="cuda")

    palette = np.random.default_rng(5).integers(0, 256, (256, 3), dtype=np.uint8)
    models = {}

    def model(ncls, H, W):
        if (ncls, H, W) not in models:
            m = runtime.Model(ctx)
            m.add_plan("op", "option graph=0 tune=0\npbuf name=logits bytes=%d\npbuf name=labels bytes=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d "
                             "logits_w=%d\nmeta labels_n=%d labels_h=%d labels_w=%d\n"
                       % (N * ncls * H * W * 4, (N * H * W + 255) // 256 * 256, N, ncls, H, W, N, H, W))
            models[(ncls, H, W)] = m
        return models[(ncls, H, W)]

    for gi, (H, W, oh, ow, h, w) in enumerate(GEOMETRIES):
        geo = (oh, ow, h, w)
        rng = np.random.default_rng(100 + gi)
        labels = rng.integers(0, 21, (N, H, W), dtype=np.uint8)
        labels[:, : H // 2, : W // 2] = 3                                       # a run
        labels2 = labels.copy()
        labels2[:, H // 4:, W // 3:] = rng.integers(0, 19, labels2[:, H // 4:, W // 3:].shape, dtype=np.uint8)
        gt = rng.integers(0, 21, (N, h, w), dtype=np.uint8)
        frames = rng.integers(0, 256, (N, h, w, 3), dtype=np.uint8)
        for pad in (0, 3):
            tag = "g%d pad%d" % (gi, pad)
            p1, p3, pm = w + pad, 3 * w + pad, w + pad                          # rows of bytes, of colours, of floats (in elements)
            gtp = host(N, h, p1)
            gtp[:, :, :w] = gt
            fr = host(N, h, p3)
            fr[:, :, :3 * w] = frames.reshape(N, h, 3 * w)
            # ---- ctx level, the label maps ----
            row(tag + " ctx.labels_to_source", ctx.labels_to_source(labels, *geo, out=host(N, h, p1)))
            row(tag + " ctx.labels_hist", ctx.labels_hist(labels, oh, ow, gtp, 19, width=w))
            row(tag + " ctx.labels_colour", ctx.labels_colour(labels, *geo, palette, out=host(N, h, p3)))
            row(tag + " ctx.labels_colour blend", ctx.labels_colour(labels, *geo, palette, frames=fr, alpha=77, rgb=False, width=w, out=host(N, h, p3)))
            kept = host(N, h, p1)
            row(tag + " ctx.labels_summary", *ctx.labels_summary(labels, *geo, 19, kept=kept))
            row(tag + " ctx.labels_summary tracked", *ctx.labels_summary(labels2, *geo, 19, prev=kept, prev_width=w, kept=host(N, h, p1)))
            # ---- model level, the label maps: host and device destinations ----
            m = model(19, H, W)
            m.write("labels", labels)
            row(tag + " model.labels_to_source", m.labels_to_source(N, *geo, out=host(N, h, p1)))
            d = dev(N, h, p1)
            m.labels_to_source_device(d.data_ptr(), N, *geo, p1)
            ctx.sync()
            row(tag + " model.labels_to_source device", d)
            m.hist_add(gtp, oh, ow, 19, width=w)
            g = torch.from_numpy(gtp).cuda()
            m.hist_add_device(g.data_ptr(), N, h, w, p1, oh, ow, 19)
            row(tag + " model.hist_add x2", m.hist_read(19, clear=True))
            row(tag + " model.labels_colour", m.labels_colour(N, *geo, palette, frames=fr, alpha=200, width=w, out=host(N, h, p3)))
            d, f = dev(N, h, p3), torch.from_numpy(fr).cuda()
            m.labels_colour_device(d.data_ptr(), N, *geo, p3, palette, frame_ptr=f.data_ptr(), frame_pitch=p3, alpha=31, rgb=False)
            m.labels_colour_device(d[:1].data_ptr(), 1, *geo, p3, palette)
            ctx.sync()
            row(tag + " model.labels_colour device", d)
            m.labels_forget()
            row(tag + " model.labels_summary", *m.labels_summary(N, *geo, 19, track=True))
            m.write("labels", labels2)
            row(tag + " model.labels_summary tracked", *m.labels_summary(N, *geo, 19, track=True))
            ds, db, dt = (torch.full((N * 19 * k,), 7, dtype=t, device="cuda") for k, t in ((3, torch.int64), (4, torch.int32), (19, torch.int64)))
            m.write("labels", labels)
            cmp_ = m.labels_summary_device(N, *geo, 19, track=True, stats_ptr=ds.data_ptr(), box_ptr=db.data_ptr(), trans_ptr=dt.data_ptr())
            ctx.sync()
            row(tag + " model.labels_summary device compared=%d" % cmp_, ds, db, dt)
            # ---- the scores ----
            for ncls in (2, 19, 21):
                for is_prob in (0, 1):
                    t2 = "%s ncls%d prob%d" % (tag, ncls, is_prob)
                    sc = scores_of(np.random.default_rng(1000 * gi + 10 * ncls + is_prob), ncls, H, W, is_prob, (oh, ow) == (h, w))
                    sc2 = np.ascontiguousarray(sc[:, ::-1]) if ncls > 2 else np.ascontiguousarray(sc[:, :, ::-1])
                    row(t2 + " ctx.scores_confidence", *ctx.scores_confidence(sc, *geo, is_prob=is_prob, conf=host(N, h, p1),
                                                                              margin=host(N, h, pm, np.float32), second=host(N, h, p1)))
                    row(t2 + " ctx.scores_confidence_interp", *ctx.scores_confidence_interp(sc, *geo, is_prob=is_prob, labels=host(N, h, p1), conf=host(N, h, p1),
                                                                                            margin=host(N, h, pm, np.float32), second=host(N, h, p1)))
                    row(t2 + " ctx.scores_confidence margin only", *ctx.scores_confidence(sc, *geo, is_prob=is_prob, conf=False, second=False, hist=False))
                    row(t2 + " ctx.scores_labels", ctx.scores_labels(sc, *geo, out=host(N, h, p1)))
                    m = model(ncls, H, W)
                    m.write("logits", sc)
                    row(t2 + " model.confidence", *m.confidence(N, *geo, is_prob=is_prob, conf=host(N, h, p1), margin=host(N, h, pm, np.float32),
                                                                second=host(N, h, p1)))
                    row(t2 + " model.confidence_interp", *m.confidence_interp(N, *geo, is_prob=is_prob, labels=host(N, h, p1), conf=host(N, h, p1),
                                                                              margin=host(N, h, pm, np.float32), second=host(N, h, p1)))
                    for interp in (0, 1):
                        dl, dc, dsec, dm, dh = dev(N, h, p1), dev(N, h, p1), dev(N, h, p1), dev(N, h, pm, torch.float32), dev(1, N, 256, torch.int64)
                        kw = dict(is_prob=is_prob, conf_ptr=dc.data_ptr(), conf_pitch=p1, margin_ptr=dm.data_ptr(), margin_pitch=4 * pm,
                                  second_ptr=dsec.data_ptr(), second_pitch=p1, hist_ptr=dh.data_ptr())
                        if interp:
                            m.confidence_interp_device(N, *geo, labels_ptr=dl.data_ptr(), labels_pitch=p1, **kw)
                        else:
                            m.confidence_device(N, *geo, **kw)
                        ctx.sync()
                        row(t2 + " model.confidence%s device" % ("_interp" if interp else ""), dl, dc, dm, dsec, dh)
                    row(t2 + " model.scores_labels", m.scores_labels(N, *geo, out=host(N, h, p1)))
                    d = dev(N, h, p1)
                    m.scores_labels_device(d.data_ptr(), N, *geo, p1)
                    ctx.sync()
                    row(t2 + " model.scores_labels device", d)
                    m.scores_hist_add(gtp, oh, ow, 21, width=w)
                    row(t2 + " model.scores_hist_add", m.hist_read(21, clear=True))
                    row(t2 + " model.scores_colour", m.scores_colour(N, *geo, palette, frames=fr, alpha=100, width=w, out=host(N, h, p3)))
                    # a tracked summary over two successive frames, then into device memory
                    m.labels_forget()
                    row(t2 + " model.scores_summary", *m.scores_summary(N, *geo, 21, track=True))
                    m.write("logits", sc2)
                    row(t2 + " model.scores_summary tracked", *m.scores_summary(N, *geo, 21, track=True))
                    ds, db, dt = (torch.full((N * 21 * k,), 7, dtype=t, device="cuda") for k, t in ((3, torch.int64), (4, torch.int32), (21, torch.int64)))
                    m.write("logits", sc)
                    cmp_ = m.scores_summary_device(N, *geo, 21, track=True, stats_ptr=ds.data_ptr(), box_ptr=db.data_ptr(), trans_ptr=dt.data_ptr())
                    ctx.sync()
                    row(t2 + " model.scores_summary device compared=%d" % cmp_, ds, db, dt)
        # ---- the overlay: the frame is as large as the source, so the source size is made even ----
        eh, ew = (h + 1) // 2 * 2, (w + 1) // 2 * 2
        for oi, (fmt, lay) in enumerate(OVERLAYS):
            tag = "g%d overlay%d %s" % (gi, oi, fmt)
            if lay and ew > 64:
                lay = {k: v * 3 for k, v in lay.items()}
            layout = image.overlay_layout(fmt, eh, ew, **lay)
            bits = 10 if fmt == "p010" else 8
            table = image.palette_ycbcr(palette, 0, bits=bits)
            nbytes = N * layout["frame_bytes"]
            buf = np.random.default_rng(7 + oi).integers(0, 256, nbytes, dtype=np.uint8)
            if fmt == "p010":
                buf = (np.random.default_rng(7 + oi).integers(0, 1024, nbytes // 2).astype(np.uint16) << 6).view(np.uint8)
            buf = buf.reshape(N, -1)
            row(tag + " ctx.labels_overlay_yuv", ctx.labels_overlay_yuv(labels, oh, ow, buf, fmt, eh, ew, table, alpha=90, **lay))
            m = model(19, H, W)
            m.write("labels", labels)
            sc = scores_of(np.random.default_rng(50 + gi), 19, H, W, 0, False)
            m.write("logits", sc)
            row(tag + " model.labels_overlay_yuv", m.labels_overlay_yuv(N, oh, ow, buf, fmt, eh, ew, table, alpha=128, **lay))
            row(tag + " model.scores_overlay_yuv", m.scores_overlay_yuv(N, oh, ow, buf, fmt, eh, ew, table, alpha=255, **lay))
            src = torch.from_numpy(buf.copy()).cuda()
            dst = torch.full_like(src, 7)
            st = runtime.yuv_struct(layout, 0)
            m.labels_overlay_yuv_device(src.data_ptr(), dst.data_ptr(), N, oh, ow, st, table, alpha=60)
            ctx.sync()
            row(tag + " model.labels_overlay_yuv device", dst)
            m.scores_overlay_yuv_device(src.data_ptr(), src.data_ptr(), N, oh, ow, st, table, alpha=60)
            ctx.sync()
            row(tag + " model.scores_overlay_yuv device in place", src)

    ctx.sync()
    for m in models.values():
        m.close()
    ctx.close()
    with open(out_path, "w") as f:
        f.write("\n".join(rows) + "\n")
    print("%d rows of %s -> %s" % (len(rows), runtime.LIB_PATH, out_path))


if __name__ == "__main__":
    main()
