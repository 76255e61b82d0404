"""The overlay in the frame's own format on the GPU (csrc/overlay_yuv.hip behind accel_labels_overlay_yuv and the accel_model_* forms): NV12,
I420 / YV12, P010 and YUY2 frames blended with the label map are what utils.image.overlay_yuv_host gives -- EXACTLY: integer arithmetic, one
rounding per sample, so every comparison is np.array_equal.  The cases are the table of overlay_ref.py: the smallest sizes at which the kernel can
still go wrong (one block, one whole patch, a patch cut by the edge, wide accesses), every layout, every geometry, every label map inside a larger
canvas of label 255.  (Host side, and the wrong kernels the table is held against: test_overlay_yuv_cpu.py.)"""
import ctypes

import numpy as np
import pytest

import overlay_ref as ref
from accel_amd.dataset.cityscape import getpallete
from accel_amd.utils import image, synth

pytestmark = pytest.mark.gpu

CANARY = 0xA5
NAMES = [c["name"] for c in ref.CASES]


def _want(c, alpha=None, labels=None):
    return image.overlay_yuv_host(c["buf"], c["fmt"], c["h"], c["w"], c["at_source"] if labels is None else labels, c["table"],
                                  c["alpha"] if alpha is None else alpha, **c["kw"])


def _labels_model(ctx, n, H, W):
    """a model that owns a `labels` buffer of n x H x W and says so (no op: nothing is ever run)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=labels bytes=%d\nmeta labels_n=%d labels_h=%d labels_w=%d\n"
                     % ((n * H * W + 255) // 256 * 256, n, H, W))
    return m


def _logits_model(ctx, n, ncls, H, W):
    """a model that owns a `logits` buffer of n x ncls x H x W and says so (no op: nothing is ever run)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=logits bytes=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d\n"
                     % ((n * ncls * H * W * 4 + 255) // 256 * 256, n, ncls, H, W))
    return m


# ---- operator level: host in, host out ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_overlay_equals_the_host_specification(ctx, name):
    c = ref.make(ref.BY_NAME[name])
    for alpha in ref.ALPHAS:
        want = _want(c, alpha)
        got = ctx.labels_overlay_yuv(c["labels"], c["out_h"], c["out_w"], c["buf"], c["fmt"], c["h"], c["w"], c["table"], alpha=alpha, **c["kw"])
        assert got.dtype == np.uint8 and got.shape == c["buf"].shape
        assert np.array_equal(got, want), (name, alpha, int(np.count_nonzero(got != want)))
    assert np.array_equal(ctx.labels_overlay_yuv(c["labels"], c["out_h"], c["out_w"], c["buf"], c["fmt"], c["h"], c["w"], c["table"], alpha=0,
                                                 **c["kw"])[~ref.sample_mask(c["lay"], c["n"])], c["buf"][~ref.sample_mask(c["lay"], c["n"])])


# ---- model level: host result, a separate device destination, in place, a refused overlap ---------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_model_overlay_into_host_and_device_memory(ctx, name):
    import torch
    from accel_amd import runtime
    c = ref.make(ref.BY_NAME[name])
    n, lay, bytes_ = c["n"], c["lay"], c["buf"].size
    want, mask = _want(c), ref.sample_mask(c["lay"], c["n"])
    m = _labels_model(ctx, n, c["H"], c["W"])
    try:
        m.write("labels", c["labels"])
        gen = m.generation("labels")
        got = m.labels_overlay_yuv(n, c["out_h"], c["out_w"], c["buf"], c["fmt"], c["h"], c["w"], c["table"], alpha=c["alpha"], **c["kw"])
        assert got.shape == c["buf"].shape and np.array_equal(got, want), ("host", int(np.count_nonzero(got != want)))
        # device memory: at the allocation's own alignment (the wide accesses where the layout allows them) and at the smallest shift the format
        # allows (sample by sample)
        for shift in (0, 2 if lay["format"] == 1 else 1):
            src = torch.zeros(bytes_ + 64, dtype=torch.uint8, device="cuda")
            src[shift:shift + bytes_] = torch.from_numpy(c["buf"].copy()).cuda()
            dst = torch.full((bytes_ + 64,), CANARY, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()          # torch's stream and the library's compute stream are not ordered by themselves
            m.labels_overlay_yuv_device(src.data_ptr() + shift, dst.data_ptr() + shift, n, c["out_h"], c["out_w"], lay, c["table"], alpha=c["alpha"])
            m.ctx.sync()
            host = dst.cpu().numpy()
            body = host[shift:shift + bytes_]
            assert np.array_equal(body[mask], want[mask]), ("device, shift %d" % shift, int(np.count_nonzero(body[mask] != want[mask])))
            assert (body[~mask] == CANARY).all() and (host[:shift] == CANARY).all() and (host[shift + bytes_:] == CANARY).all(), \
                "shift %d: a byte that is no sample was written" % shift
            assert np.array_equal(src.cpu().numpy()[shift:shift + bytes_], c["buf"]), "the source was written"
            # in place
            m.labels_overlay_yuv_device(src.data_ptr() + shift, src.data_ptr() + shift, n, c["out_h"], c["out_w"], lay, c["table"], alpha=c["alpha"])
            m.ctx.sync()
            host = src.cpu().numpy()
            assert np.array_equal(host[shift:shift + bytes_], want), ("in place, shift %d" % shift, int(np.count_nonzero(host[shift:shift + bytes_] != want)))
            assert not host[:shift].any() and not host[shift + bytes_:].any()
            # any other overlap of the two buffers is refused, and nothing is written
            step = 2 if lay["format"] == 1 else 1
            for delta in (step, bytes_ - step if bytes_ > 2 * step else step):
                with pytest.raises(runtime.AccelError, match="overlaps"):
                    m.labels_overlay_yuv_device(src.data_ptr(), src.data_ptr() + delta, n, c["out_h"], c["out_w"], lay, c["table"], alpha=c["alpha"])
            m.ctx.sync()
            assert np.array_equal(src.cpu().numpy(), host)
            del src, dst
        assert m.generation("labels") == gen and np.array_equal(m.read("labels", c["labels"].shape, np.uint8), c["labels"])
    finally:
        ctx.sync()
        m.close()


@pytest.mark.parametrize("name", [n for n in NAMES if ("-6x10-tight-n2-5x7" in n or "-8x32-tight-n1-ident-W+4" in n or "-8x32-tight-n1-5x19" in n)])
def test_model_overlay_of_interpolated_scores(ctx, name):
    """interpolate=True: the labels are those of labels_interpolated_host, made into the library's scratch, then blended at the identity geometry"""
    import torch
    c = ref.make(ref.BY_NAME[name])
    n, ncls, lay = c["n"], 19, c["lay"]
    scores = np.random.default_rng(len(name)).standard_normal((n, ncls, c["H"], c["W"])).astype(np.float32)
    labels = image.labels_interpolated_host(scores, c["out_h"], c["out_w"], c["h"], c["w"])
    m = _logits_model(ctx, n, ncls, c["H"], c["W"])
    try:
        m.write("logits", scores)
        gen = m.generation("logits")
        for alpha in (0, 128, 256):
            want = _want(c, alpha, labels)
            got = m.scores_overlay_yuv(n, c["out_h"], c["out_w"], c["buf"], c["fmt"], c["h"], c["w"], c["table"], alpha=alpha, **c["kw"])
            assert np.array_equal(got, want), (alpha, int(np.count_nonzero(got != want)))
        want = _want(c, 128, labels)
        dev = torch.from_numpy(c["buf"].copy()).cuda()
        torch.cuda.synchronize()
        m.scores_overlay_yuv_device(dev.data_ptr(), dev.data_ptr(), n, c["out_h"], c["out_w"], lay, c["table"], alpha=128)
        m.ctx.sync()
        assert np.array_equal(dev.cpu().numpy(), want)
        assert m.generation("logits") == gen and np.array_equal(m.read("logits", scores.shape), scores)
        del dev
    finally:
        ctx.sync()
        m.close()


def test_argument_errors_return_err_arg(ctx):
    """what the kernel could not honour is refused on the host, with a message that names the argument; nothing is launched"""
    from accel_amd import runtime
    lib = runtime.lib()
    n, H, W, h, w = 2, 10, 16, 6, 10
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 19, (n, H, W), dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lays = {fmt: image.overlay_layout(fmt, h, w) for fmt in ref.FORMATS}
    tables = {fmt: np.ascontiguousarray(image.palette_ycbcr(ref.palette(), 0, bits=10 if fmt == "p010" else 8).reshape(-1)) for fmt in ref.FORMATS}
    m = _labels_model(ctx, n, H, W)
    s = _logits_model(ctx, n, 19, H, W)
    try:
        m.write("labels", labels)
        s.write("logits", rng.standard_normal((n, 19, H, W)).astype(np.float32))
        state = m.generation("labels"), s.generation("logits")
        for fmt in ref.FORMATS:
            lay = lays[fmt]
            frame = rng.integers(0, 256, n * lay["frame_bytes"], dtype=np.uint8)
            dst = np.zeros_like(frame)
            good = dict(labels=vp(labels), n=n, H=H, W=W, out_h=8, out_w=13, lay=dict(lay), table=tables[fmt], alpha=128, frame=vp(frame), dst=vp(dst))

            def struct(a):
                if a["lay"] is None:
                    return None
                y = a["lay"]
                return ctypes.byref(runtime.YUVLayout(y["format"], y.get("colour", 0), y["h"], y["w"], y["pitch"], y["pitch_c"], y["u_offset"],
                                                      y["v_offset"], y["frame_bytes"]))

            def table(a):
                return None if a["table"] is None else vp(a["table"])

            calls = {
                "op": lambda a: lib.accel_labels_overlay_yuv(ctx.handle, a["labels"], a["n"], a["H"], a["W"], a["out_h"], a["out_w"], struct(a), table(a),
                                                             a["alpha"], a["frame"], a["dst"]),
                "labels": lambda a: lib.accel_model_labels_overlay_yuv(m.handle, a["n"], a["out_h"], a["out_w"], struct(a), table(a), a["alpha"],
                                                                       a["frame"], 0, a["dst"], 0),
                "scores": lambda a: lib.accel_model_scores_overlay_yuv(s.handle, a["n"], a["out_h"], a["out_w"], struct(a), table(a), a["alpha"],
                                                                       a["frame"], 0, a["dst"], 0),
            }
            every = tuple(calls)
            big = tables[fmt].copy()
            big[3 * 200 + 2] = 1024 if fmt == "p010" else 256
            cases = [(dict(n=0), "n =", every), (dict(out_h=H + 1), "out_h", every), (dict(out_w=0), "out_w", every), (dict(H=0), "H x W", ("op",)),
                     (dict(alpha=-1), "alpha", every), (dict(alpha=257), "alpha", every), (dict(frame=None), "frame is NULL", every),
                     (dict(dst=None), "dst is NULL", every), (dict(table=None), "palette_ycc is NULL", every), (dict(lay=None), "layout is NULL", every),
                     (dict(labels=None), "labels", ("op",)), (dict(table=big), "palette_ycc[602]", every),
                     (dict(lay=dict(lay, format=4)), "format", every), (dict(lay=dict(lay, w=w + 1)), "w =", every),
                     (dict(lay=dict(lay, pitch=lay["pitch"] - 1)), "pitch", every), (dict(lay=dict(lay, frame_bytes=lay["frame_bytes"] - 1)), "frame_bytes", every),
                     (dict(n=n + 1), "n =", ("labels", "scores"))]
            if fmt != "yuy2":
                cases += [(dict(lay=dict(lay, h=h + 1)), "h =", every), (dict(lay=dict(lay, u_offset=lay["u_offset"] - 2)), "u_offset", every)]
            if fmt != "i420":
                cases += [(dict(lay=dict(lay, pitch_c=8)), "pitch_c", every), (dict(lay=dict(lay, v_offset=lay["frame_bytes"])), "v_offset", every)]
            for change, word, names in cases:
                for name in names:
                    rc = calls[name](dict(good, **change))
                    msg = lib.accel_last_error().decode()
                    assert rc == -1, (fmt, name, change, rc, msg)       # ACCEL_ERR_ARG
                    assert word in msg, (fmt, name, change, msg)
            assert not dst.any()
            # the colour field is not looked at, and every call is accepted as it stands
            for name in every:
                assert calls[name](dict(good, lay=dict(lay, colour=7) if name == "op" else dict(lay))) == 0, (fmt, name, lib.accel_last_error().decode())
            # the entry points from before keep refusing format 3
            if fmt == "nv12":
                bgr = np.zeros((n, h, w, 3), np.uint8)
                assert lib.accel_yuv_to_bgr(ctx.handle, vp(frame), n, ctypes.byref(runtime.yuv_struct(lay, 0)), vp(bgr), 3 * w, 0) == -1
                assert "format" in lib.accel_last_error().decode()
        # P010 words are 2-byte aligned in device memory, source and destination
        import torch
        lay = lays["p010"]
        dev = torch.zeros(2 * n * lay["frame_bytes"] + 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for src_ptr, dst_ptr, word in ((dev.data_ptr() + 1, dev.data_ptr(), "frame ="), (dev.data_ptr(), dev.data_ptr() + n * lay["frame_bytes"] + 1, "dst =")):
            with pytest.raises(runtime.AccelError, match=word):
                m.labels_overlay_yuv_device(src_ptr, dst_ptr, n, 8, 13, lay, tables["p010"])
        ctx.sync()
        assert not dev.cpu().numpy().any()
        bare = runtime.Model(ctx)
        with pytest.raises(runtime.AccelError, match="labels"):
            bare.labels_overlay_yuv(1, 6, 10, np.zeros(lays["nv12"]["frame_bytes"], np.uint8), "nv12", 6, 10, tables["nv12"])
        with pytest.raises(runtime.AccelError, match="logits"):
            bare.scores_overlay_yuv(1, 6, 10, np.zeros(lays["nv12"]["frame_bytes"], np.uint8), "nv12", 6, 10, tables["nv12"])
        bare.close()
        assert (m.generation("labels"), s.generation("logits")) == state
        assert np.array_equal(m.read("labels", (n, H, W), np.uint8), labels)
    finally:
        ctx.sync()
        m.close()
        s.close()


# ---- the whole graph ----------------------------------------------------------------------------------------------------------------------------------
def test_results_overlay_on_accel18(demo_cfg):
    """Accel-18 at 128 x 256 fed with 90 x 180 frames in each of the four formats: results.overlay of the label handle and, interpolated, of the
    logits handle are the specification applied to the frame's own bytes; the calls change nothing in the model"""
    from accel_amd import demo, runtime
    from accel_amd.core import results, tester
    H, W, rows, cols = 128, 256, 90, 180
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = 16
    out_h, out_w = image.resize_geometry(rows, cols, H, W, 16)[1:3]
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    frames = synth.make_clip(rows, cols, 1)
    pal = getpallete(256)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        kept = None
        for fmt, kw in (("nv12", dict(nv12="bt601")), ("i420", dict(yuv="i420")), ("p010", dict(yuv="p010", yuv_colour="bt709-full")), ("yuy2", dict(yuv="yuy2"))):
            batch = demo.build_batches(frames, demo_cfg, **kw)[0]
            like = batch[0]
            lg, lab = r.step(0, batch, 3)
            m = lab.device_ref[0]
            gen = m.generation("labels"), m.generation("logits")
            labels0, logits0 = m.read("labels", (1, H, W), np.uint8), m.read("logits", (1, 19, H, W))
            buf = like.nv12 if fmt == "nv12" else like.yuv
            table = image.palette_ycbcr(pal, like.layout["colour"], bits=10 if fmt == "p010" else 8)
            for interpolate in (False, True):
                at = (image.labels_interpolated_host(logits0, out_h, out_w, rows, cols) if interpolate
                      else image.labels_to_source_host(labels0, out_h, out_w, rows, cols))
                want = image.overlay_yuv_host(buf, fmt, rows, cols, at, table, 96)
                got = results.overlay(lg if interpolate else lab, like, pal, alpha=96, interpolate=interpolate)
                assert got.dtype == buf.dtype and got.shape == buf.shape
                assert np.array_equal(got, want), (fmt, interpolate, int(np.count_nonzero(got != want)))
                assert not np.array_equal(got, buf)
            assert like._frames is None, "the overlay does not convert the frames to BGR on the host"
            assert (m.generation("labels"), m.generation("logits")) == gen
            assert np.array_equal(m.read("labels", (1, H, W), np.uint8), labels0) and np.array_equal(m.read("logits", (1, 19, H, W)), logits0)
            with pytest.raises(runtime.AccelError, match="logits"):
                results.overlay(lab, like, pal, interpolate=True)
            if kept is not None:       # a handle kept across a forward names a buffer that has been rewritten: never read
                with pytest.raises(runtime.AccelError, match="stale"):
                    results.overlay(kept, like, pal)
            kept = lab
    finally:
        tester.release_models()


@pytest.mark.parametrize("flags", [["--nv12"], ["--yuv", "i420"], ["--yuv", "p010", "--interpolate"], ["--yuv", "yuy2"]])
def test_demo_writes_the_overlay(demo_cfg, capsys, tmp_path, flags):
    from PIL import Image
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "2", "--num_ex", "1", "--synthetic", "90x180", "--scales", "128x256", "--finish-on-gpu",
                   "--overlay-yuv", "--out", str(tmp_path)] + flags)
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    assert out.rstrip().endswith("done") and out.count("testing synthetic_") == 2, out[-1500:]
    pngs = sorted(tmp_path.glob("overlay_*.png"))
    assert len(pngs) == 2 and len(sorted(tmp_path.glob("seg_*.png"))) == 2
    im = Image.open(str(pngs[0]))
    assert im.size == (180, 90) and im.mode == "RGB"
    with pytest.raises(ValueError, match="--overlay-yuv"):
        demo.main(["--version", "18", "--synthetic", "90x180", "--finish-on-gpu", "--overlay-yuv"])
