"""Finished frames on the GPU (csrc/results_u8.hip behind accel_labels_to_source / _hist / _colour and the accel_model_* forms): labels at the
source frame's size, the confusion matrix and the colour image are what the host restatements give -- utils/image.py labels_to_source_host and
colour_host, demo.fast_hist -- EXACTLY.  Everything is integer arithmetic on bytes, so every comparison is np.array_equal: no tolerance.
(Host side: test_results_cpu.py.)"""
import ctypes

import numpy as np
import pytest

from accel_amd.utils import image, synth

from test_frames_u8_gpu import SMALL

pytestmark = pytest.mark.gpu

STRIDE = 16
ALPHAS = (0, 1, 128, 255, 256)
# (rows, cols, target, max): the ten small geometries, the BASELINE frame (identity) and a 720p camera against its bound size (a 1024 x 1820
# region padded to 1024 x 1824)
GEOMETRIES = SMALL + [(1024, 2048, 1024, 2048), (720, 1280, 1024, 2048)]
PALETTE = np.random.default_rng(2026).integers(0, 256, (256, 3), dtype=np.uint8)


def _geo(rows, cols, target, max_size, stride=STRIDE):
    """(out_h, out_w, H, W): the valid region and the padded size of the label map a rows x cols frame gives"""
    return image.resize_geometry(rows, cols, target, max_size, stride)[1:]


def _fast_hist(pred, gt, ncls):
    """demo.fast_hist over the pixels that count: it assumes pred < ncls (argmax of ncls channels); an id >= ncls on either side is ignored"""
    from accel_amd import demo
    pred, gt = pred.reshape(-1), gt.reshape(-1)
    k = pred < ncls
    return demo.fast_hist(pred[k], gt[k], ncls)


def _pitches(row):
    """a tight row, a pitch that is a multiple of 16, one that is a multiple of 4 only, an odd one"""
    p16 = (row + 15) // 16 * 16 + 16
    return [row, p16, p16 + 4, p16 + (1 if p16 % 2 == 0 else 2) + 4]


def _pitched(a, pitch, seed):
    """n x h x row bytes inside n x h x pitch bytes whose other bytes are non-zero noise"""
    n, h, row = a.shape
    out = np.random.default_rng(seed).integers(1, 256, (n, h, pitch), dtype=np.uint8)
    out[:, :, :row] = a
    return out


def _check_rows(out, before, want, what):
    """the rows hold `want`, the bytes between the rows are untouched"""
    row = want.shape[2]
    assert np.array_equal(out[:, :, :row], want), "%s: %d bytes differ" % (what, int(np.count_nonzero(out[:, :, :row] != want)))
    assert np.array_equal(out[:, :, row:], before[:, :, row:]), "%s: bytes between the rows were written" % (what,)


# ---- operator level: labels at the source size ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rows,cols,target,max_size", GEOMETRIES)
def test_labels_to_source_equals_the_host_restatement(ctx, rows, cols, target, max_size, n):
    out_h, out_w, H, W = _geo(rows, cols, target, max_size)
    labels = np.random.default_rng(rows * 4096 + cols + n).integers(0, 256, (n, H, W), dtype=np.uint8)
    want = image.labels_to_source_host(labels, out_h, out_w, rows, cols)
    got = ctx.labels_to_source(labels, out_h, out_w, rows, cols)
    assert got.dtype == np.uint8 and got.shape == (n, rows, cols)
    assert np.array_equal(got, want), (rows, cols, int(np.count_nonzero(got != want)))
    for pitch in _pitches(cols)[1:]:
        out = _pitched(np.zeros((n, rows, cols), np.uint8), pitch, pitch)
        before = out.copy()
        assert ctx.labels_to_source(labels, out_h, out_w, rows, cols, out=out) is out
        _check_rows(out, before, want, "pitch %d" % pitch)


@pytest.mark.parametrize("rows,cols", [(48, 90), (31, 50), (17, 33), (16, 20)])
def test_labels_to_source_crops_widths_not_divisible_by_four(ctx, rows, cols):
    """the identity case with a valid region narrower than the map: a crop, through the scalar and the dword path"""
    H, W = (rows + 15) // 16 * 16, (cols + 15) // 16 * 16
    labels = np.random.default_rng(cols).integers(0, 256, (2, H, W), dtype=np.uint8)
    assert np.array_equal(ctx.labels_to_source(labels, rows, cols, rows, cols), labels[:, :rows, :cols])


# ---- operator level: confusion matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rows,cols,target,max_size", GEOMETRIES)
def test_hist_of_uniform_random_pairs(ctx, rows, cols, target, max_size, n):
    out_h, out_w, H, W = _geo(rows, cols, target, max_size)
    rng = np.random.default_rng(rows * 8192 + cols + n)
    labels = rng.integers(0, 19, (n, H, W), dtype=np.uint8)
    gt = rng.integers(0, 19, (n, rows, cols), dtype=np.uint8)
    want = _fast_hist(image.labels_to_source_host(labels, out_h, out_w, rows, cols), gt, 19)
    assert want.sum() == n * rows * cols
    for pitch in _pitches(cols):
        g = gt if pitch == cols else _pitched(gt, pitch, pitch)
        got = ctx.labels_hist(labels, out_h, out_w, g, 19, width=cols)
        assert got.dtype == np.uint64 and got.shape == (19, 19)
        assert np.array_equal(got.astype(np.int64), want), ("pitch %d" % pitch, int(np.abs(got.astype(np.int64) - want).sum()))


def test_hist_of_one_pair_on_every_pixel(ctx):
    """the contention case: 8 x 1024 x 2048 pixels, all of them (gt 7, pred 5) -- one bin takes 2^24"""
    labels = np.full((8, 1024, 2048), 5, np.uint8)
    gt = np.full((8, 1024, 2048), 7, np.uint8)
    got = ctx.labels_hist(labels, 1024, 2048, gt, 19)
    want = np.zeros((19, 19), np.int64)
    want[7, 5] = 1 << 24
    assert np.array_equal(got.astype(np.int64), want), got[7, 5]
    # and through the resampling path: a 720p source against a 1024 x 1824 region of the same maps
    got = ctx.labels_hist(labels[:2], 1024, 1824, gt[:2, :720, :1280], 19)
    want[7, 5] = 2 * 720 * 1280
    assert np.array_equal(got.astype(np.int64), want), got[7, 5]


def _runs(rng, count, ncls):
    """`count` values in runs of 1 .. 4096 equal ones"""
    lengths = rng.integers(1, 4097, count // 1024 + 8)
    values = rng.integers(0, ncls, lengths.size, dtype=np.uint8)
    return np.repeat(values, lengths)[:count]


@pytest.mark.parametrize("rows,cols,target,max_size", [(512, 1024, 512, 1024), (360, 640, 512, 1024)])
def test_hist_of_runs_of_equal_pixels(ctx, rows, cols, target, max_size):
    out_h, out_w, H, W = _geo(rows, cols, target, max_size)
    rng = np.random.default_rng(rows)
    labels = _runs(rng, 2 * H * W, 19).reshape(2, H, W)
    gt = _runs(rng, 2 * rows * cols, 19).reshape(2, rows, cols)
    want = _fast_hist(image.labels_to_source_host(labels, out_h, out_w, rows, cols), gt, 19)
    assert np.array_equal(ctx.labels_hist(labels, out_h, out_w, gt, 19).astype(np.int64), want)


@pytest.mark.parametrize("ncls", [2, 19, 21, 32])
@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (45, 83, 48, 96), (60, 120, 48, 96)])
def test_hist_ignores_ids_outside_the_classes(ctx, ncls, rows, cols, target, max_size):
    """gt holds 255 and every id in 19 .. 254 (and the labels ids up to 40): a pixel counts iff gt < ncls and pred < ncls"""
    out_h, out_w, H, W = _geo(rows, cols, target, max_size)
    rng = np.random.default_rng(ncls * 100 + rows)
    labels = rng.integers(0, 41, (3, H, W), dtype=np.uint8)
    gt = rng.integers(0, 256, (3, rows, cols), dtype=np.uint8)
    gt[:, ::3, ::2] = rng.integers(0, ncls, gt[:, ::3, ::2].shape, dtype=np.uint8)
    gt[1, 5:20, :] = 255
    gt.reshape(-1)[:236] = np.arange(19, 255)
    src = image.labels_to_source_host(labels, out_h, out_w, rows, cols)
    want = _fast_hist(src, gt, ncls)
    assert 0 < want.sum() == int(np.count_nonzero((gt < ncls) & (src < ncls))) < gt.size
    got = ctx.labels_hist(labels, out_h, out_w, gt, ncls)
    assert got.shape == (ncls, ncls) and np.array_equal(got.astype(np.int64), want)
    # the caller's matrix is added to
    start = rng.integers(0, 1 << 40, (ncls, ncls)).astype(np.uint64)
    got = ctx.labels_hist(labels, out_h, out_w, gt, ncls, hist=start)
    assert np.array_equal(got.astype(np.int64), want + start.astype(np.int64))


# ---- operator level: colour image ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rows,cols,target,max_size", GEOMETRIES)
def test_colour_equals_the_host_restatement(ctx, rows, cols, target, max_size, n):
    out_h, out_w, H, W = _geo(rows, cols, target, max_size)
    rng = np.random.default_rng(rows * 2048 + cols + n)
    labels = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    frames = rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)
    src = image.labels_to_source_host(labels, out_h, out_w, rows, cols)
    for rgb in (True, False):
        got = ctx.labels_colour(labels, out_h, out_w, rows, cols, PALETTE, rgb=rgb)
        assert got.dtype == np.uint8 and got.shape == (n, rows, cols, 3)
        assert np.array_equal(got, image.colour_host(src, PALETTE, rgb=rgb)), ("no frame", rgb)
        for alpha in ALPHAS:
            got = ctx.labels_colour(labels, out_h, out_w, rows, cols, PALETTE, frames=frames, alpha=alpha, rgb=rgb)
            want = image.colour_host(src, PALETTE, frames=frames, alpha=alpha, rgb=rgb)
            assert np.array_equal(got, want), ("alpha %d" % alpha, rgb, int(np.count_nonzero(got != want)))


@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (45, 83, 48, 96), (60, 120, 48, 96)])
def test_colour_with_pitched_rows(ctx, rows, cols, target, max_size):
    out_h, out_w, H, W = _geo(rows, cols, target, max_size)
    rng = np.random.default_rng(cols)
    labels = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    frames = rng.integers(0, 256, (2, rows, cols, 3), dtype=np.uint8)
    src = image.labels_to_source_host(labels, out_h, out_w, rows, cols)
    for pitch in _pitches(3 * cols)[1:]:
        for fpitch in (3 * cols, pitch):
            f = _pitched(frames.reshape(2, rows, 3 * cols), fpitch, fpitch)
            out = _pitched(np.zeros((2, rows, 3 * cols), np.uint8), pitch, pitch + 1)
            before = out.copy()
            ctx.labels_colour(labels, out_h, out_w, rows, cols, PALETTE, frames=f, width=cols, alpha=128, rgb=False, out=out)
            _check_rows(out, before, image.colour_host(src, PALETTE, frames=frames, alpha=128, rgb=False).reshape(2, rows, 3 * cols),
                        "dst pitch %d, frame pitch %d" % (pitch, fpitch))


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------
def _labels_model(ctx, n, H, W):
    """a model that owns a `labels` buffer of n x H x W and says so (no op: nothing is ever run)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    m.add_plan("op", "option graph=0 tune=0\npbuf name=labels bytes=%d\nmeta labels_n=%d labels_h=%d labels_w=%d\n"
                     % ((n * H * W + 255) // 256 * 256, n, H, W))
    return m


def test_accumulator_counts_past_32_bits_and_is_per_model(ctx):
    """the single-pair map, 2^24 pixels per call, ground truth resident in HBM: 257 calls leave 257 * 2^24 > 2^32 in one bin"""
    import torch
    n, H, W = 8, 1024, 2048
    m = _labels_model(ctx, n, H, W)
    other = _labels_model(ctx, 1, 32, 64)
    try:
        m.write("labels", np.full((n, H, W), 5, np.uint8))
        other.write("labels", np.full((1, 32, 64), 2, np.uint8))
        assert not m.hist_read(19).any()
        gt = torch.full((n, H, W), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                     # torch's stream and the library's compute stream are not ordered by themselves
        for _ in range(257):
            m.hist_add_device(gt.data_ptr(), n, H, W, W, H, W, 19)
        other.hist_add(np.full((1, 32, 64), 3, np.uint8), 32, 64, 19)
        want = np.zeros((19, 19), np.int64)
        want[7, 5] = 257 * (1 << 24)
        assert want[7, 5] > 1 << 32
        got = m.hist_read(19)
        assert got.dtype == np.uint64 and np.array_equal(got.astype(np.int64), want), got[7, 5]
        theirs = np.zeros((19, 19), np.int64)
        theirs[3, 2] = 32 * 64
        assert np.array_equal(other.hist_read(19).astype(np.int64), theirs)
        assert np.array_equal(m.hist_read(19, clear=True).astype(np.int64), want)
        assert not m.hist_read(19).any()
        assert np.array_equal(other.hist_read(19).astype(np.int64), theirs)      # the other model's accumulator was not cleared
        m.hist_add_device(gt.data_ptr(), n, H, W, W, H, W, 21)                  # after a clear another class count may start
        assert int(m.hist_read(21)[7, 5]) == 1 << 24
        ctx.sync()
        del gt
    finally:
        ctx.sync()
        m.close()
        other.close()


def _steps(runner, batches, interval, count):
    outs = []
    for i in range(count):
        lg, lab = runner.step(i, batches[i], interval)
        outs.append((lg.asnumpy().copy(), lab.asnumpy().copy()))
    return outs


@pytest.mark.parametrize("rows,cols", [(90, 180),        # resampled: the whole 128 x 256 map is valid, every source pixel is a gather
                                       (128, 256),       # the frame itself
                                       (120, 250)])      # a 123 x 256 region padded to 128 x 256
def test_finishing_calls_on_accel18(demo_cfg, rows, cols):
    """Accel-18 at 128 x 256 on the synthetic clip, raw frames: a key and a non-key frame are finished on the GPU; the finishing calls
    change nothing -- not the generation, not the buffers, not what the captured graphs compute next"""
    from accel_amd import demo, runtime
    from accel_amd.core import results, tester
    H, W = 128, 256
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = STRIDE
    out_h, out_w = _geo(rows, cols, H, W)[:2]
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    frames = synth.make_clip(rows, cols, 3)
    rng = np.random.default_rng(rows)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        raw = demo.build_batches(frames, demo_cfg, raw=True)
        assert raw[0][0].shape == (1, 3, H, W) and (raw[0][0].geometry["out_h"], raw[0][0].geometry["out_w"]) == (out_h, out_w)
        ref = _steps(r, raw, 3, 3)                       # frames 0 (key), 1, 2 (non-key) without any finishing call
        ev = results.Evaluator(19)
        total = np.zeros((19, 19), np.int64)
        kept = None
        for i in (0, 1):
            lg, lab = r.step(i, raw[i], 3)
            m = lab.device_ref[0]
            gen = m.generation("labels"), m.generation("logits")
            labels0, logits0 = m.read("labels", (1, H, W), np.uint8), m.read("logits", (1, 19, H, W))
            assert np.array_equal(labels0, ref[i][1]) and np.array_equal(logits0, ref[i][0])
            gt = rng.integers(0, 19, (rows, cols), dtype=np.uint8)
            gt[rng.integers(0, 4, gt.shape) == 0] = 255
            want_src = image.labels_to_source_host(labels0, out_h, out_w, rows, cols)
            # the three finishing calls, each through the handle
            ev.add(lab, gt, like=raw[i][0])
            src = results.labels_at_source(lab, raw[i][0])
            col = results.colour(lab, raw[i][0], PALETTE, frames=True, alpha=128)
            assert src.dtype == np.uint8 and np.array_equal(src, want_src)
            total += _fast_hist(want_src, gt, 19)
            assert ev.hist().dtype == np.int64 and np.array_equal(ev.hist(), total)
            assert np.array_equal(col, image.colour_host(want_src, PALETTE, frames=frames[i][None], alpha=128))
            assert np.array_equal(results.colour(lab, dict(raw[i][0].geometry, h=rows, w=cols), PALETTE, rgb=False),
                                  image.colour_host(want_src, PALETTE, rgb=False))
            # nothing was written: generations, labels and logits are what they were
            assert (m.generation("labels"), m.generation("logits")) == gen
            assert np.array_equal(m.read("labels", (1, H, W), np.uint8), labels0)
            assert np.array_equal(m.read("logits", (1, 19, H, W)), logits0)
            assert np.array_equal(lab.asnumpy(), labels0)
            kept = lab
        assert np.allclose(ev.per_class_iu(), demo.per_class_iu(total), equal_nan=True)
        # the captured graphs are undisturbed: the next step gives what the run without finishing calls gave
        lg, lab = r.step(2, raw[2], 3)
        assert np.array_equal(lg.asnumpy(), ref[2][0]) and np.array_equal(lab.asnumpy(), ref[2][1])
        # a label handle kept across that step names a buffer that has been rewritten: never read
        for call in (lambda: results.labels_at_source(kept, raw[1][0]), lambda: ev.add(kept, np.zeros((rows, cols), np.uint8), like=raw[1][0]),
                     lambda: results.colour(kept, raw[1][0], PALETTE)):
            with pytest.raises(runtime.AccelError, match="stale"):
                call()
        assert np.array_equal(ev.hist(), total)
    finally:
        tester.release_models()


def test_argument_errors_return_err_arg(ctx):
    """every geometry the kernels could not honour is refused on the host, with a message that names the argument; nothing is launched and the
    model is what it was"""
    from accel_amd import runtime
    lib = runtime.lib()
    n, H, W, rows, cols = 2, 32, 64, 29, 50
    out_h, out_w = 31, 54
    rng = np.random.default_rng(1)
    labels = rng.integers(0, 19, (n, H, W), dtype=np.uint8)
    gt = rng.integers(0, 19, (n, rows, cols), dtype=np.uint8)
    frame = rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)
    pal = np.ascontiguousarray(PALETTE.reshape(-1))
    dst = np.zeros((n, rows, cols), np.uint8)
    dst3 = np.zeros((n, rows, cols, 3), np.uint8)
    hist = np.zeros((19, 19), np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(labels=vp(labels), n=n, H=H, W=W, out_h=out_h, out_w=out_w, h=rows, w=cols, dst=vp(dst), dst_pitch=cols, gt=vp(gt), gt_pitch=cols,
                ncls=19, hist=vp(hist), pal=vp(pal), frame=vp(frame), frame_pitch=3 * cols, alpha=128, dst3=vp(dst3), dst3_pitch=3 * cols)
    m = _labels_model(ctx, n, H, W)
    try:
        m.write("labels", labels)
        m.hist_add(gt, out_h, out_w, 19)
        state = m.generation("labels"), m.hist_read(19)

        calls = {
            "op source": lambda a: lib.accel_labels_to_source(ctx.handle, a["labels"], a["n"], a["H"], a["W"], a["out_h"], a["out_w"], a["h"], a["w"],
                                                              a["dst"], a["dst_pitch"]),
            "op hist": lambda a: lib.accel_labels_hist(ctx.handle, a["labels"], a["n"], a["H"], a["W"], a["out_h"], a["out_w"], a["gt"], a["h"], a["w"],
                                                       a["gt_pitch"], a["ncls"], a["hist"]),
            "op colour": lambda a: lib.accel_labels_colour(ctx.handle, a["labels"], a["n"], a["H"], a["W"], a["out_h"], a["out_w"], a["h"], a["w"],
                                                           a["pal"], 1, a["frame"], a["frame_pitch"], a["alpha"], a["dst3"], a["dst3_pitch"]),
            "model source": lambda a: lib.accel_model_labels_to_source(m.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], a["dst"], a["dst_pitch"], 0),
            "model hist": lambda a: lib.accel_model_hist_add(m.handle, a["gt"], a["n"], a["h"], a["w"], a["gt_pitch"], a["out_h"], a["out_w"], a["ncls"], 0),
            "model colour": lambda a: lib.accel_model_labels_colour(m.handle, a["n"], a["out_h"], a["out_w"], a["h"], a["w"], a["pal"], 1, a["frame"],
                                                                    a["frame_pitch"], a["alpha"], 0, a["dst3"], a["dst3_pitch"], 0),
        }
        every = tuple(calls)
        source, hists, colours = ("op source", "model source"), ("op hist", "model hist"), ("op colour", "model colour")
        cases = [(dict(n=0), "n =", every), (dict(n=-1), "n =", every), (dict(h=0), "h =", every), (dict(w=0), "w =", every), (dict(h=-3), "h =", every),
                 (dict(out_h=H + 1), "out_h", every), (dict(out_w=W + 1), "out_w", every), (dict(out_h=0), "out_h", every), (dict(out_w=0), "out_w", every),
                 (dict(H=0), "H x W", ("op source", "op hist", "op colour")),
                 (dict(dst_pitch=cols - 1), "dst_pitch", source), (dict(gt_pitch=cols - 1), "gt_pitch", hists),
                 (dict(dst3_pitch=3 * cols - 1), "dst_pitch", colours), (dict(frame_pitch=3 * cols - 1), "frame_pitch", colours),
                 (dict(ncls=0), "ncls", hists), (dict(ncls=33), "ncls", hists), (dict(alpha=-1), "alpha", colours), (dict(alpha=257), "alpha", colours),
                 (dict(labels=None), "labels", ("op source", "op hist", "op colour")), (dict(dst=None), "dst", source), (dict(dst3=None), "dst", colours),
                 (dict(gt=None), "gt", hists), (dict(hist=None), "hist", ("op hist",)), (dict(pal=None), "palette_rgb", colours),
                 (dict(n=n + 1), "n =", ("model source", "model hist", "model colour")),       # larger than the bound batch
                 (dict(ncls=21), "ncls", ("model hist",))]                                     # the accumulator holds 19 classes since its last clear
        for change, word, names in cases:
            for name in names:
                rc = calls[name](dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (name, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg, (name, change, msg)
        out = np.zeros((21, 21), np.uint64)
        for ncls, word in ((21, "ncls"), (0, "ncls"), (33, "ncls")):
            assert lib.accel_model_hist_read(m.handle, vp(out), ncls, 0) == -1 and word in lib.accel_last_error().decode()
        assert lib.accel_model_hist_read(m.handle, None, 19, 0) == -1 and "out" in lib.accel_last_error().decode()
        assert lib.accel_model_hist_read(None, vp(out), 19, 0) == -1
        bare = runtime.Model(ctx)                               # a model without label maps
        assert lib.accel_model_labels_to_source(bare.handle, 1, 8, 8, 8, 8, vp(dst), 8, 0) == -1 and "labels" in lib.accel_last_error().decode()
        bare.close()
        # none of the refused calls reached the model: generation, labels, accumulator
        assert m.generation("labels") == state[0]
        assert np.array_equal(m.read("labels", (n, H, W), np.uint8), labels)
        assert np.array_equal(m.hist_read(19), state[1])
        assert not dst.any() and not dst3.any() and not hist.any()
        for name in every:                                       # and every call is accepted as it stands
            assert calls[name](good) == 0, (name, lib.accel_last_error().decode())
        src = image.labels_to_source_host(labels, out_h, out_w, rows, cols)
        assert np.array_equal(dst, src) and np.array_equal(dst3, image.colour_host(src, PALETTE, frames=frame, alpha=128))
        assert np.array_equal(hist.astype(np.int64), _fast_hist(src, gt, 19))
        assert np.array_equal(m.hist_read(19), 2 * state[1])
    finally:
        ctx.sync()
        m.close()


def test_demo_finishes_raw_frames_of_another_size_on_the_gpu(demo_cfg, capsys, tmp_path):
    """90 x 180 frames bound at 128 x 256: the loop fetches source-size labels and writes them as PNGs"""
    from PIL import Image
    from accel_amd import demo
    from accel_amd.core import tester
    try:
        demo.main(["--version", "18", "--interval", "3", "--num_ex", "2", "--synthetic", "90x180", "--scales", "128x256", "--raw-frames",
                   "--finish-on-gpu", "--out", str(tmp_path)])
    finally:
        tester.release_models()
    out = capsys.readouterr().out
    assert out.rstrip().endswith("done") and out.count("testing synthetic_") == 6, out[-1500:]
    pngs = sorted(tmp_path.glob("seg_*.png"))
    assert len(pngs) == 6
    assert Image.open(str(pngs[0])).size == (180, 90)
