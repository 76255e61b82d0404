"""Interpolated chroma siting on the GPU (csrc/frames_sited.hip behind accel_frame_yuv_sited / accel_yuv_to_bgr_sited / accel_model_write_yuv_sited /
_commit_yuv_sited): the tensor and the BGR bytes are those accel_amd/utils/image.py builds on the host with siting = s -- BIT FOR BIT; the rule is
integer arithmetic with one rounding, so every comparison is np.array_equal.  The inputs are siting_ref.CASES, the smallest sizes at which the
kernels can go wrong; test_chroma_siting_cpu.py shows that they tell the specification from the usual wrong kernels, and holds the specification
itself to a scalar restatement of the rule."""
import ctypes

import numpy as np
import pytest

import siting_ref as ref
from accel_amd.utils import image, synth

from test_frames_yuv_cpu import MEANS, RESAMPLED, _i420_of_nv12, _tight
from test_frames_nv12_gpu import _same_bytes
from test_frames_u8_gpu import _geometry, _identical, _input_model, _run, _same

pytestmark = pytest.mark.gpu

RANDOM = [c for c in ref.CASES if c.content == "random"]
IMPULSES = [c for c in ref.CASES if c.content != "random"]
IDS = lambda c: "-".join(map(str, c))
BOTH_STEPS = RESAMPLED[:2]        # 44 x 82 -> 48 x 96 (step < 1) and 60 x 120 -> 48 x 96 (step > 1)


def _whole(buf, n, lay):
    """the NV12 keywords of the Python surface take whole frames; the others a buffer that ends with its last frame"""
    if lay["format"] != 3:
        return buf
    out = np.zeros(n * lay["frame_bytes"], np.uint8)
    out[:buf.size] = buf
    return out


def _frame(ctx, buf, n, lay, colour, siting, g):
    if lay["format"] == 3:
        return ctx.frame_nv12(_whole(buf, n, lay), lay["h"], lay["w"], MEANS, colour=colour, siting=siting, **ref.keywords(lay), **g)
    return ctx.frame_yuv(buf, ref.FORMATS[lay["format"]], lay["h"], lay["w"], MEANS, colour=colour, siting=siting, **ref.keywords(lay), **g)


def _bytes(ctx, buf, n, lay, colour, siting, out=None):
    if lay["format"] == 3:
        return ctx.nv12_to_bgr(_whole(buf, n, lay), lay["h"], lay["w"], colour=colour, siting=siting, out=out, **ref.keywords(lay))
    return ctx.yuv_to_bgr(buf, ref.FORMATS[lay["format"]], lay["h"], lay["w"], colour=colour, siting=siting, out=out, **ref.keywords(lay))


def _tensor(bgr, target, max_size, stride=16):
    return np.concatenate([image.transform(image.resize(f, target, max_size, stride=stride)[0], MEANS) for f in bgr]).astype(np.float32)


def _struct(lay, colour):
    from accel_amd import runtime
    return runtime.YUVLayout(*(int(v) for v in (lay["format"], colour, lay["h"], lay["w"], lay["pitch"], lay["pitch_c"], lay["u_offset"],
                                                 lay["v_offset"], lay["frame_bytes"])))


def _tight_of(fmt, n, h, w, seed):
    """(flat bytes, n, layout dict) of n tightly packed random frames of any of the four formats"""
    if fmt == "nv12":
        buf = np.random.default_rng(seed).integers(0, 256, (n, h * w * 3 // 2), dtype=np.uint8)
        lay = dict(format=3, h=h, w=w, pitch=w, pitch_c=0, u_offset=h * w, v_offset=0, frame_bytes=h * w * 3 // 2)
    else:
        buf, lay = _tight(fmt, n, h, w, seed), image.yuv_layout(fmt, h, w)
    return buf.reshape(-1), n, lay


# ---- operator level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RANDOM, ids=IDS)
def test_step_one_copy_and_byte_converter(ctx, case):
    """batches of 3 with frame tails; aligned layouts (the wide loads, every frame) and odd ones (sample by sample, frames at odd addresses);
    stride 16 (float4 stores) and stride 0 (scalar stores with a row tail where w % 4); tight BGR rows and pitched ones whose gaps stay"""
    buf, n, lay = ref.make(case)
    h, w = case.h, case.w
    for siting in (1, 2, 3):
        for colour in (0, 3):
            bgr = ref.expected(case, colour, siting)
            for stride in (16, 0):
                g = _geometry(h, w, min(h, w), max(h, w), stride)
                assert g["step"] == 1.0 and (g["out_h"], g["out_w"]) == (h, w)
                _same(_frame(ctx, buf, n, lay, colour, siting, g), _tensor(bgr, min(h, w), max(h, w), stride), (case, siting, colour, stride))
            _same_bytes(_bytes(ctx, buf, n, lay, colour, siting), bgr, (case, siting, colour))
        for out_pitch in (3 * w + 4, 3 * w + 5):
            before = np.random.default_rng(out_pitch).integers(0, 256, (n, h, out_pitch), dtype=np.uint8)
            out = before.copy()
            assert _bytes(ctx, buf, n, lay, 3, siting, out=out) is out
            _same_bytes(out[:, :, :3 * w].reshape(bgr.shape), ref.expected(case, 3, siting), (case, siting, out_pitch))
            assert np.array_equal(out[:, :, 3 * w:], before[:, :, 3 * w:]), "bytes between the rows were written"


@pytest.mark.parametrize("rows,cols,target,max_size", BOTH_STEPS)
@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_resampled(ctx, fmt, rows, cols, target, max_size):
    buf, n, lay = _tight_of(fmt, 2, rows, cols, rows * 4096 + cols)
    g = _geometry(rows, cols, target, max_size)
    assert g["step"] != 1.0
    for siting in (1, 2, 3):
        for colour in (1, 2):
            want = _tensor(ref.host(buf, lay, colour, siting), target, max_size)
            _same(_frame(ctx, buf, n, lay, colour, siting, g), want, (fmt, rows, cols, siting, colour, g))


@pytest.mark.parametrize("case", [c for c in RANDOM if c.layout in ("odd", "interleaved") and (c.h, c.w) in ((16, 18), (3, 6))], ids=IDS)
def test_resampled_from_pitched_layouts(ctx, case):
    buf, n, lay = ref.make(case)
    h, w = case.h, case.w
    for target, max_size in ((h + h // 2, 2 * w), (max(h // 2, 2), w)):       # enlarged and reduced
        g = _geometry(h, w, target, max_size)
        assert g["step"] != 1.0
        for siting in (1, 2, 3):
            _same(_frame(ctx, buf, n, lay, 1, siting, g), _tensor(ref.expected(case, 1, siting), target, max_size), (case, siting, g))


@pytest.mark.parametrize("case", IMPULSES, ids=IDS)
def test_impulses_through_both_kernels(ctx, case):
    """a single chroma sample at every corner, on an edge and inside: where it spreads to is the siting"""
    buf, n, lay = ref.make(case)
    h, w = case.h, case.w
    for siting in (1, 2, 3):
        bgr = ref.expected(case, 2, siting)
        _same_bytes(_bytes(ctx, buf, n, lay, 2, siting), bgr, (case, siting))
        for target, max_size in ((h, w), (h + h // 2, 2 * w), (h // 2, w)):
            g = _geometry(h, w, target, max_size)
            assert (g["step"] == 1.0) == (target == h)
            _same(_frame(ctx, buf, n, lay, 2, siting, g), _tensor(bgr, target, max_size), (case, siting, g))


def _call_frame(ctx, buf, n, lay, colour, siting, g):
    """accel_frame_yuv_sited itself: (return code, tensor)"""
    from accel_amd import runtime
    out = np.full((n, 3, g["H"], g["W"]), 7.0, np.float32)
    a = np.ascontiguousarray(buf)
    rc = runtime.lib().accel_frame_yuv_sited(ctx.handle, a.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(_struct(lay, colour)),
                                             (ctypes.c_double * 3)(*MEANS), g["out_h"], g["out_w"], ctypes.c_double(g["step"]), g["H"], g["W"],
                                             out.ctypes.data_as(ctypes.c_void_p), siting)
    return rc, out


def _call_bytes(ctx, buf, n, lay, colour, siting):
    from accel_amd import runtime
    out = np.full((n, lay["h"], lay["w"], 3), 7, np.uint8)
    a = np.ascontiguousarray(buf)
    rc = runtime.lib().accel_yuv_to_bgr_sited(ctx.handle, a.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(_struct(lay, colour)),
                                              out.ctypes.data_as(ctypes.c_void_p), 3 * lay["w"], siting, 0)
    return rc, out


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_siting_zero_is_the_existing_entry_point(ctx, fmt):
    """replicate on the new entry points dispatches to the launchers of the replicated kernels: byte for byte what the existing entry points give"""
    for (rows, cols, target, max_size) in ((16, 18, 16, 18), (44, 82, 48, 96)):
        buf, n, lay = _tight_of(fmt, 2, rows, cols, 31 + rows)
        g = _geometry(rows, cols, target, max_size)
        for colour in (0, 3):
            rc, got = _call_frame(ctx, buf, n, lay, colour, 0, g)
            assert rc == 0
            _same(got, _frame(ctx, buf, n, lay, colour, 0, g), (fmt, rows, colour))
            rc, got = _call_bytes(ctx, buf, n, lay, colour, 0)
            assert rc == 0
            _same_bytes(got, _bytes(ctx, buf, n, lay, colour, 0), (fmt, rows, colour))
            _same_bytes(got, ref.host(buf, lay, colour, "replicate"), (fmt, rows, colour, "host"))
    for case in (c for c in RANDOM if c.fmt == fmt and c.layout != "aligned" and (c.h, c.w) == (16, 18)):      # and on pitched layouts
        buf, n, lay = ref.make(case)
        rc, got = _call_bytes(ctx, _whole(buf, n, lay), n, lay, 1, 0)
        assert rc == 0
        _same_bytes(got, ref.expected(case, 1, "replicate"), case)


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_constant_chroma_equals_the_replicated_kernels(ctx, fmt):
    """flat chroma planes under arbitrary luma: every siting interpolates to the same sample, so the sited kernels must give what the existing
    replicated entry points give"""
    h, w = 12, 16
    ch, cw = (h if fmt == "yuy2" else h // 2), w // 2
    top = 1024 if fmt == "p010" else 256
    rng = np.random.default_rng(12)
    planes = [(rng.integers(0, top, (h, w)), np.full((ch, cw), v), np.full((ch, cw), top - 1 - v)) for v in (0, top - 1, top // 3)]
    for name in ("aligned", "odd"):
        lay = ref.layout(fmt, h, w, name)
        buf = ref.place(planes, lay, 13)
        for target, max_size in ((h, w), (18, 32)):
            g = _geometry(h, w, target, max_size)
            want, want_bytes = _frame(ctx, buf, 3, lay, 1, 0, g), _bytes(ctx, buf, 3, lay, 1, 0)
            for siting in (1, 2, 3):
                _same(_frame(ctx, buf, 3, lay, 1, siting, g), want, (fmt, name, siting, g))
                _same_bytes(_bytes(ctx, buf, 3, lay, 1, siting), want_bytes, (fmt, name, siting))


@pytest.mark.parametrize("rows,cols,target,max_size", [(16, 18, 16, 18), (44, 82, 48, 96)])
def test_nv12_and_i420_of_one_picture_agree(ctx, rows, cols, target, max_size):
    """(P010 is not asked to agree: interpolating 4 c and rounding is not 4 times interpolating c)"""
    nv = np.random.default_rng(rows + cols).integers(0, 256, (2, rows * cols * 3 // 2), dtype=np.uint8)
    i420 = _i420_of_nv12(nv, rows, cols)
    g = _geometry(rows, cols, target, max_size)
    for siting in (0, 1, 2, 3):
        for colour in (0, 3):
            _same(ctx.frame_yuv(i420, "i420", rows, cols, MEANS, colour=colour, siting=siting, **g),
                  ctx.frame_nv12(nv, rows, cols, MEANS, colour=colour, siting=siting, **g), (siting, colour))
            _same_bytes(ctx.yuv_to_bgr(i420, "i420", rows, cols, colour=colour, siting=siting),
                        ctx.nv12_to_bgr(nv, rows, cols, colour=colour, siting=siting), (siting, colour))


def test_p010_low_bits_change_nothing(ctx):
    rows, cols = 16, 18
    words = np.random.default_rng(3).integers(0, 1024, (2, rows * cols * 3 // 2)).astype("<u2") << 6
    noisy = words | np.random.default_rng(4).integers(1, 64, words.shape).astype("<u2")
    clean, noisy = words.view(np.uint8).reshape(2, -1), noisy.view(np.uint8).reshape(2, -1)
    assert not np.array_equal(clean, noisy)
    for target, max_size in ((16, 18), (24, 36)):
        g = _geometry(rows, cols, target, max_size)
        for siting in (1, 2, 3):
            want = ctx.frame_yuv(clean, "p010", rows, cols, MEANS, colour=1, siting=siting, **g)
            _same(want, _tensor(image.yuv_to_bgr_host(clean, "p010", rows, cols, colour=1, siting=siting), target, max_size), (siting, g))
            _same(ctx.frame_yuv(noisy, "p010", rows, cols, MEANS, colour=1, siting=siting, **g), want, ("low bits", siting, g))
            _same_bytes(ctx.yuv_to_bgr(noisy, "p010", rows, cols, colour=1, siting=siting),
                        ctx.yuv_to_bgr(clean, "p010", rows, cols, colour=1, siting=siting), ("low bits", siting))


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_device_sources_and_canaries_behind_rows_and_frames(ctx, fmt):
    """the byte converter from HBM into HBM: an aligned source (the wide loads) and the same bytes off every alignment but the one the format
    needs; destination rows with a gap, one more frame behind the batch: nothing but n x h rows of 3 w bytes is written"""
    import torch
    case = next(c for c in RANDOM if c.fmt == fmt and (c.h, c.w) == (16, 18) and c.layout == "aligned")
    buf, n, lay = ref.make(case)
    h, w = case.h, case.w
    st = _struct(lay, 2)
    for off in (0, 2 if fmt == "p010" else 1):
        dev = torch.zeros(buf.size + 8, dtype=torch.uint8, device="cuda")
        dev[off:off + buf.size] = torch.from_numpy(np.array(buf))
        for out_pitch, shift in ((3 * w + 2, 0), (3 * w + 7, 1)):       # dword stores need a 4-byte aligned destination and pitch
            for siting in (1, 2, 3):
                out = torch.full(((n + 1) * h * out_pitch + 8,), 201, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()              # torch's stream and the library's stream are not ordered by themselves
                from accel_amd import runtime
                rc = runtime.lib().accel_yuv_to_bgr_sited(ctx.handle, ctypes.c_void_p(dev.data_ptr() + off), n, ctypes.byref(st),
                                                          ctypes.c_void_p(out.data_ptr() + shift), out_pitch, siting, 1)
                assert rc == 0, runtime.lib().accel_last_error().decode()
                ctx.sync()
                got = out.cpu().numpy()
                assert np.all(got[:shift] == 201) and np.all(got[shift + n * h * out_pitch:] == 201), "bytes behind the last frame were written"
                rows = got[shift:shift + n * h * out_pitch].reshape(n, h, out_pitch)
                _same_bytes(np.ascontiguousarray(rows[:, :, :3 * w]).reshape(n, h, w, 3), ref.expected(case, 2, siting), (fmt, off, out_pitch, siting))
                assert np.all(rows[:, :, 3 * w:] == 201), "bytes between the rows were written"
                # and through the Python surface
                out.fill_(201)
                torch.cuda.synchronize()
                if fmt == "nv12":
                    ctx.nv12_to_bgr_device(dev.data_ptr() + off, out.data_ptr() + shift, n, h, w, lay["pitch"], lay["u_offset"], lay["frame_bytes"], 2,
                                           out_pitch, siting=siting)
                else:
                    ctx.yuv_to_bgr_device(dev.data_ptr() + off, out.data_ptr() + shift, n, dict(lay, colour=2), out_pitch, siting=siting)
                ctx.sync()
                assert np.array_equal(out.cpu().numpy(), got)
        del dev, out


# ---- model level --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_model_write_prefetch_commit_and_device_source(ctx, fmt):
    import torch
    from accel_amd import runtime
    rows, cols, target, max_size = 44, 82, 48, 96
    g = _geometry(rows, cols, target, max_size)
    H, W = g["H"], g["W"]
    frames = [_tight_of(fmt, 1, rows, cols, 500 + i) for i in range(3)]
    lay = frames[0][2]
    fa, fb, fc = (f[0] for f in frames)
    host = lambda f, s: _tensor(ref.host(f, lay, 2, s), target, max_size)
    nv = (lay["pitch"], lay["u_offset"], lay["frame_bytes"], 2)
    m = _input_model(ctx, H, W)
    pin = runtime.PinnedBuffer(fa.shape, np.uint8)
    try:
        def write(f, s):
            if fmt == "nv12":
                m.write_nv12("data", f, rows, cols, MEANS, colour=2, siting=s, **g)
            else:
                m.write_yuv("data", f, fmt, rows, cols, MEANS, colour=2, siting=s, **g)

        def commit(s):
            if fmt == "nv12":
                m.commit_nv12("data", 1, rows, cols, *nv, MEANS, siting=s, **g)
            else:
                m.commit_yuv("data", 1, dict(lay, colour=2), MEANS, siting=s, **g)

        for s in ("left", "centre", "topleft", 0):
            write(fa, s)
            _same(m.read("data", (1, 3, H, W)), host(fa, s), ("write", fmt, s))
        gen = m.generation("data")
        write(fc, 2)
        assert m.generation("data") == gen + 1
        # the overlapped upload: the bytes on the copy stream into the uint8 shadow, converted with sited chroma at commit
        with pytest.raises(runtime.AccelError, match="no uint8 frames were prefetched"):
            commit(1)
        for f, s in ((fb, 1), (fa, 3), (fc, 2)):
            pin.array[...] = f
            m.prefetch_u8("data", pin)
            commit(s)
            _same(m.read("data", (1, 3, H, W)), host(f, s), ("prefetch_u8 + commit", fmt, s))
        # a device-resident source off every alignment but the one the format needs, read in place into the other input
        off = 2 if fmt == "p010" else 1
        dev = torch.zeros(fc.size + off, dtype=torch.uint8, device="cuda")
        dev[off:] = torch.from_numpy(fc)
        torch.cuda.synchronize()
        for s in (1, 2, 3):
            if fmt == "nv12":
                m.write_nv12_device("data_key", dev.data_ptr() + off, 1, rows, cols, *nv, MEANS, siting=s, **g)
            else:
                m.write_yuv_device("data_key", dev.data_ptr() + off, 1, dict(lay, colour=2), MEANS, siting=s, **g)
            _same(m.read("data_key", (1, 3, H, W)), host(fc, s), ("device source", fmt, s))
        _same(m.read("data", (1, 3, H, W)), host(fc, 2), "the other input is untouched")
        del dev
    finally:
        ctx.sync()
        pin.close()
        m.close()


def test_argument_errors_return_err_arg(ctx):
    """what the kernels could not honour is refused before anything is enqueued, with a message that names the argument; nothing is written"""
    from accel_amd import runtime
    lib = runtime.lib()
    rows, cols = 44, 82
    g = _geometry(rows, cols, 48, 96)
    H, W = g["H"], g["W"]
    means = (ctypes.c_double * 3)(*MEANS)
    out = np.full((1, 3, H, W), 7.0, np.float32)
    bgr = np.full((1, rows, cols, 3), 7, np.uint8)
    m = _input_model(ctx, H, W)
    pin = runtime.PinnedBuffer((rows * cols * 3,), np.uint8)
    try:
        for fmt in ref.FORMATS:
            f, _, lay = _tight_of(fmt, 1, rows, cols, 9)
            src = f.ctypes.data_as(ctypes.c_void_p)
            write_ok = lambda: lib.accel_model_write_yuv_sited(m.handle, b"data", src, 1, ctypes.byref(_struct(lay, 0)), means, g["out_h"], g["out_w"],
                                                               ctypes.c_double(g["step"]), H, W, 2, 0)
            assert write_ok() == 0, lib.accel_last_error().decode()
            want = m.read("data", (1, 3, H, W))
            _same(want, _tensor(ref.host(f, lay, 0, 2), 48, 96), fmt)
            pin.array[:f.size] = f
            m.prefetch_u8("data", pin)
            good = dict(lay, siting=1)
            cases = [(dict(siting=-1), "siting"), (dict(siting=4), "siting"), (dict(format=-1), "format"), (dict(format=4), "format")]
            if fmt == "nv12":
                cases += [(dict(pitch_c=cols), "pitch_c"), (dict(v_offset=lay["frame_bytes"]), "v_offset"), (dict(u_offset=rows * cols - 2), "u_offset"),
                          (dict(frame_bytes=ref.extent(lay) - 1), "frame_bytes"), (dict(h=rows + 1), "h ="), (dict(w=cols - 1), "w ="),
                          (dict(pitch=cols - 2), "pitch")]
            else:           # the checks of the yuv entry points still hold: format 3 is not a way around them
                cases += [(dict(frame_bytes=ref.extent(lay) - 2), "frame_bytes"), (dict(w=cols - 1), "w =")]
            for change, word in cases:
                a = dict(good, **change)
                st, siting = ctypes.byref(_struct(a, 0)), a["siting"]
                res = (g["out_h"], g["out_w"], ctypes.c_double(g["step"]), H, W)
                calls = {"frame": lambda: lib.accel_frame_yuv_sited(ctx.handle, src, 1, st, means, *res, out.ctypes.data_as(ctypes.c_void_p), siting),
                         "to_bgr": lambda: lib.accel_yuv_to_bgr_sited(ctx.handle, src, 1, st, bgr.ctypes.data_as(ctypes.c_void_p), 3 * cols, siting, 0),
                         "write": lambda: lib.accel_model_write_yuv_sited(m.handle, b"data", src, 1, st, means, *res, siting, 0),
                         "commit": lambda: lib.accel_model_commit_yuv_sited(m.handle, b"data", 1, st, means, *res, siting)}
                for name, call in calls.items():
                    rc = call()
                    msg = lib.accel_last_error().decode()
                    assert rc == -1, (fmt, name, change, rc, msg)       # ACCEL_ERR_ARG
                    assert word in msg, (fmt, name, change, msg)
            # none of the refused calls touched a target or consumed the prefetch
            assert np.all(out == 7.0) and np.all(bgr == 7)
            _same(m.read("data", (1, 3, H, W)), want, "after the refused calls")
            assert lib.accel_model_commit_yuv_sited(m.handle, b"data", 1, ctypes.byref(_struct(lay, 0)), means, g["out_h"], g["out_w"],
                                                    ctypes.c_double(g["step"]), H, W, 2) == 0
            _same(m.read("data", (1, 3, H, W)), want, "commit after the refused calls")
        # the existing entry points still refuse format 3: nothing was folded into their arguments
        f, _, lay = _tight_of("nv12", 1, rows, cols, 9)
        rc = lib.accel_frame_yuv(ctx.handle, f.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(_struct(lay, 0)), means, g["out_h"], g["out_w"],
                                 ctypes.c_double(g["step"]), H, W, out.ctypes.data_as(ctypes.c_void_p))
        assert rc == -1 and "format" in lib.accel_last_error().decode() and np.all(out == 7.0)
    finally:
        ctx.sync()
        pin.close()
        m.close()


# ---- whole path ---------------------------------------------------------------------------------------------------------------------------
def test_sited_nv12_frames_give_the_logits_of_their_bgr_frames(demo_cfg):
    """Accel-18, 4 frames of 120 x 250 (resampled), interval 3: NV12 frames with siting = left must give BIT-IDENTICAL logits and labels to raw BGR
    frames of their host conversion -- through the plain loop and the pinned prefetch loop, with nothing converted on the host -- and they
    differ from what replicated chroma gives"""
    from accel_amd import demo, mx
    from accel_amd.core import results, tester
    from test_results_gpu import PALETTE
    H, W, rows, cols = 128, 256, 120, 250
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = 16
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    clip = synth.make_clip(rows, cols, 4)
    nv = [image.bgr_to_nv12_host(f, 2, siting="left") for f in clip]
    bgr = [image.nv12_to_bgr_host(b, rows, cols, colour=2, siting="left")[0] for b in nv]
    assert not np.array_equal(bgr[0], image.nv12_to_bgr_host(nv[0], rows, cols, colour=2)[0])
    zero = mx.nd.array(np.zeros((1, demo_cfg.network.DFF_FEAT_DIM, 1, 1)))

    def batches(ctx=None, siting="left"):
        arrs = [mx.nd.nv12_frames(b, rows, cols, demo_cfg, colour=2, ctx=ctx, siting=siting) for b in nv]
        return [[arrs[t], arrs[t - 1] if t else arrs[0], zero] for t in range(len(arrs))]
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        want = _run(r, demo.build_batches(bgr, demo_cfg, raw=True), 3)
        plain = batches()
        assert plain[0][0].siting == 1
        _identical(_run(r, plain, 3), want, "sited NV12 frames, plain loop")
        assert plain[0][0]._host is None and plain[0][0]._frames is None, "the NV12 route must not convert anything on the host"
        pinned = batches(ctx=mx.cpu_pinned())
        _identical(_run(r, pinned, 3, prefetch=True), want, "sited NV12 frames, pinned prefetch loop")
        assert pinned[1][0]._host is None and pinned[1][0]._frames is None
        replicated = _run(r, batches(siting="replicate"), 3)
        assert not np.array_equal(replicated[0][0], want[0][0])
        # the colour image is blended over the picture the network saw
        lg, lab = r.step(0, plain[0], 3)
        like = plain[0][0]
        src = image.labels_to_source_host(lab.asnumpy(), like.geometry["out_h"], like.geometry["out_w"], rows, cols)
        assert np.array_equal(results.colour(lab, like, PALETTE, frames=True, alpha=128), image.colour_host(src, PALETTE, frames=bgr[0][None], alpha=128))
    finally:
        tester.release_models()
