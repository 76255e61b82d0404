"""I420, P010 and YUY2 video frames, host side: the host specification (utils/image.py yuv_to_bgr_host) is tied to the NV12 route already proven on
all 2^24 triples, P010's integer rule is a fair restatement of the standards' float matrices at 10 bits, yuv_layout gives the stated defaults and
refuses what the C ABI refuses, and the cases of the GPU file can tell a correct reader from the usual wrong ones.  (GPU side:
test_frames_yuv_gpu.py, which imports the helpers below.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from accel_amd.utils import image

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
MEANS = (103.06, 115.9, 123.15)
FORMATS = ("i420", "p010", "yuy2")
ENTRY_POINTS = ("accel_yuv10_coefficients", "accel_frame_yuv", "accel_yuv_to_bgr", "accel_model_write_yuv", "accel_model_commit_yuv")

# what the GPU file runs: step 1 (rows, cols, stride) and resampled (rows, cols, target, max)
COPIES = [(48, 96, 16), (96, 48, 16), (2, 2, 16), (16, 18, 16), (30, 50, 0)]
COPIES_YUY2 = COPIES + [(3, 6, 16)]          # an odd height
RESAMPLED = [(44, 82, 48, 96), (60, 120, 48, 96), (22, 150, 48, 96)]


def _copies(fmt):
    return COPIES_YUY2 if fmt == "yuy2" else COPIES


def _tight_bytes(fmt, h, w):
    return {"i420": h * w * 3 // 2, "p010": h * w * 3, "yuy2": h * w * 2}[fmt]


def _tight(fmt, n, h, w, seed):
    """n tightly packed frames of random bytes: luma and both chroma components independent, all 16 bits of every P010 word random (so the low
    six are noise)"""
    return np.random.default_rng(seed).integers(0, 256, (n, _tight_bytes(fmt, h, w)), dtype=np.uint8)


def _planes(lay):
    """(offset, rows, bytes per row, pitch) of every plane of a layout"""
    f, h, w = lay["format"], lay["h"], lay["w"]
    if f == 0:
        return [(0, h, w, lay["pitch"]), (lay["u_offset"], h // 2, w // 2, lay["pitch_c"]), (lay["v_offset"], h // 2, w // 2, lay["pitch_c"])]
    if f == 1:
        return [(0, h, 2 * w, lay["pitch"]), (lay["u_offset"], h // 2, 2 * w, lay["pitch"])]
    return [(0, h, 2 * w, lay["pitch"])]


def _spread(fmt, tight, h, w, seed, tail=0, **layout):
    """the frames of `tight` laid out as the layout keywords say, NON-ZERO random bytes in every gap; `tail` bytes of it after the last frame
    are cut off (a host buffer may end with the last byte of its last frame).  Returns (flat bytes, layout)."""
    lay = image.yuv_layout(fmt, h, w, **layout)
    src = image.yuv_layout(fmt, h, w)
    n, fb = tight.shape[0], lay["frame_bytes"]
    out = np.random.default_rng(seed).integers(1, 256, n * fb, dtype=np.uint8)
    for i in range(n):
        for (so, rows, rb, sp), (do, _, _, dp) in zip(_planes(src), _planes(lay)):
            for y in range(rows):
                out[i * fb + do + y * dp:i * fb + do + y * dp + rb] = tight[i, so + y * sp:so + y * sp + rb]
    return out[:out.size - tail] if tail else out, lay


def _keywords(lay):
    return {k: lay[k] for k in ("pitch", "pitch_c", "u_offset", "v_offset", "frame_bytes") if lay[k] or k in ("pitch", "frame_bytes")}


def _host(buf, fmt, rows, cols, target, max_size, stride=16, means=MEANS, colour=0, **layout):
    bgr = image.yuv_to_bgr_host(buf, fmt, rows, cols, colour=colour, **layout)
    return np.concatenate([image.transform(image.resize(f, target, max_size, stride=stride)[0], means) for f in bgr]).astype(np.float32)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from accel_amd import runtime
    hdr = open(os.path.join(ROOT, "include", "accel_hip.h")).read()
    declared = set(re.findall(r"\b(accel_[a-z0-9_]+)\s*\(", hdr))
    assert "accel_yuv_layout" in hdr
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, "include/accel_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libaccel_hip.so does not export %s" % name
    runtime.lib()
    assert set(ENTRY_POINTS) <= set(runtime.EXPORTS)
    for name in ("frame_yuv", "yuv_to_bgr", "yuv_to_bgr_device"):
        assert hasattr(runtime.Context, name)
    for name in ("write_yuv", "write_yuv_device", "commit_yuv"):
        assert hasattr(runtime.Model, name)
    # the ctypes structure is the C one: four ints and five size_t
    assert [f[0] for f in runtime.YUVLayout._fields_] == ["format", "colour", "h", "w", "pitch", "pitch_c", "u_offset", "v_offset", "frame_bytes"]
    assert ctypes.sizeof(runtime.YUVLayout) == 4 * ctypes.sizeof(ctypes.c_int) + 5 * ctypes.sizeof(ctypes.c_size_t)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name
    assert "nor are P010, I420 or YUY2" not in doc


def test_coefficients_equal_the_formula_and_the_library():
    from accel_amd import runtime
    assert image.YUV_FORMATS == {"i420": 0, "p010": 1, "yuy2": 2}
    for c in range(4):
        m = image.nv12_matrix(c)
        if c in (0, 2):       # limited range: the 10-bit signal is 4 times the 8-bit one, the same integers serve
            want = image.nv12_coefficients(c)
        else:                 # full range: 1023, not 1020, is white
            want = (0,) + tuple(int(round(65536.0 * v * 1020.0 / 1023.0)) for v in m[1:])
        assert image.yuv10_coefficients(c) == want
        assert runtime.yuv10_coefficients(c) == want
        # |accumulator| < 1.5e8: int32 holds
        yoff, ky, krv, kgu, kgv, kbu = want
        assert ky * 1023 + max(krv, kbu, kgu + kgv) * 512 + (1 << 17) < 1.5e8
    out = (ctypes.c_int32 * 6)()
    for bad in (-1, 4):
        assert runtime.lib().accel_yuv10_coefficients(bad, out) == -1       # ACCEL_ERR_ARG
        assert "colour" in runtime.lib().accel_last_error().decode()
        with pytest.raises(ValueError, match="colour"):
            image.yuv10_coefficients(bad)


# ---- the 8-bit formats and limited-range P010 against NV12 ---------------------------------------------------------------------------------
def _i420_of_nv12(nv, h, w):
    n = nv.shape[0]
    uv = nv[:, h * w:].reshape(n, h // 2, w // 2, 2)
    return np.concatenate([nv[:, :h * w], uv[..., 0].reshape(n, -1), uv[..., 1].reshape(n, -1)], axis=1)


def _yuy2_of_nv12(nv, h, w):
    n = nv.shape[0]
    uv = np.repeat(nv[:, h * w:].reshape(n, h // 2, w // 2, 2), 2, axis=1)        # every chroma row serves two rows
    luma = nv[:, :h * w].reshape(n, h, w // 2, 2)
    return np.stack([luma[..., 0], uv[..., 0], luma[..., 1], uv[..., 1]], axis=-1).reshape(n, -1)


def _p010_of_nv12(nv, low=None):
    """word = byte << 8, optionally with noise in the low six bits"""
    words = nv.astype("<u2") << 8
    if low is not None:
        words = words | np.random.default_rng(low).integers(0, 64, words.shape).astype("<u2")
    return np.ascontiguousarray(words).view(np.uint8).reshape(nv.shape[0], -1)


@pytest.mark.parametrize("colour", [0, 1, 2, 3])
@pytest.mark.parametrize("h,w", [(6, 10), (48, 96), (2, 2)])
def test_eight_bit_formats_equal_the_nv12_conversion(h, w, colour):
    nv = np.random.default_rng(h * 100 + w).integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    want = image.nv12_to_bgr_host(nv, h, w, colour=colour)
    assert np.array_equal(image.yuv_to_bgr_host(_i420_of_nv12(nv, h, w), "i420", h, w, colour=colour), want)
    assert np.array_equal(image.yuv_to_bgr_host(_yuy2_of_nv12(nv, h, w), "yuy2", h, w, colour=colour), want)


@pytest.mark.parametrize("colour", [0, 2])
@pytest.mark.parametrize("h,w", [(6, 10), (48, 96), (2, 2)])
def test_p010_limited_range_equals_the_nv12_conversion(h, w, colour):
    """word = byte << 8 is the 10-bit sample 4 x byte: the accumulator is 4 times the 8-bit one and the shift two places longer"""
    nv = np.random.default_rng(h * 100 + w + 1).integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    assert np.array_equal(image.yuv_to_bgr_host(_p010_of_nv12(nv), "p010", h, w, colour=colour), image.nv12_to_bgr_host(nv, h, w, colour=colour))


@pytest.mark.parametrize("colour", [0, 1, 2, 3])
def test_p010_low_bits_are_never_looked_at(colour):
    h, w = 16, 18
    words = np.random.default_rng(5).integers(0, 1024, (2, h * w * 3 // 2)).astype("<u2") << 6
    noisy = words | np.random.default_rng(6).integers(1, 64, words.shape).astype("<u2")
    clean = image.yuv_to_bgr_host(words.view(np.uint8), "p010", h, w, colour=colour)
    assert np.array_equal(image.yuv_to_bgr_host(noisy.view(np.uint8), "p010", h, w, colour=colour), clean)
    assert np.array_equal(image.yuv_to_bgr_host(noisy, "p010", h, w, colour=colour), clean)       # uint16 words are viewed as bytes


@pytest.mark.parametrize("colour", [0, 1, 2, 3])
def test_p010_integer_rule_is_within_one_level_of_the_float_matrix(colour):
    """The integer rule against clip(rint(the standard's float64 matrix at 10 bits)) on a lattice of every 8th value per component (2^21
    triples), the eight corners of the cube and the planes Y10 in {0, 64, 940, 1023} (4 x 2^20 triples): never more than one level apart.
    Measured share of (triple, channel) results that differ by that one level, per colour mode and set:
        lattice   0: 1.45e-04   1: 2.26e-04   2: 1.77e-04   3: 2.50e-04
        planes    0: 2.56e-04   1: 2.12e-04   2: 6.92e-05   3: 4.56e-04
        corners   none
    -- fewer than 1 in 2000, beside NV12's "fewer than 1 in 1000".  The share is measured and printed, not asserted."""
    yoff, ky, krv, kgu, kgv, kbu = image.yuv10_matrix(colour)
    quant = lambda a: np.clip(np.rint(a), 0, 255).astype(np.int64)

    def apart(y, cb, cr):
        y, cb, cr = (np.asarray(v, np.int64).reshape(-1) for v in (y, cb, cr))
        b, g, r = image.yuv10_to_bgr(y, cb, cr, colour)
        yf, d, e = ky * (y.astype(np.float64) - yoff), cb.astype(np.float64) - 512.0, cr.astype(np.float64) - 512.0
        diff = np.stack([np.abs(got.astype(np.int64) - want) for got, want in ((r, quant(yf + krv * e)), (g, quant(yf - kgu * d - kgv * e)),
                                                                                   (b, quant(yf + kbu * d)))])
        return int(diff.max()), float(np.count_nonzero(diff)) / diff.size

    v8, v = np.arange(0, 1024, 8), np.arange(1024)
    sets = {"lattice": np.meshgrid(v8, v8, v8, indexing="ij"),
            "corners": np.meshgrid([0, 1023], [0, 1023], [0, 1023], indexing="ij"),
            "planes": np.meshgrid([0, 64, 940, 1023], v, v, indexing="ij")}
    for name, (y, cb, cr) in sets.items():
        worst, share = apart(y, cb, cr)
        print("colour %d %s: max %d level(s), share %.3g" % (colour, name, worst, share))
        assert worst <= 1, (colour, name, worst)


@pytest.mark.parametrize("colour", [0, 1, 2, 3])
def test_p010_known_answers(colour):
    v = np.arange(1024)
    grey = np.full(1024, 512)
    b, g, r = image.yuv10_to_bgr(v, grey, grey, colour)
    assert np.array_equal(b, g) and np.array_equal(g, r)        # no chroma: a grey pixel
    if colour in (1, 3):
        assert g[0] == 0 and g[1023] == 255 and g[1020] == 254   # 1023, not 1020, is white
        assert np.all(np.diff(g.astype(int)) >= 0)
    else:
        assert g[64] == 0 and g[940] == 255 and np.all(g[:64] == 0) and np.all(g[940:] == 255)
    b, g, r = image.yuv10_to_bgr([1023, 0], [1023, 0], [1023, 0], colour)       # strong chroma saturates instead of wrapping
    assert (b[0], r[0]) == (255, 255) and (b[1], r[1]) == (0, 0)


# ---- layout ---------------------------------------------------------------------------------------------------------------------------------
def test_yuv_layout_gives_the_stated_defaults():
    h, w = 6, 10
    assert image.yuv_layout("i420", h, w) == dict(format=0, h=h, w=w, pitch=w, pitch_c=w // 2, u_offset=h * w, v_offset=h * w + h * w // 4,
                                                  frame_bytes=h * w * 3 // 2)
    assert image.yuv_layout("p010", h, w) == dict(format=1, h=h, w=w, pitch=2 * w, pitch_c=0, u_offset=2 * h * w, v_offset=0, frame_bytes=3 * h * w)
    assert image.yuv_layout("yuy2", h, w) == dict(format=2, h=h, w=w, pitch=2 * w, pitch_c=0, u_offset=0, v_offset=0, frame_bytes=2 * h * w)
    assert image.yuv_layout(2, 3, 6)["frame_bytes"] == 36          # YUY2 may have an odd height
    assert image.yuv_layout("I420", h, w) == image.yuv_layout(0, h, w)
    lay = image.yuv_layout("i420", h, w, pitch=16)
    assert (lay["pitch_c"], lay["u_offset"], lay["v_offset"], lay["frame_bytes"]) == (8, 96, 120, 120 + 2 * 8 + 5)
    # YV12, and rows interleaved: the chroma planes need not be disjoint from each other
    assert image.yuv_layout("i420", h, w, u_offset=75, v_offset=60)["frame_bytes"] == 90
    inter = image.yuv_layout("i420", h, w, pitch=16, pitch_c=16, u_offset=96, v_offset=104)
    assert inter["frame_bytes"] == 104 + 2 * 16 + 5 and image.yuv_extent(inter) == inter["frame_bytes"]
    assert image.yuv_layout("p010", h, w, pitch=24, u_offset=160)["frame_bytes"] == 160 + 2 * 24 + 20
    assert image.yuv_layout("yuy2", h, w, pitch=23)["frame_bytes"] == 5 * 23 + 20


REFUSED = [("i420", dict(h=7), "h ="), ("i420", dict(w=9), "w ="), ("p010", dict(h=7), "h ="), ("p010", dict(w=9), "w ="), ("yuy2", dict(w=9), "w ="),
           ("i420", dict(h=0), "h ="), ("yuy2", dict(h=0), "h ="), ("i420", dict(w=0), "w ="), ("i420", dict(h=32770), "h ="),
           ("yuy2", dict(w=32770), "w ="), ("i420", dict(pitch=9), "pitch"), ("p010", dict(pitch=18), "pitch"), ("yuy2", dict(pitch=19), "pitch"),
           ("i420", dict(pitch_c=4), "pitch_c"), ("i420", dict(u_offset=59), "u_offset"), ("i420", dict(v_offset=59), "v_offset"),
           ("p010", dict(u_offset=118), "u_offset"), ("i420", dict(frame_bytes=89), "frame_bytes"), ("p010", dict(frame_bytes=178), "frame_bytes"),
           ("yuy2", dict(frame_bytes=119), "frame_bytes"), ("i420", dict(pitch=12), "frame_bytes", dict(frame_bytes=90)),
           ("p010", dict(pitch_c=10), "pitch_c"), ("p010", dict(v_offset=150), "v_offset"), ("yuy2", dict(pitch_c=10), "pitch_c"),
           ("yuy2", dict(v_offset=150), "v_offset"), ("yuy2", dict(u_offset=120), "u_offset"),
           ("p010", dict(pitch=21), "pitch"), ("p010", dict(u_offset=121), "u_offset"), ("p010", dict(frame_bytes=181), "frame_bytes")]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "%s-%s" % (c[0], "-".join("%s%s" % kv for kv in c[1].items())))
def test_yuv_layout_refuses_what_the_c_abi_refuses(case):
    fmt, change, word = case[:3]
    args = dict(dict(h=6, w=10), **change)
    if len(case) > 3:
        args.update(case[3])
    with pytest.raises(ValueError, match=word):
        image.yuv_layout(fmt, **args)
    for bad in ("nv21", 3, -1, None):
        with pytest.raises(ValueError, match="format"):
            image.yuv_layout(bad, 6, 10)


def test_layout_gaps_are_not_interpreted_and_buffers_may_end_with_the_last_frame():
    h, w = 6, 10
    for fmt, layouts in (("i420", [dict(pitch=17, pitch_c=7, u_offset=17 * 8, v_offset=17 * 8 + 40, frame_bytes=260),
                                   dict(pitch=16, pitch_c=16, u_offset=96, v_offset=104),                       # rows interleaved
                                   dict(u_offset=75, v_offset=60)]),                                              # YV12
                         ("p010", [dict(pitch=22, u_offset=22 * 7, frame_bytes=22 * 7 + 3 * 22 + 6)]),
                         ("yuy2", [dict(pitch=23, frame_bytes=6 * 23 + 5)])):
        tight = _tight(fmt, 2, h, w, 1)
        want = image.yuv_to_bgr_host(tight, fmt, h, w, colour=2)
        assert want.shape == (2, h, w, 3) and want.dtype == np.uint8
        assert np.array_equal(image.yuv_to_bgr_host(tight.reshape(-1), fmt, h, w, colour=2), want)       # a flat run of whole frames
        for layout in layouts:
            for seed in (2, 3):
                spread, lay = _spread(fmt, tight, h, w, seed, **layout)
                assert np.array_equal(image.yuv_to_bgr_host(spread, fmt, h, w, colour=2, **layout), want), (fmt, layout)
            tail = lay["frame_bytes"] - image.yuv_extent(lay)
            if tail:
                assert np.array_equal(image.yuv_to_bgr_host(spread[:spread.size - tail], fmt, h, w, colour=2, **_keywords(lay)), want)
                with pytest.raises(ValueError, match="frame_bytes"):
                    image.yuv_to_bgr_host(spread[:spread.size - tail - 1], fmt, h, w, colour=2, **_keywords(lay))
        with pytest.raises(ValueError, match="uint8"):
            image.yuv_to_bgr_host(tight.astype(np.float32), fmt, h, w)
    with pytest.raises(ValueError, match="uint8"):
        image.yuv_to_bgr_host(np.zeros(90, np.uint16), "i420", h, w)              # words are P010's alone
    # replicated chroma in (Cb, Cr) order: YUY2 takes it from its own row, I420 from the row pair
    quads = np.uint8([[50, 90, 100, 240, 150, 30, 200, 60]])
    got = image.yuv_to_bgr_host(quads, "yuy2", 2, 2, colour=1)[0]
    for (y, x), (luma, cb, cr) in zip(((0, 0), (0, 1), (1, 0), (1, 1)), ((50, 90, 240), (100, 90, 240), (150, 30, 60), (200, 30, 60))):
        assert tuple(got[y, x]) == tuple(int(v) for v in image.yuv_to_bgr(luma, cb, cr, 1))
    got = image.yuv_to_bgr_host(np.uint8([[50, 100, 150, 200, 90, 240]]), "i420", 2, 2, colour=1)[0]
    for (y, x), luma in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (50, 100, 150, 200)):
        assert tuple(got[y, x]) == tuple(int(v) for v in image.yuv_to_bgr(luma, 90, 240, 1))


# ---- the cases of the GPU file tell a correct reader from the usual wrong ones -------------------------------------------------------------
def _addresses(lay, mutant=None):
    """byte addresses (luma, cb, cr) of every pixel of frame 0, h x w each, as a correct reader computes them -- or as a reader with one
    of the usual mistakes does"""
    f, h, w, pitch = lay["format"], lay["h"], lay["w"], lay["pitch"]
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    cx = xs if mutant == "chroma_x" else xs >> 1
    cy = ys if mutant == "chroma_y" else ys >> 1
    if f == 0:
        step = pitch if mutant == "chroma_pitch" else lay["pitch_c"]
        luma, cb, cr = ys * pitch + xs, lay["u_offset"] + cy * step + cx, lay["v_offset"] + cy * step + cx
    elif f == 2:
        quad = ys * pitch + 4 * ((xs >> 1) + (1 if mutant == "next_quad" else 0))
        luma, cb, cr = ys * pitch + 2 * xs, quad + 1, quad + 3
    else:
        uv = lay["u_offset"] + cy * pitch + 4 * cx
        luma, cb, cr = ys * pitch + 2 * xs, uv, uv + 2
    if mutant == "swap":
        cb, cr = cr, cb
    return np.broadcast_to(luma, (h, w)), np.broadcast_to(cb, (h, w)), np.broadcast_to(cr, (h, w))


def _read(a, lay, colour, mutant=None):
    luma, cb, cr = _addresses(lay, mutant)
    if lay["format"] != 1:
        return np.stack(image.yuv_to_bgr(a[luma], a[cb], a[cr], colour), axis=-1)
    lo, hi = (1, 0) if mutant == "big_endian" else (0, 1)
    word = lambda i: a[i + lo].astype(np.int32) | a[i + hi].astype(np.int32) << 8
    sample = (lambda i: word(i) & 1023) if mutant == "low_ten_bits" else (lambda i: word(i) >> 6)
    return np.stack(image.yuv10_to_bgr(sample(luma), sample(cb), sample(cr), colour), axis=-1)


MUTANTS = {"i420": ("swap", "chroma_x", "chroma_y", "chroma_pitch"), "p010": ("swap", "chroma_x", "chroma_y", "low_ten_bits", "big_endian"),
           "yuy2": ("swap", "next_quad")}


@pytest.mark.parametrize("fmt", FORMATS)
def test_case_shapes_tell_a_correct_reader_from_the_wrong_ones(fmt):
    """Wrong host readers -- Cb and Cr swapped; chroma from (x, y >> 1) or (x >> 1, y); the chroma row advanced by `pitch` instead of `pitch_c`;
    YUY2's chroma of the next quad; P010 read as word & 1023 or big-endian -- must differ from the specification on the frames the GPU file uses,
    at every case shape.  (A wrong reader runs past the frame: a run of random bytes follows it here.)  One combination is no mutant at all and
    is held to be IDENTICAL instead: with h = 2 there is a single chroma row, which `pitch` and `pitch_c` place at the same address."""
    shapes = [(r, c) for r, c, _ in _copies(fmt)] + [(r, c) for r, c, _, _ in RESAMPLED]
    for h, w in shapes:
        lay = image.yuv_layout(fmt, h, w)
        frame = _tight(fmt, 1, h, w, h * 4096 + w)[0]
        a = np.concatenate([frame, np.random.default_rng(h + w).integers(0, 256, 4 * frame.size + 64, dtype=np.uint8)])
        for colour in (0, 3):
            want = image.yuv_to_bgr_host(frame, fmt, h, w, colour=colour)[0]
            assert np.array_equal(_read(a, lay, colour), want), (fmt, h, w, "the correct reader")
            for mutant in MUTANTS[fmt]:
                same_addresses = all(np.array_equal(p, q) for p, q in zip(_addresses(lay), _addresses(lay, mutant)))
                if mutant == "chroma_pitch" and h == 2:
                    assert same_addresses and np.array_equal(_read(a, lay, colour, mutant), want)
                else:
                    assert not np.array_equal(_read(a, lay, colour, mutant), want), (fmt, h, w, colour, mutant)


# ---- the array, the batches and the demo ---------------------------------------------------------------------------------------------------
def _cfg(demo_cfg, target, max_size, stride):
    demo_cfg.SCALES[0] = (target, max_size)
    demo_cfg.network.IMAGE_STRIDE = stride
    return demo_cfg


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("rows,cols,target,max_size", [(48, 96, 48, 96), (44, 82, 48, 96)])
def test_yuv_array_stands_for_the_host_tensor(demo_cfg, fmt, rows, cols, target, max_size):
    from accel_amd import mx
    cfg = _cfg(demo_cfg, target, max_size, 16)
    buf = _tight(fmt, 2, rows, cols, rows * 1000 + cols)
    keep = buf.copy()
    arr = mx.nd.yuv_frames(buf, fmt, rows, cols, cfg)
    assert isinstance(arr, mx.nd.NDArray) and isinstance(arr, mx.nd.RawFrames) and isinstance(arr, mx.nd.YUVFrames)
    assert not isinstance(arr, mx.nd.NV12Frames) and not issubclass(mx.nd.NV12Frames, mx.nd.YUVFrames)
    like = mx.nd.raw_frames(np.zeros((2, rows, cols, 3), np.uint8), cfg)
    assert arr.shape == like.shape and arr.geometry == like.geometry and arr.scale == like.scale and arr.means == like.means == MEANS
    assert arr.layout == dict(n=2, colour=2, **image.yuv_layout(fmt, rows, cols))              # the default colour mode is bt709
    buf[...] = 0                                      # the payload is a copy: editing the source does not reach it
    assert np.array_equal(arr.yuv, keep.reshape(-1)) and not arr.yuv.flags.writeable
    assert arr._frames is None and arr._host is None  # nothing converted on the host so far
    want = _host(keep, fmt, rows, cols, target, max_size, colour=2)
    assert np.array_equal(arr.asnumpy(), want) and arr.asnumpy().dtype == np.float32
    assert np.array_equal(arr.frames, image.yuv_to_bgr_host(keep, fmt, rows, cols, colour=2)) and not arr.frames.flags.writeable
    # one flat frame, a flat run of frames and a list of frames; another colour mode
    assert np.array_equal(mx.nd.yuv_frames(keep[0], fmt, rows, cols, cfg).asnumpy(), want[:1])
    assert np.array_equal(mx.nd.yuv_frames(keep.reshape(-1), fmt, rows, cols, cfg, colour="bt709").asnumpy(), want)
    assert np.array_equal(mx.nd.yuv_frames([keep[0], keep[1]], fmt, rows, cols, cfg, colour=2).asnumpy(), want)
    assert not np.array_equal(mx.nd.yuv_frames(keep, fmt, rows, cols, cfg, colour="bt601").asnumpy(), want)
    if fmt == "p010":                                 # uint16 words are viewed as bytes
        assert np.array_equal(mx.nd.yuv_frames(keep.view("<u2"), fmt, rows, cols, cfg).asnumpy(), want)
    # a pitched layout: the rows of an n x frame_bytes buffer are the frames
    extra = dict(i420=dict(pitch=cols + 12, pitch_c=cols // 2 + 3), p010=dict(pitch=2 * cols + 6), yuy2=dict(pitch=2 * cols + 7))[fmt]
    fb = image.yuv_layout(fmt, rows, cols, **extra)["frame_bytes"] + 6
    spread, lay = _spread(fmt, keep, rows, cols, 7, frame_bytes=fb, **extra)
    pitched = mx.nd.yuv_frames(spread.reshape(2, fb), fmt, rows, cols, cfg, **extra)
    assert pitched.layout["frame_bytes"] == fb and np.array_equal(pitched.asnumpy(), want)
    with pytest.raises(ValueError, match="h = %d" % (rows + 1) if fmt != "yuy2" else "frame_bytes"):
        mx.nd.yuv_frames(keep, fmt, rows + 1, cols, cfg)
    with pytest.raises(ValueError, match="colour"):
        mx.nd.yuv_frames(keep, fmt, rows, cols, cfg, colour="rec2020")
    with pytest.raises(ValueError, match="format"):
        mx.nd.yuv_frames(keep, "nv21", rows, cols, cfg)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("colour", [0, 3])
def test_bgr_to_yuv_has_the_documented_size_and_is_accepted_back(fmt, colour):
    f = np.random.default_rng(colour).integers(0, 256, (2, 8, 12, 3), dtype=np.uint8)
    b = image.bgr_to_yuv_host(f, fmt, colour)
    assert b.dtype == np.uint8 and b.shape == (2, _tight_bytes(fmt, 8, 12))
    assert image.yuv_to_bgr_host(b, fmt, 8, 12, colour=colour).shape == f.shape
    flat = np.empty((1, 8, 12, 3), np.uint8)
    flat[...] = (40, 120, 200)                        # a frame of one colour comes back within the quantisation of two conversions
    back = image.yuv_to_bgr_host(image.bgr_to_yuv_host(flat, fmt, colour), fmt, 8, 12, colour=colour)
    assert np.abs(back.astype(int) - flat.astype(int)).max() <= 2
    for bad in (f[:, :7], f[:, :, :11]):
        with pytest.raises(ValueError, match="even"):
            image.bgr_to_yuv_host(bad, fmt, colour)


def test_build_batches_yuv_and_the_demo_flags(demo_cfg):
    from accel_amd import demo, mx
    from accel_amd.utils import synth
    cfg = _cfg(demo_cfg, 128, 256, 16)
    frames = synth.make_clip(120, 250, 3)
    raw = demo.build_batches(frames, cfg, raw=True)
    for fmt in FORMATS:
        yuv = demo.build_batches(frames, cfg, raw=True, yuv=fmt, yuv_colour="bt601-full")
        for t in range(3):
            assert isinstance(yuv[t][0], mx.nd.YUVFrames) and yuv[t][0].layout["colour"] == 1 and yuv[t][0].layout["format"] == image.YUV_FORMATS[fmt]
            assert [a.shape for a in yuv[t]] == [a.shape for a in raw[t]]
            assert yuv[t][1] is (yuv[t - 1][0] if t else yuv[0][0])
            assert np.array_equal(yuv[t][0].yuv, image.bgr_to_yuv_host(frames[t], fmt, 1).reshape(-1))
        with pytest.raises(ValueError, match="odd-sized"):
            demo.build_batches(synth.make_clip(121, 250, 1), cfg, raw=True, yuv=fmt)
    with pytest.raises(SystemExit) as e:
        demo.main(["--yuv", "p010", "--yuv-colour", "bt601", "--help"])
    assert e.value.code == 0
    for bad in (["--yuv", "nv21"], ["--yuv", "i420", "--yuv-colour", "bt2020"]):
        with pytest.raises(SystemExit) as e:
            demo.main(bad)
        assert e.value.code != 0
    with pytest.raises(ValueError, match="odd-sized"):
        demo.main(["--version", "18", "--num_ex", "1", "--interval", "2", "--synthetic", "127x256", "--yuv", "yuy2"])
    with pytest.raises(ValueError, match="mutually exclusive"):
        demo.main(["--version", "18", "--num_ex", "1", "--interval", "2", "--synthetic", "128x256", "--yuv", "i420", "--nv12"])
