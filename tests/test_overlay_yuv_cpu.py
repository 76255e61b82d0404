"""The overlay in the frame's own format, host side: utils.image.overlay_yuv_host (the specification of accel_labels_overlay_yuv) against the
scalar restatement of overlay_ref.py on the whole case table, the consequences of the rule, utils.image.palette_ycbcr, the wrong kernels, and the
argument checks that need no GPU.  Every comparison of samples is bit for bit.  (GPU side: test_overlay_yuv_gpu.py.)

The one comparison with a bar is the matrix-sanity check, which holds the (Y, Cb, Cr) table to the colours it stands for: constant-label frames
of constant colour (the 19 Cityscapes colours x a grey ramp, alpha 64, 128 and 256) blended in YUV and converted to BGR, against colour_host on
the BGR conversion of the frame.  MEASURED on the CPU: the largest difference of a channel is, for the 8-bit formats (NV12, I420 and YUY2 alike),
2 levels in bt601, bt601-full and bt709-full and 3 levels in bt709, and 1 level for P010 in all four modes; the bar is that plus one level, the one
extra rounding of the table.  The same palette with R and B swapped misses pure red by far more than that."""
import numpy as np
import pytest

import overlay_ref as ref
from accel_amd.dataset.cityscape import getpallete
from accel_amd.utils import image

MEASURED_8BIT = {"bt601": 2, "bt601-full": 2, "bt709": 3, "bt709-full": 2}       # see the module docstring
MEASURED_P010 = 1
COLOURS = sorted(image.NV12_COLOURS)


def _measured(fmt, colour):
    return MEASURED_P010 if fmt == "p010" else MEASURED_8BIT[colour]


def _host(c, alpha=None, labels=None):
    return image.overlay_yuv_host(c["buf"], c["fmt"], c["h"], c["w"], c["at_source"] if labels is None else labels, c["table"],
                                  c["alpha"] if alpha is None else alpha, **c["kw"])


def _scalar(c, alpha=None, mutant=None):
    return ref.overlay_scalar(c["buf"], c["lay"], c["n"], c["labels"], c["out_h"], c["out_w"], c["table"], c["alpha"] if alpha is None else alpha, mutant)


@pytest.mark.parametrize("name", [c["name"] for c in ref.CASES])
def test_the_vectorised_specification_equals_the_scalar_restatement(name):
    c = ref.make(ref.BY_NAME[name])
    alphas = ref.ALPHAS if c["h"] * c["w"] <= 64 else (c["alpha"], 1)
    for alpha in alphas:
        got, want = _host(c, alpha), _scalar(c, alpha)
        assert got.dtype == np.uint8 and got.shape == c["buf"].shape
        assert np.array_equal(got, want), (name, alpha, int(np.count_nonzero(got != want)))
        mask = ref.sample_mask(c["lay"], c["n"])
        assert np.array_equal(got[~mask], c["buf"][~mask]), "bytes that are not samples changed"
        if c["lay"]["format"] == 1:
            assert not (got.view("<u2")[mask[0::2]] & 63).any(), "the low six bits of a stored P010 word are zero"


def test_the_table_names_every_size_layout_and_geometry():
    """what the GPU file relies on: the table holds what the issue lists"""
    have = {(c["fmt"], c["h"], c["w"]) for c in ref.CASES}
    for fmt in ref.FORMATS:
        for size in [(2, 2), (2, 4), (4, 6), (6, 10), (16, 16), (8, 32)] + ([(1, 2), (3, 6)] if fmt == "yuy2" else []):
            assert (fmt,) + size in have
        kinds = {c["kind"] for c in ref.CASES if c["fmt"] == fmt}
        assert {"tight", "odd", "padded16", "tail"} <= kinds
        geos = {(c["out_h"], c["out_w"]) for c in ref.CASES if c["fmt"] == fmt and (c["h"], c["w"]) == (6, 10)}
        assert {(6, 10), (3, 5), (5, 7), (12, 20)} <= geos
    assert {"pitch_c", "yv12", "interleaved"} <= {c["kind"] for c in ref.CASES if c["fmt"] == "i420"}
    assert "gap" in {c["kind"] for c in ref.CASES if c["fmt"] == "nv12"}
    assert any(c["n"] == 3 and c["kind"] == "tail" for c in ref.CASES) and any(c["hi"] == 256 for c in ref.CASES)
    for c in ref.CASES:       # every map sits in a larger canvas
        assert c["H"] > c["out_h"] and c["W"] > c["out_w"]
    lay = ref.make(ref.BY_NAME[[c["name"] for c in ref.CASES if c["kind"] == "interleaved"][0]])["lay"]
    assert lay["pitch_c"] == lay["pitch"] and lay["v_offset"] == lay["u_offset"] + lay["pitch"] // 2


# ---- consequences of the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in ref.CASES])
def test_alpha_zero_returns_every_sample_unchanged(name):
    c = ref.make(ref.BY_NAME[name])
    got = _host(c, 0)
    want = c["buf"].copy()
    if c["lay"]["format"] == 1:       # a P010 sample is word >> 6: the low six bits of a stored word are zero, every other byte is the input's
        want.view("<u2")[ref.sample_mask(c["lay"], c["n"])[0::2]] &= 0xffc0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", ref.FORMATS)
@pytest.mark.parametrize("alpha", [1, 64, 128, 255, 256])
def test_chroma_of_uniform_blocks_is_the_per_sample_form(fmt, alpha):
    """on a block whose pixels share one label, (a S + (256 - a) 4 C + 512) >> 10 is (a T + (256 - a) C + 128) >> 8: the same integer"""
    h, w, n = 6, 12, 2
    rng = np.random.default_rng(alpha)
    lay = image.overlay_layout(fmt, h, w)
    f = lay["format"]
    buf = rng.integers(0, 256, n * lay["frame_bytes"], dtype=np.uint8)
    blocks = rng.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8)
    labels = np.repeat(np.repeat(blocks, 2, axis=1), 2, axis=2)
    table = image.palette_ycbcr(ref.palette(3), 2, bits=10 if f == 1 else 8)
    got = image.overlay_yuv_host(buf, fmt, h, w, labels, table, alpha)
    T = table.astype(np.int64)
    if f == 1:
        words, out = buf.view("<u2").reshape(n, -1).astype(np.int64) >> 6, got.view("<u2").reshape(n, -1).astype(np.int64) >> 6
        c, o = words[:, h * w:].reshape(n, h // 2, w // 2, 2), out[:, h * w:].reshape(n, h // 2, w // 2, 2)
        per = [blocks, blocks]
    elif f == 2:
        quads, out = buf.reshape(n, h, w // 2, 4).astype(np.int64), got.reshape(n, h, w // 2, 4).astype(np.int64)
        c, o = quads[..., 1::2], out[..., 1::2]
        per = [np.repeat(blocks, 2, axis=1)] * 2
    elif f == 3:
        c = buf.reshape(n, -1)[:, h * w:].reshape(n, h // 2, w // 2, 2).astype(np.int64)
        o = got.reshape(n, -1)[:, h * w:].reshape(n, h // 2, w // 2, 2).astype(np.int64)
        per = [blocks, blocks]
    else:
        planes = lambda a: np.stack([a.reshape(n, -1)[:, h * w:h * w * 5 // 4], a.reshape(n, -1)[:, h * w * 5 // 4:]], axis=-1)
        c, o = planes(buf).reshape(n, h // 2, w // 2, 2).astype(np.int64), planes(got).reshape(n, h // 2, w // 2, 2).astype(np.int64)
        per = [blocks, blocks]
    for ch in (0, 1):
        want = (alpha * T[per[ch], ch + 1] + (256 - alpha) * c[..., ch] + 128) >> 8
        assert np.array_equal(o[..., ch], want), (fmt, alpha, ch)


@pytest.mark.parametrize("alpha", [1, 128, 255, 256])
def test_nv12_and_i420_outputs_are_equal_after_repacking(alpha):
    h, w, n = 6, 10, 2
    rng = np.random.default_rng(alpha)
    nv12 = rng.integers(0, 256, (n, h * w * 3 // 2), dtype=np.uint8)
    uv = nv12[:, h * w:].reshape(n, h // 2, w // 2, 2)
    i420 = np.concatenate([nv12[:, :h * w], uv[..., 0].reshape(n, -1), uv[..., 1].reshape(n, -1)], axis=1)
    labels = rng.integers(0, 19, (n, h, w), dtype=np.uint8)
    table = image.palette_ycbcr(getpallete(256), 0)
    a = image.overlay_yuv_host(nv12, "nv12", h, w, labels, table, alpha)
    b = image.overlay_yuv_host(i420, "i420", h, w, labels, table, alpha)
    assert a.shape == nv12.shape and b.shape == i420.shape
    auv = a[:, h * w:].reshape(n, h // 2, w // 2, 2)
    assert np.array_equal(b, np.concatenate([a[:, :h * w], auv[..., 0].reshape(n, -1), auv[..., 1].reshape(n, -1)], axis=1))
    assert not np.array_equal(a, nv12)


# ---- the palette table -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", COLOURS)
def test_palette_ycbcr_of_black_and_white(colour):
    pal = np.zeros((256, 3), np.uint8)
    pal[1] = 255
    t8, t10 = image.palette_ycbcr(pal, colour), image.palette_ycbcr(pal, colour, bits=10)
    assert t8.dtype == np.uint16 and t8.shape == (256, 3) and t10.dtype == np.uint16 and t10.shape == (256, 3)
    if colour.endswith("full"):
        assert t8[0, 0] == 0 and t8[1, 0] == 255 and t10[0, 0] == 0 and t10[1, 0] == 1023
        assert tuple(t8[0, 1:]) == tuple(t8[1, 1:]) == (128, 128)
    else:
        assert tuple(t8[0]) == (16, 128, 128) and tuple(t8[1]) == (235, 128, 128)
        assert tuple(t10[0]) == (64, 512, 512) and tuple(t10[1]) == (940, 512, 512)
    assert int(t8.max()) <= 255 and int(t10.max()) <= 1023
    with pytest.raises(ValueError, match="bits"):
        image.palette_ycbcr(pal, colour, bits=12)
    with pytest.raises(ValueError, match="256 x 3"):
        image.palette_ycbcr(pal[:19], colour)


def _to_bgr(buf, fmt, h, w, colour):
    if fmt == "nv12":
        return image.nv12_to_bgr_host(buf, h, w, colour=colour)
    return image.yuv_to_bgr_host(buf, fmt, h, w, colour=colour)


def _matrix_error(fmt, colour, palette, classes=range(19)):
    """max |yuv_to_bgr_host(overlay) - colour_host(labels, palette, yuv_to_bgr_host(frame), alpha)| over constant-label frames of constant grey"""
    h, w = 2, 2
    greys = list(range(0, 256, 17))
    classes = list(classes)
    n = len(classes) * len(greys)
    bgr = np.repeat(np.tile(np.array(greys, np.uint8), len(classes)), h * w * 3).reshape(n, h, w, 3)
    labels = np.repeat(np.repeat(np.array(classes, np.uint8), len(greys)), h * w).reshape(n, h, w)
    frames = image.bgr_to_nv12_host(bgr, colour) if fmt == "nv12" else image.bgr_to_yuv_host(bgr, fmt, colour)
    table = image.palette_ycbcr(palette, colour, bits=10 if fmt == "p010" else 8)
    seen = _to_bgr(frames, fmt, h, w, colour)
    worst = 0
    for alpha in (64, 128, 256):
        got = _to_bgr(image.overlay_yuv_host(frames, fmt, h, w, labels, table, alpha), fmt, h, w, colour)
        want = image.colour_host(labels, palette, frames=seen, alpha=alpha, rgb=False)
        worst = max(worst, int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()))
    return worst


@pytest.mark.parametrize("colour", COLOURS)
@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_the_table_stands_for_the_palettes_colours(fmt, colour):
    pal = getpallete(256).reshape(256, 3)
    err = _matrix_error(fmt, colour, pal)
    print("matrix sanity %s %s: max |difference| = %d level(s)" % (fmt, colour, err))
    assert err <= _measured(fmt, colour) + 1
    swapped = np.ascontiguousarray(pal[:, ::-1])
    red = [i for i in range(19) if tuple(pal[i]) == (255, 0, 0)]
    assert red, "the palette has a saturated colour"
    # the table made of the swapped palette, judged against the true one
    h, w, n = 2, 2, 1
    bgr = np.full((n, h, w, 3), 128, np.uint8)
    labels = np.full((n, h, w), red[0], np.uint8)
    frames = image.bgr_to_nv12_host(bgr, colour) if fmt == "nv12" else image.bgr_to_yuv_host(bgr, fmt, colour)
    table = image.palette_ycbcr(swapped, colour, bits=10 if fmt == "p010" else 8)
    got = _to_bgr(image.overlay_yuv_host(frames, fmt, h, w, labels, table, 256), fmt, h, w, colour)
    want = image.colour_host(labels, pal, frames=_to_bgr(frames, fmt, h, w, colour), alpha=256, rgb=False)
    assert int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()) > _measured(fmt, colour) + 1


# ---- the wrong kernels -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_wrong_kernel_differs_on_the_cases_named_for_it(mutant):
    names = ref.MUTANT_CASES[mutant]
    assert names, "no case is named for %s" % mutant
    for name in names:
        c = ref.make(ref.BY_NAME[name])
        want = _host(c)
        assert np.array_equal(_scalar(c), want)
        wrong = _scalar(c, mutant=mutant)
        assert not np.array_equal(wrong, want), "%s equals the rule on %s: the table has a hole" % (mutant, name)


def test_the_two_rounding_kernel_is_the_rule_at_alpha_256():
    c = ref.make(ref.BY_NAME[ref.MUTANT_CASES["two_roundings"][0]])
    assert np.array_equal(_scalar(c, 256, mutant="two_roundings"), _host(c, 256))
    assert {ref.BY_NAME[n]["alpha"] for n in ref.MUTANT_CASES["two_roundings"]} == {128, 255}


def test_an_unclamped_floor_row_is_the_rule():
    """why the row mutant rounds: y * out_h // h never reaches out_h for y < h, so a kernel that merely drops the clamp is the rule"""
    for h in range(1, 40):
        for out_h in range(1, 40):
            assert (h - 1) * out_h // h <= out_h - 1


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------------------
def test_overlay_refuses_frames_that_are_not_yuv(demo_cfg):
    from accel_amd import mx
    from accel_amd.core import results
    raw = mx.nd.raw_frames(np.zeros((4, 6, 3), np.uint8), demo_cfg)
    with pytest.raises(ValueError, match="colour"):
        results.overlay(object(), raw, getpallete(256))
    with pytest.raises(ValueError, match="NV12Frames"):
        results.overlay(object(), dict(out_h=4, out_w=6, h=4, w=6), getpallete(256))


def test_host_argument_checks_of_the_layout():
    buf = np.zeros(6 * 10 * 3 // 2, np.uint8)
    labels = np.zeros((1, 6, 10), np.uint8)
    table = image.palette_ycbcr(getpallete(256), 0)
    good = dict(buf=buf, fmt="nv12", h=6, w=10, labels_at_source=labels, table=table, alpha=128)
    assert image.overlay_yuv_host(**good).shape == buf.shape
    for change, word in ((dict(alpha=257), "alpha"), (dict(alpha=-1), "alpha"), (dict(h=5), "h ="), (dict(w=9), "w ="), (dict(pitch=9), "pitch"),
                         (dict(u_offset=59), "uv_offset"), (dict(frame_bytes=89), "frame_bytes"), (dict(pitch_c=5), "pitch_c"),
                         (dict(v_offset=70), "v_offset"), (dict(labels_at_source=labels[:, :4]), "labels"), (dict(table=table[:19]), "table"),
                         (dict(table=table.astype(np.int64) + 200), "table"), (dict(fmt="rgb"), "format"), (dict(fmt=4), "format")):
        with pytest.raises(ValueError, match=word):
            image.overlay_yuv_host(**dict(good, **change))
    for fmt, change, word in (("i420", dict(pitch_c=4), "pitch_c"), ("p010", dict(pitch=21), "pitch"), ("p010", dict(u_offset=121), "u_offset"),
                              ("yuy2", dict(u_offset=4), "u_offset"), ("i420", dict(v_offset=3), "v_offset")):
        lay = image.overlay_layout(fmt, 6, 10)
        with pytest.raises(ValueError, match=word):
            image.overlay_yuv_host(np.zeros(lay["frame_bytes"], np.uint8), fmt, 6, 10, labels, image.palette_ycbcr(getpallete(256), 0), 128, **change)
    assert image.overlay_format("NV12") == 3 and image.overlay_format(3) == 3 and image.overlay_format("yuy2") == 2
    assert image.overlay_layout(3, 6, 10, uv_offset=64)["u_offset"] == 64
