"""Interpolated chroma siting, host side: utils/image.py's chroma_upsample and the siting keyword of nv12_to_bgr_host / yuv_to_bgr_host are held to
a scalar-loop restatement of the table (siting_ref.py); the sitings are pinned by where a linear chroma ramp comes out, independently of any
implementation; the cases of the GPU file tell the specification from a matrix of wrong kernels; a round trip through the fabricators orders the
sitings; and the Python surface carries the siting from the demo's flag to the C ABI.  (GPU side: test_chroma_siting_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import siting_ref as ref
from accel_amd.utils import image
from test_frames_yuv_cpu import MEANS, _i420_of_nv12

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("accel_frame_yuv_sited", "accel_yuv_to_bgr_sited", "accel_model_write_yuv_sited", "accel_model_commit_yuv_sited")
ALL = ("replicate",) + ref.SITINGS


# ---- names and numbers ---------------------------------------------------------------------------------------------------------------------------
def test_sitings_are_named_and_numbered():
    assert image.CHROMA_SITINGS == {"replicate": 0, "left": 1, "centre": 2, "topleft": 3}
    for name, number in image.CHROMA_SITINGS.items():
        assert image.chroma_siting(name) == number and image.chroma_siting(number) == number and image.chroma_siting(np.int64(number)) == number
    for bad in ("center", "Left", "", -1, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="siting"):
            image.chroma_siting(bad)
    for fn in (lambda s: image.chroma_upsample(np.zeros((1, 1), np.uint8), 2, 2, s),
               lambda s: image.nv12_to_bgr_host(np.zeros(6, np.uint8), 2, 2, siting=s),
               lambda s: image.yuv_to_bgr_host(np.zeros(6, np.uint8), "i420", 2, 2, siting=s),
               lambda s: image.bgr_to_nv12_host(np.zeros((2, 2, 3), np.uint8), siting=s),
               lambda s: image.bgr_to_yuv_host(np.zeros((2, 2, 3), np.uint8), "yuy2", siting=s)):
        with pytest.raises(ValueError, match="siting"):
            fn("bottom")
    with pytest.raises(ValueError, match="replicate"):       # samples are made WITH a siting; replication is a way of reading them
        image.bgr_to_nv12_host(np.zeros((2, 2, 3), np.uint8), siting="replicate")


# ---- the independent restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("siting", ALL)
@pytest.mark.parametrize("ch,cw,top", [(1, 1, 256), (1, 2, 256), (2, 1, 256), (3, 5, 256), (6, 8, 1024), (7, 9, 1024)])
def test_chroma_upsample_equals_the_scalar_table(ch, cw, top, siting):
    plane = np.random.default_rng(ch * 100 + cw).integers(0, top, (ch, cw))
    for vertical in (True, False):
        h, w = (2 * ch if vertical else ch), 2 * cw
        got = image.chroma_upsample(plane.astype(np.uint16), h, w, siting, vertical=vertical)
        assert got.shape == (h, w) and got.dtype == np.int64
        assert np.array_equal(got, ref.upsample_scalar(plane, h, w, siting, vertical)), (siting, vertical)
        assert got.min() >= plane.min() and got.max() <= plane.max()
        # by number, and with leading axes
        both = image.chroma_upsample(np.stack([plane, plane[::-1]]), h, w, image.CHROMA_SITINGS[siting], vertical=vertical)
        assert np.array_equal(both[0], got) and np.array_equal(both[1], ref.upsample_scalar(plane[::-1], h, w, siting, vertical))
    with pytest.raises(ValueError, match="does not belong"):
        image.chroma_upsample(plane, 2 * ch, 2 * cw + 2, siting)
    with pytest.raises(ValueError, match="integer"):
        image.chroma_upsample(plane.astype(np.float64), 2 * ch, 2 * cw, siting)


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "-".join(map(str, c)))
def test_host_conversion_equals_the_scalar_restatement_on_every_case(case):
    """all four formats, layouts with pitches, gaps, YV12 order and interleaved chroma rows, 1 x 1 chroma planes: every sample from its own address"""
    buf, n, lay = ref.make(case)
    for siting in ALL:
        for colour in ((0, 3) if siting == "left" else (2,)):
            want = ref.to_bgr(buf, n, lay, colour, siting)
            got = ref.host(buf, lay, colour, siting)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (case, siting, colour)
            assert np.array_equal(ref.host(buf, lay, colour, image.CHROMA_SITINGS[siting]), want)
    if case.content.startswith("impulse"):       # the impulse is seen: siting changes the picture
        assert len({ref.expected(case, 2, s).tobytes() for s in ALL}) == (3 if case.fmt == "yuy2" else 4)


def test_overlapping_planes_are_read_sample_by_sample():
    """I420 whose Cr plane starts inside the Cb plane: every tap comes from its own byte address"""
    h, w = 8, 12
    lay = dict(format=0, h=h, w=w, pitch=w, pitch_c=w // 2, u_offset=h * w, v_offset=h * w + 7)
    lay["frame_bytes"] = ref.extent(lay) + 2
    buf = np.random.default_rng(3).integers(0, 256, lay["frame_bytes"] + ref.extent(lay), dtype=np.uint8)
    for siting in ALL:
        assert np.array_equal(ref.host(buf, lay, 1, siting), ref.to_bgr(buf, 2, lay, 1, siting)), siting


# ---- the sitings, pinned independently of any implementation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("siting", ref.SITINGS)
def test_a_chroma_ramp_comes_out_where_the_siting_puts_it(siting):
    """sample (k, j) = a + 8k + 8j lies on luma (2k + x0, 2j + y0): the interpolated plane is a + 4 (x - x0) + 4 (y - y0) at every interior pixel,
    and the extreme sample at the edges where the ramp would leave the plane"""
    h, w, a = 12, 20, 16
    x0, y0 = ref.POSITION[siting]
    k, j = np.meshgrid(np.arange(w // 2), np.arange(h // 2))
    plane = a + 8 * k + 8 * j
    got = image.chroma_upsample(plane, h, w, siting)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    line = a + 4 * (x - x0) + 4 * (y - y0)
    assert np.array_equal(got[2:-2, 2:-2], line[2:-2, 2:-2].astype(np.int64)) and np.all(line[2:-2, 2:-2] % 1 == 0)
    # the whole plane: the ramp with its coordinates clamped to the span of the samples, rounded half up once
    cx = np.clip(x, x0, 2 * (w // 2 - 1) + x0)
    cy = np.clip(y, y0, 2 * (h // 2 - 1) + y0)
    assert np.array_equal(got, np.floor(a + 4 * (cx - x0) + 4 * (cy - y0) + 0.5).astype(np.int64))
    assert got[0, 0] == plane[0, 0] and got[-1, -1] == plane[-1, -1]
    # YUY2: no vertical step, the horizontal rule alone
    wide = a + 8 * k[:1].repeat(h, axis=0) + 3 * np.arange(h)[:, None]
    got = image.chroma_upsample(wide, h, w, siting, vertical=False)
    assert np.array_equal(got[:, 2:-2], (a + 4 * (x - x0) + 3 * y)[:, 2:-2].astype(np.int64))


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_constant_chroma_gives_the_replicated_result(fmt):
    h, w = 6, 10
    ch, cw = (h if fmt == "yuy2" else h // 2), w // 2
    top = 1024 if fmt == "p010" else 256
    rng = np.random.default_rng(5)
    for cbv, crv in ((0, top - 1), (top - 1, 0), (top // 2 + 3, top // 3)):
        planes = [(rng.integers(0, top, (h, w)), np.full((ch, cw), cbv), np.full((ch, cw), crv))]
        for name in ("aligned", "odd"):
            lay = ref.layout(fmt, h, w, name)
            buf = ref.place(planes, lay, 6)
            for colour in range(4):
                want = ref.host(buf, lay, colour, "replicate")
                for siting in ref.SITINGS:
                    assert np.array_equal(ref.host(buf, lay, colour, siting), want), (fmt, name, colour, siting)


def _replicated(buf, n, lay, colour):
    """the rule of the parent commit, restated: pixel (x, y) takes the chroma sample (x >> 1, y >> 1) (YUY2: (x >> 1, y))"""
    f, h, w = lay["format"], lay["h"], lay["w"]
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        Y, cb, cr = ref.samples(buf, i, lay)
        rows = np.arange(h) if f == 2 else np.arange(h) >> 1
        up = lambda p: p[rows[:, None], (np.arange(w) >> 1)[None, :]]
        out[i] = np.stack((image.yuv10_to_bgr if f == 1 else image.yuv_to_bgr)(Y, up(cb), up(cr), colour), axis=-1)
    return out


@pytest.mark.parametrize("case", [c for c in ref.CASES if c.content == "random" and (c.h, c.w) in ((2, 2), (6, 10), (16, 18), (3, 6))],
                         ids=lambda c: "-".join(map(str, c)))
def test_the_default_is_the_replicated_rule(case):
    buf, n, lay = ref.make(case)
    want = _replicated(buf, n, lay, 1)
    kw = ref.keywords(lay)
    if case.fmt == "nv12":
        whole = np.zeros(n * lay["frame_bytes"], np.uint8)
        whole[:buf.size] = buf
        assert np.array_equal(image.nv12_to_bgr_host(whole, case.h, case.w, colour=1, **kw), want)
        assert np.array_equal(image.nv12_to_bgr_host(whole, case.h, case.w, colour=1, siting=0, **kw), want)
    else:
        assert np.array_equal(image.yuv_to_bgr_host(buf, case.fmt, case.h, case.w, colour=1, **kw), want)
        assert np.array_equal(image.yuv_to_bgr_host(buf, case.fmt, case.h, case.w, colour=1, siting="replicate", **kw), want)


# ---- the cases of the GPU file can tell a wrong kernel from a right one -------------------------------------------------------------------------
def test_the_case_table_covers_what_the_gpu_file_promises():
    for fmt in ref.FORMATS:
        mine = [c for c in ref.CASES if c.fmt == fmt]
        sizes = {(c.h, c.w) for c in mine}
        assert {(2, 2), (2, 4), (4, 2), (6, 10), (12, 16), (16, 18)} <= sizes
        assert ({(1, 6), (3, 6)} <= sizes) == (fmt == "yuy2")
        assert {c.layout for c in mine} >= {"aligned", "odd"}
        assert {c.content for c in mine} == {"random"} | {"impulse-" + p for p in ref.IMPULSES}
        for c in mine:
            buf, n, lay = ref.make(c)
            assert n == (3 if c.content == "random" else 1) and buf.size == (n - 1) * lay["frame_bytes"] + ref.extent(lay)
            assert ref.expected(c, 2, "left").shape == (n, c.h, c.w, 3)       # the specification takes every one of them
            if c.layout == "aligned":       # the wide loads, in every frame of the batch
                assert lay["pitch"] % 8 == 0 and lay["frame_bytes"] % 8 == 0 and lay["u_offset"] % 8 == 0
            if c.layout == "odd":           # sample by sample: no row starts where a wide load could (P010's words stay 2-byte aligned)
                assert (lay["pitch"] % 2 == 1 and lay["frame_bytes"] % 2 == 1) if fmt != "p010" else (lay["pitch"] % 8 != 0 and lay["pitch"] % 2 == 0)
    assert {c.layout for c in ref.CASES if c.fmt == "i420"} >= {"yv12", "interleaved"}


@pytest.mark.parametrize("name", sorted(ref.MUTANTS))
def test_the_cases_kill_the_wrong_kernel(name):
    """every wrong kernel differs from the specification on at least one case of every format it applies to"""
    rule, formats, sitings = ref.MUTANTS[name]
    for fmt in formats:
        killed = None
        # (the larger random cases first: most mutants die there at once)
        for case in sorted((c for c in ref.CASES if c.fmt == fmt), key=lambda c: (c.content != "random", -c.h * c.w)):
            buf, n, lay = ref.make(case)
            for siting in sitings:
                if not np.array_equal(ref.to_bgr(buf, n, lay, 2, siting, rule), ref.expected(case, 2, siting)):
                    killed = (case, siting)
                    break
            if killed:
                break
        assert killed, "no case of %s tells '%s' from the specification" % (fmt, name)


def test_the_right_rule_is_not_killed():
    for case in ref.CASES[::7]:
        buf, n, lay = ref.make(case)
        for siting in ref.SITINGS:
            assert np.array_equal(ref.to_bgr(buf, n, lay, 2, siting, ref.RIGHT), ref.expected(case, 2, siting))


def test_nv12_and_i420_of_one_picture_agree_and_p010_need_not():
    h, w = 12, 16
    nv = np.random.default_rng(8).integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    for siting in ALL:
        for colour in range(4):
            assert np.array_equal(image.yuv_to_bgr_host(_i420_of_nv12(nv, h, w), "i420", h, w, colour=colour, siting=siting),
                                  image.nv12_to_bgr_host(nv, h, w, colour=colour, siting=siting))


# ---- the fabricators and the round trip --------------------------------------------------------------------------------------------------------
def _ramp(h, w):
    """a BGR picture whose colour is a ramp of 1.5 to 3 levels per pixel: half a chroma sample is worth more than the rounding noise"""
    y, x = np.mgrid[:h, :w]
    return np.stack([np.clip(20 + 2.2 * x, 0, 255), np.clip(230 - 1.7 * y - 0.5 * x, 0, 255), np.clip(30 + 2.5 * y, 0, 255)], axis=-1).astype(np.uint8)


def test_fabricators_default_to_the_block_mean():
    im = np.random.default_rng(2).integers(0, 256, (2, 8, 12, 3), dtype=np.uint8)
    assert np.array_equal(image.bgr_to_nv12_host(im, 2), image.bgr_to_nv12_host(im, 2, siting="centre"))
    # the block mean, restated: chroma of the mean colour of each 2 x 2 block (the forward matrix is linear)
    kr, kg, kb, yoff, ky, s = image._nv12_standard(2)
    mean = im.astype(np.float64).reshape(2, 4, 2, 6, 2, 3).mean(axis=(2, 4))
    y = kr * mean[..., 2] + kg * mean[..., 1] + kb * mean[..., 0]
    cb = np.clip(np.rint(128.0 + (mean[..., 0] - y) / (2.0 * (1.0 - kb)) / s), 0, 255)
    got = image.bgr_to_nv12_host(im, 2)[:, 8 * 12:].reshape(2, 4, 6, 2)[..., 0]
    assert np.abs(got.astype(np.float64) - cb).max() <= 1       # (the order of the float operations may move a tie)
    for fmt in ("i420", "p010", "yuy2"):
        assert np.array_equal(image.bgr_to_yuv_host(im, fmt, 1), image.bgr_to_yuv_host(im, fmt, 1, siting=2))
        assert np.array_equal(image.bgr_to_yuv_host(im, "yuy2", 1, siting="left"), image.bgr_to_yuv_host(im, "yuy2", 1, siting="topleft"))
        for siting in ("left", "topleft"):
            out = image.bgr_to_yuv_host(im, fmt, 1, siting=siting)
            assert out.shape == image.bgr_to_yuv_host(im, fmt, 1).shape and not np.array_equal(out, image.bgr_to_yuv_host(im, fmt, 1))
    # the luma does not know the siting
    assert np.array_equal(image.bgr_to_nv12_host(im, 2, siting="left")[:, :96], image.bgr_to_nv12_host(im, 2)[:, :96])
    # a flat colour has one chroma whatever the siting, the replicated edge included
    flat = np.full((4, 6, 3), (40, 90, 200), np.uint8)
    for siting in ref.SITINGS:
        assert np.array_equal(image.bgr_to_nv12_host(flat, 0, siting=siting), image.bgr_to_nv12_host(flat, 0))


@pytest.mark.parametrize("fmt", ref.FORMATS)
@pytest.mark.parametrize("made", ref.SITINGS)
def test_round_trip_prefers_the_siting_the_frames_were_made_with(fmt, made):
    """an ordering, no number: the matching interpolation reconstructs a colour ramp strictly better than every other siting and than replication"""
    if fmt == "yuy2" and made == "topleft":
        made = "left"              # one rule for YUY2
    h, w = 64, 96
    im = _ramp(h, w)
    error = {}
    for siting in ALL:
        if fmt == "nv12":
            back = image.nv12_to_bgr_host(image.bgr_to_nv12_host(im, 2, siting=made), h, w, colour=2, siting=siting)
        else:
            back = image.yuv_to_bgr_host(image.bgr_to_yuv_host(im, fmt, 2, siting=made), fmt, h, w, colour=2, siting=siting)
        error[siting] = float(np.abs(back[0, 4:-4, 4:-4].astype(np.int64) - im[4:-4, 4:-4]).mean())
    print(fmt, made, error)
    same = ("left", "topleft") if fmt == "yuy2" and made == "left" else (made,)
    for siting in ALL:
        if siting not in same:
            assert error[made] < error[siting], (fmt, made, error)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def _cfg(demo_cfg, target, max_size, stride):
    demo_cfg.SCALES[0] = (target, max_size)
    demo_cfg.network.IMAGE_STRIDE = stride
    return demo_cfg


def _tensor(bgr, target, max_size, stride=16):
    return np.concatenate([image.transform(image.resize(f, target, max_size, stride=stride)[0], MEANS) for f in bgr]).astype(np.float32)


@pytest.mark.parametrize("siting", ALL)
def test_arrays_keep_the_siting_and_stand_for_the_host_tensor(demo_cfg, siting):
    from accel_amd import mx
    rows, cols = 44, 82
    cfg = _cfg(demo_cfg, 48, 96, 16)
    number = image.CHROMA_SITINGS[siting]
    nv = np.random.default_rng(4).integers(0, 256, (2, rows * cols * 3 // 2), dtype=np.uint8)
    arr = mx.nd.nv12_frames(nv, rows, cols, cfg, colour="bt709", siting=siting)
    assert arr.siting == number and isinstance(arr.siting, int)
    assert arr.layout == dict(n=2, colour=2, **image.nv12_layout(rows, cols, frame_bytes=nv.shape[1]))       # no new key
    want = image.nv12_to_bgr_host(nv, rows, cols, colour=2, siting=siting)
    assert np.array_equal(arr.frames, want) and np.array_equal(arr.asnumpy(), _tensor(want, 48, 96))
    assert mx.nd.nv12_frames(nv, rows, cols, cfg, siting=number).siting == number
    assert mx.nd.nv12_frames(nv, rows, cols, cfg).siting == 0
    for fmt in ("i420", "p010", "yuy2"):
        buf = np.random.default_rng(5).integers(0, 256, (2, rows * cols * {"i420": 3, "p010": 6, "yuy2": 4}[fmt] // 2), dtype=np.uint8)
        arr = mx.nd.yuv_frames(buf, fmt, rows, cols, cfg, siting=siting)
        assert arr.siting == number and arr.layout == dict(n=2, colour=2, **image.yuv_layout(fmt, rows, cols))
        want = image.yuv_to_bgr_host(buf, fmt, rows, cols, colour=2, siting=siting)
        assert np.array_equal(arr.frames, want) and np.array_equal(arr.asnumpy(), _tensor(want, 48, 96))
        assert mx.nd.yuv_frames(buf, fmt, rows, cols, cfg).siting == 0
    for bad in ("center", 4):
        with pytest.raises(ValueError, match="siting"):
            mx.nd.nv12_frames(nv, rows, cols, cfg, siting=bad)
        with pytest.raises(ValueError, match="siting"):
            mx.nd.yuv_frames(nv, "i420", rows, cols, cfg, siting=bad)


def test_build_batches_and_the_demo_flag(demo_cfg):
    from accel_amd import demo, mx
    from accel_amd.utils import synth
    cfg = _cfg(demo_cfg, 128, 256, 16)
    frames = synth.make_clip(120, 250, 2)
    for siting in ALL:
        made = "centre" if siting == "replicate" else siting
        nv = demo.build_batches(frames, cfg, raw=True, nv12="bt709", siting=siting)
        yuv = demo.build_batches(frames, cfg, raw=True, yuv="p010", yuv_colour="bt601", siting=siting)
        for t in range(2):
            assert isinstance(nv[t][0], mx.nd.NV12Frames) and nv[t][0].siting == image.CHROMA_SITINGS[siting]
            assert np.array_equal(nv[t][0].nv12, image.bgr_to_nv12_host(frames[t], "bt709", siting=made))
            assert isinstance(yuv[t][0], mx.nd.YUVFrames) and yuv[t][0].siting == image.CHROMA_SITINGS[siting]
            assert np.array_equal(yuv[t][0].yuv, image.bgr_to_yuv_host(frames[t], "p010", "bt601", siting=made).reshape(-1))
    # the default: what build_batches made before
    assert np.array_equal(demo.build_batches(frames, cfg, raw=True, nv12="bt601")[0][0].nv12, image.bgr_to_nv12_host(frames[0], "bt601"))
    assert demo.build_batches(frames, cfg, raw=True, yuv="i420")[1][0].siting == 0
    with pytest.raises(ValueError, match="siting"):
        demo.build_batches(frames, cfg, raw=True, nv12="bt601", siting="bottom")
    with pytest.raises(SystemExit) as e:
        demo.main(["--nv12", "bt709", "--chroma-siting", "left", "--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit) as e:
        demo.main(["--nv12", "--chroma-siting", "bottom"])
    assert e.value.code != 0
    with pytest.raises(ValueError, match="--chroma-siting needs --nv12 or --yuv"):
        demo.main(["--version", "18", "--num_ex", "1", "--interval", "2", "--synthetic", "128x256", "--chroma-siting", "centre"])
    with pytest.raises(ValueError, match="odd-sized"):       # the flag is accepted with --yuv: the next check is the frame size
        demo.main(["--version", "18", "--num_ex", "1", "--interval", "2", "--synthetic", "127x256", "--yuv", "yuy2", "--chroma-siting", "topleft"])


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_sited_entry_points():
    from accel_amd import runtime
    hdr = open(os.path.join(ROOT, "include", "accel_hip.h")).read()
    declared = set(re.findall(r"\b(accel_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, "include/accel_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libaccel_hip.so does not export %s" % name
        proto = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        args = [a.strip() for a in proto.replace("\n", " ").split(",")]
        assert "int siting" in args, name
        tail = [a for a in args if a in ("int on_device", "int src_on_device")]
        assert args[-1] == (tail[0] if tail else "int siting") and args[-1 - len(tail)] == "int siting", (name, args)   # before on_device
    runtime.lib()
    assert set(ENTRY_POINTS) <= set(runtime.EXPORTS)
    for name in ENTRY_POINTS:       # the twin's signature plus one int
        assert len(runtime.EXPORTS[name]) == len(runtime.EXPORTS[name[:-len("_sited")]]) + 1
    assert ctypes.sizeof(runtime.YUVLayout) == 4 * ctypes.sizeof(ctypes.c_int) + 5 * ctypes.sizeof(ctypes.c_size_t)      # the layout keeps its size
    for text in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        doc = open(os.path.join(ROOT, text)).read()
        flat = " ".join(doc.split())
        assert "chroma siting is not offered" not in flat and "chroma siting (left or centre) is not offered" not in flat, text
        assert "--chroma-siting" in flat or text == "DESIGN.md", text
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, "INTEGRATION.md does not describe %s" % name
