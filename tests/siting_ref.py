"""Interpolated chroma siting, restated independently of accel_amd/utils/image.py, and the inputs the GPU file runs.

The rule (include/accel_hip.h): chroma planes of cw = w/2 columns and ch = h/2 rows (YUY2: ch = h, no vertical step).  For luma pixel (x, y),
k = x >> 1 and j = y >> 1, each axis takes two neighbouring samples with weights that sum to 4 -- co-sited: even (k: 4), odd (k: 2, k+1: 2);
centred: even (k-1: 1, k: 3), odd (k: 3, k+1: 1) -- indices clamped, C = (sum wy wx c + 8) >> 4.  left = (co-sited, centred), centre = (centred,
centred), topleft = (co-sited, co-sited) as (horizontal, vertical).

`upsample_scalar` is that table as a scalar loop.  `to_bgr` is a whole converter built on it -- every sample read from its own byte address by
a scalar loop -- with a `Rule` whose knobs turn it into the usual WRONG kernels (MUTANTS); test_chroma_siting_cpu.py asserts that CASES, the
inputs of test_chroma_siting_gpu.py, tell every one of them from the specification."""
import collections

import numpy as np

from accel_amd.utils import image

FORMATS = ("i420", "p010", "yuy2", "nv12")
NUMBER = {"i420": 0, "p010": 1, "yuy2": 2, "nv12": 3}
SITINGS = ("left", "centre", "topleft")
MODES = {"left": ("co", "ce"), "centre": ("ce", "ce"), "topleft": ("co", "co")}      # (horizontal, vertical)
POSITION = {"left": (0.0, 0.5), "centre": (0.5, 0.5), "topleft": (0.0, 0.0)}         # (x0, y0): where sample 0 lies on the luma grid

Rule = collections.namedtuple("Rule", "parity_swapped axes_swapped siting_map edge two_roundings bias cr_from_cb nv12_stride p010_late")
RIGHT = Rule(parity_swapped=False, axes_swapped=False, siting_map={}, edge="clamp", two_roundings=False, bias=8, cr_from_cb=False, nv12_stride=2,
             p010_late=False)

# name -> (rule, the formats it applies to, the sitings it applies to)
MUTANTS = {
    "even/odd weights swapped": (RIGHT._replace(parity_swapped=True), FORMATS, SITINGS),
    "horizontal and vertical modes swapped": (RIGHT._replace(axes_swapped=True), FORMATS, ("left",)),
    "left computed as centre": (RIGHT._replace(siting_map={"left": "centre"}), FORMATS, ("left",)),
    "centre computed as left": (RIGHT._replace(siting_map={"centre": "left"}), FORMATS, ("centre",)),
    "centre computed as topleft": (RIGHT._replace(siting_map={"centre": "topleft"}), FORMATS, ("centre",)),
    "topleft computed as centre": (RIGHT._replace(siting_map={"topleft": "centre"}), FORMATS, ("topleft",)),
    "left computed as topleft": (RIGHT._replace(siting_map={"left": "topleft"}), ("i420", "p010", "nv12"), ("left",)),      # one rule for YUY2
    "topleft computed as left": (RIGHT._replace(siting_map={"topleft": "left"}), ("i420", "p010", "nv12"), ("topleft",)),
    "wrap instead of clamp": (RIGHT._replace(edge="wrap"), FORMATS, SITINGS),
    "zero instead of clamp": (RIGHT._replace(edge="zero"), FORMATS, SITINGS),
    "a rounding per axis": (RIGHT._replace(two_roundings=True), ("i420", "p010", "nv12"), SITINGS),                        # YUY2 has one axis
    "bias 7": (RIGHT._replace(bias=7), FORMATS, SITINGS),
    "bias 0": (RIGHT._replace(bias=0), FORMATS, SITINGS),
    "Cb taps used for Cr": (RIGHT._replace(cr_from_cb=True), FORMATS, SITINGS),
    "NV12 chroma read at stride 1": (RIGHT._replace(nv12_stride=1), ("nv12",), SITINGS),
    "P010 interpolated after conversion to 8 bits": (RIGHT._replace(p010_late=True), ("p010",), SITINGS),
}


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
def taps(x, mode, swapped=False):
    """[(index, weight)] of luma coordinate x on one axis, indices not clamped"""
    if mode == "none":
        return [(x, 4)]
    k, odd = x >> 1, (x % 2 == 1) != swapped
    if mode == "co":
        return [(k, 2), (k + 1, 2)] if odd else [(k, 4)]
    return [(k, 3), (k + 1, 1)] if odd else [(k - 1, 1), (k, 3)]


def _edge(i, count, edge):
    """(index to read, whether the sample counts) under an edge rule"""
    if 0 <= i < count:
        return i, True
    if edge == "clamp":
        return min(max(i, 0), count - 1), True
    if edge == "wrap":
        return i % count, True
    return 0, False


def upsample_scalar(plane, h, w, siting, vertical=True, rule=RIGHT):
    """a ch x cw plane of integer samples -> h x w int64: the table, pixel by pixel; siting "replicate": sample (x >> 1, y >> 1)"""
    p = np.asarray(plane).astype(np.int64)
    ch, cw = p.shape
    assert cw == w // 2 and ch == (h // 2 if vertical else h)
    out = np.zeros((h, w), np.int64)
    if siting == "replicate":
        for y in range(h):
            for x in range(w):
                out[y, x] = p[y >> 1 if vertical else y, x >> 1]
        return out
    hm, vm = MODES[rule.siting_map.get(siting, siting)]
    if rule.axes_swapped:
        hm, vm = vm, hm
    if not vertical:
        vm = "none"
    for y in range(h):
        for x in range(w):
            total = 0
            for j, wy in taps(y, vm, rule.parity_swapped):
                j, row_counts = _edge(j, ch, rule.edge)
                line = 0
                for k, wx in taps(x, hm, rule.parity_swapped):
                    k, counts = _edge(k, cw, rule.edge)
                    line += wx * int(p[j, k]) if counts and row_counts else 0
                total += wy * ((line + 2) >> 2 if rule.two_roundings else line)
            out[y, x] = (total + 2) >> 2 if rule.two_roundings else (total + rule.bias) >> 4
    return out


# ---- frames: samples at their byte addresses -----------------------------------------------------------------------------------------------------
def _up(v, k):
    return -(-v // k) * k


def extent(lay):
    """one past the last byte of a frame (format 3: the last chroma row ends after w bytes)"""
    if lay["format"] == 3:
        return lay["u_offset"] + (lay["h"] // 2 - 1) * lay["pitch"] + lay["w"]
    return image.yuv_extent(lay)


def layout(fmt, h, w, name):
    """the layout dict (the fields of accel_yuv_layout) of a named layout.  aligned: every row of every frame starts on 8 bytes -- the wide
    loads; odd: odd pitches, odd plane offsets and an odd frame_bytes (P010: all even, none a multiple of 8) -- sample by sample, and frames
    at odd addresses; yv12 / interleaved: I420 with Cr first / with a Cb and a Cr row in every row of the chroma area"""
    f = NUMBER[fmt]
    lay = dict(format=f, h=h, w=w, pitch_c=0, u_offset=0, v_offset=0)
    cw = w // 2
    if name == "aligned":
        lay["pitch"] = _up(w + 1, 8) if f in (0, 3) else _up(2 * w + 2, 8)
        if f == 0:
            lay.update(pitch_c=lay["pitch"] // 2, u_offset=h * lay["pitch"], v_offset=h * lay["pitch"] + (h // 2) * (lay["pitch"] // 2))
        elif f != 2:
            lay["u_offset"] = h * lay["pitch"]
        lay["frame_bytes"] = _up(extent(lay), 8) + (8 if f != 2 else 0)
    elif name == "odd":
        if f == 1:
            lay["pitch"] = 2 * w + 2
            lay["u_offset"] = h * lay["pitch"] + 2
            lay["frame_bytes"] = extent(lay) + 6
        else:
            lay["pitch"] = (w + 3 if f in (0, 3) else 2 * w + 7) | 1
            if f == 0:
                lay["pitch_c"] = (cw + 2) | 1
                lay["u_offset"] = h * lay["pitch"] + 1
                lay["v_offset"] = lay["u_offset"] + (h // 2) * lay["pitch_c"] + 3
            elif f == 3:
                lay["u_offset"] = h * lay["pitch"] + 1
            lay["frame_bytes"] = (extent(lay) + 4) | 1
            if f == 3:                                   # (the NV12 route counts a whole pitch for the last chroma row)
                lay["frame_bytes"] = (lay["u_offset"] + (h // 2) * lay["pitch"] + 4) | 1
    elif name == "yv12" and f == 0:
        lay.update(pitch=w, pitch_c=cw, v_offset=h * w, u_offset=h * w + (h // 2) * cw)
        lay["frame_bytes"] = extent(lay)
    elif name == "interleaved" and f == 0:
        pitch = _up(w + 9, 4)
        lay.update(pitch=pitch, pitch_c=pitch, u_offset=h * pitch, v_offset=h * pitch + pitch // 2)
        lay["frame_bytes"] = extent(lay) + 3
    else:
        raise KeyError((fmt, name))
    return lay


def keywords(lay):
    """the layout as the keywords of image.yuv_to_bgr_host / Context.frame_yuv (formats 0 .. 2) or of nv12_to_bgr_host / frame_nv12 (3)"""
    if lay["format"] == 3:
        return dict(pitch=lay["pitch"], uv_offset=lay["u_offset"], frame_bytes=lay["frame_bytes"])
    return {k: lay[k] for k in ("pitch", "pitch_c", "u_offset", "v_offset", "frame_bytes") if lay[k] or k in ("pitch", "frame_bytes")}


def _addresses(lay, stride=2):
    """the byte address of (luma (x, y), Cb (col, row), Cr (col, row)) within a frame, as three functions"""
    f, pitch = lay["format"], lay["pitch"]
    if f == 0:
        return (lambda x, y: y * pitch + x, lambda c, r: lay["u_offset"] + r * lay["pitch_c"] + c, lambda c, r: lay["v_offset"] + r * lay["pitch_c"] + c)
    if f == 1:
        return (lambda x, y: y * pitch + 2 * x, lambda c, r: lay["u_offset"] + r * pitch + 4 * c, lambda c, r: lay["u_offset"] + r * pitch + 4 * c + 2)
    if f == 2:
        return (lambda x, y: y * pitch + 2 * x, lambda c, r: r * pitch + 4 * c + 1, lambda c, r: r * pitch + 4 * c + 3)
    return (lambda x, y: y * pitch + x, lambda c, r: lay["u_offset"] + r * pitch + stride * c, lambda c, r: lay["u_offset"] + r * pitch + stride * c + 1)


def samples(buf, i, lay, stride=2):
    """(Y h x w, Cb ch x cw, Cr ch x cw) int64 samples of frame i of flat bytes `buf`, each read from its own address; P010: word >> 6"""
    f, h, w = lay["format"], lay["h"], lay["w"]
    ch, cw = (h if f == 2 else h // 2), w // 2
    base = i * lay["frame_bytes"]
    get = (lambda a: (int(buf[base + a]) | int(buf[base + a + 1]) << 8) >> 6) if f == 1 else (lambda a: int(buf[base + a]))
    ya, ua, va = _addresses(lay, stride)
    Y = np.array([[get(ya(x, y)) for x in range(w)] for y in range(h)], np.int64)
    cb = np.array([[get(ua(c, r)) for c in range(cw)] for r in range(ch)], np.int64)
    cr = np.array([[get(va(c, r)) for c in range(cw)] for r in range(ch)], np.int64)
    return Y, cb, cr


def place(planes, lay, seed):
    """flat bytes of the frames [(Y, Cb, Cr)] laid out as `lay` says: NON-ZERO noise in every gap, and in the low six bits of every P010 word;
    the buffer ends with the last byte of its last frame"""
    f, h, w, fb = lay["format"], lay["h"], lay["w"], lay["frame_bytes"]
    ch, cw = (h if f == 2 else h // 2), w // 2
    rng = np.random.default_rng(seed)
    out = rng.integers(1, 256, (len(planes) - 1) * fb + extent(lay), dtype=np.uint8)
    ya, ua, va = _addresses(lay)
    for i, (Y, cb, cr) in enumerate(planes):
        def put(a, v):
            if f == 1:
                word = (int(v) << 6) | int(rng.integers(0, 64))
                out[i * fb + a], out[i * fb + a + 1] = word & 255, word >> 8
            else:
                out[i * fb + a] = v
        for y in range(h):
            for x in range(w):
                put(ya(x, y), Y[y, x])
        for r in range(ch):
            for c in range(cw):
                put(ua(c, r), cb[r, c])
                put(va(c, r), cr[r, c])
    return out


def to_bgr(buf, n, lay, colour, siting, rule=RIGHT):
    """n x h x w x 3 uint8 BGR of flat frame bytes under a siting ("replicate" or one of SITINGS): the restatement, or with another `rule` a
    wrong kernel"""
    f, h, w = lay["format"], lay["h"], lay["w"]
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        Y, cb, cr = samples(buf, i, lay, rule.nv12_stride if f == 3 else 2)
        if rule.cr_from_cb and siting != "replicate":
            cr = cb
        if f == 1 and rule.p010_late and siting != "replicate":
            up = lambda p: upsample_scalar(p >> 2, h, w, siting, True, rule) << 2
        else:
            up = lambda p: upsample_scalar(p, h, w, siting, f != 2, rule)
        rgb = (image.yuv10_to_bgr if f == 1 else image.yuv_to_bgr)(Y, up(cb), up(cr), colour)
        out[i] = np.stack(rgb, axis=-1)
    return out


def host(buf, lay, colour, siting):
    """the specification under test on the same bytes: image.yuv_to_bgr_host, or nv12_to_bgr_host for format 3"""
    if lay["format"] == 3:
        fb = lay["frame_bytes"]
        whole = np.zeros(_up(buf.size, fb), np.uint8)      # nv12_bytes takes whole frames
        whole[:buf.size] = buf
        return image.nv12_to_bgr_host(whole, lay["h"], lay["w"], colour=colour, siting=siting, **keywords(lay))
    return image.yuv_to_bgr_host(buf, FORMATS[lay["format"]], lay["h"], lay["w"], colour=colour, siting=siting, **keywords(lay))


# ---- the inputs of the GPU file --------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "fmt h w layout content")

# 2 x 2: every tap clamped, cw = ch = 1; 2 x 4 and 4 x 2: the smallest planes with a second chroma column or row; 6 x 10: the last patch of a
# row cut to 2 columns; 12 x 16: whole patches, the wide loads; 16 x 18: a ragged width; YUY2 at h = 1 and 3: no vertical step, odd heights
SIZES = [(2, 2), (2, 4), (4, 2), (6, 10), (12, 16), (16, 18)]
SIZES_YUY2 = SIZES + [(1, 6), (3, 6)]
IMPULSES = ("tl", "tr", "bl", "br", "top", "mid")      # a single chroma sample at every corner, on an edge and inside


def _cases():
    cases = []
    for fmt in FORMATS:
        for h, w in (SIZES_YUY2 if fmt == "yuy2" else SIZES):
            for name in ("aligned", "odd"):
                cases.append(Case(fmt, h, w, name, "random"))
        for name in (("yv12", "interleaved") if fmt == "i420" else ()):
            cases.append(Case(fmt, 16, 18, name, "random"))
        for where in IMPULSES:
            cases.append(Case(fmt, 12, 16, "aligned", "impulse-" + where))
    return cases


CASES = _cases()
_MADE = {}


def make(case):
    """(flat uint8 bytes, n, layout dict) of a case, made once: random content is 3 frames (luma and both chroma components independent);
    an impulse is 1 frame of random luma over flat chroma with a single sample of Cb and of Cr standing out"""
    if case not in _MADE:
        fmt, h, w = case.fmt, case.h, case.w
        ch, cw = (h if fmt == "yuy2" else h // 2), w // 2
        top = 1024 if fmt == "p010" else 256
        seed = CASES.index(case) if case in CASES else 999
        rng = np.random.default_rng(1000 + seed)
        lay = layout(fmt, h, w, case.layout)
        if case.content == "random":
            planes = [(rng.integers(0, top, (h, w)), rng.integers(0, top, (ch, cw)), rng.integers(0, top, (ch, cw))) for _ in range(3)]
        else:
            r, c = {"tl": (0, 0), "tr": (0, cw - 1), "bl": (ch - 1, 0), "br": (ch - 1, cw - 1), "top": (0, cw // 2 - 1),
                    "mid": (ch // 2 - 1, cw // 2)}[case.content.split("-")[1]]
            cb, cr = np.full((ch, cw), top * 3 // 8), np.full((ch, cw), top * 5 // 8)
            cb[r, c], cr[r, c] = top - 6, 10
            planes = [(rng.integers(0, top, (h, w)), cb, cr)]
        buf = place(planes, lay, 2000 + seed)
        buf.setflags(write=False)
        _MADE[case] = (buf, len(planes), lay)
    return _MADE[case]


_HOST = {}


def expected(case, colour, siting):
    """the host specification's BGR frames of a case, computed once and shared"""
    key = (case, colour, siting)
    if key not in _HOST:
        buf, n, lay = make(case)
        out = host(buf, lay, colour, siting)
        out.setflags(write=False)
        _HOST[key] = out
    return _HOST[key]
