"""Host-side frame preprocessing: counterparts of lib/utils/image.py:194-235."""
import numpy as np


def _resize_bilinear(im, out_h, out_w, scale_y=None, scale_x=None):
    """cv2.resize(..., INTER_LINEAR) geometry: half-pixel centres, source coordinate (dst + 0.5) * scale - 0.5 clamped to the
    image, where scale = 1 / fx when the caller gave fx (cv2 keeps the REQUESTED factor, not in / out, when dsize is derived
    from it -- lib/utils/image.py:209 calls it that way) and in / out otherwise.  Arithmetic in float64 with one final
    rounding; cv2's uint8 path uses 11-bit fixed-point weights and may differ by one grey level.  (The BASELINE path never
    gets here: 1024x2048 frames at SCALES (1024, 2048) have scale exactly 1.)"""
    h, w = im.shape[:2]
    if (h, w) == (out_h, out_w):
        return im
    sy = float(h) / out_h if scale_y is None else scale_y
    sx = float(w) / out_w if scale_x is None else scale_x
    ys = np.clip((np.arange(out_h) + 0.5) * sy - 0.5, 0, h - 1)
    xs = np.clip((np.arange(out_w) + 0.5) * sx - 0.5, 0, w - 1)
    y0 = np.floor(ys).astype(int)
    x0 = np.floor(xs).astype(int)
    y1 = np.minimum(y0 + 1, h - 1)
    x1 = np.minimum(x0 + 1, w - 1)
    fy = (ys - y0)[:, None, None]
    fx = (xs - x0)[None, :, None]
    a = im.astype(np.float64)
    top = a[y0][:, x0] * (1 - fx) + a[y0][:, x1] * fx
    bot = a[y1][:, x0] * (1 - fx) + a[y1][:, x1] * fx
    out = top * (1 - fy) + bot * fy
    if im.dtype == np.uint8:
        out = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out


def resize(im, target_size, max_size, stride=0):
    """Contract of lib/utils/image.py:194-222: the SHORT side goes to `target_size` unless that would push the long side past
    `max_size` (then the long side goes to `max_size`); with `stride` > 0 the result is zero-padded at the bottom / right to the
    next multiple of it (as float64, like the reference's pad buffer).  Returns (image, scale).  1024x2048 Cityscapes frames at
    SCALES (1024, 2048): scale exactly 1, nothing is resampled."""
    rows, cols = im.shape[:2]
    short, long_ = (rows, cols) if rows <= cols else (cols, rows)
    scale = float(target_size) / float(short)
    if np.round(scale * long_) > max_size:
        scale = float(max_size) / float(long_)
    if scale != 1.0:
        im = _resize_bilinear(im, int(round(rows * scale)), int(round(cols * scale)), 1.0 / scale, 1.0 / scale)
    if stride == 0:
        return im, scale
    up = lambda n: -(-n // stride) * stride         # next multiple of the stride
    canvas = np.zeros((up(im.shape[0]), up(im.shape[1]), im.shape[2]))
    canvas[:im.shape[0], :im.shape[1]] = im
    return canvas, scale


def resize_geometry(rows, cols, target_size, max_size, stride=0):
    """The geometry `resize` would produce for a rows x cols frame, WITHOUT resampling anything: (scale, out_h, out_w, H, W) --
    the scale `resize` returns, the size of the resized image and the size after padding to the stride (H, W = out_h, out_w
    when stride == 0).  The same expressions as `resize`, so the uint8 route of the library (accel_frame_u8, which is told
    out_h, out_w and the step instead of deriving them) and the host path cannot disagree about a rounding."""
    rows, cols = int(rows), int(cols)
    short, long_ = (rows, cols) if rows <= cols else (cols, rows)
    scale = float(target_size) / float(short)
    if np.round(scale * long_) > max_size:
        scale = float(max_size) / float(long_)
    out_h, out_w = (int(round(rows * scale)), int(round(cols * scale))) if scale != 1.0 else (rows, cols)
    if stride == 0:
        return scale, out_h, out_w, out_h, out_w
    up = lambda n: -(-n // stride) * stride
    return scale, out_h, out_w, up(out_h), up(out_w)


def resample_step(rows, cols, scale, out_h, out_w):
    """Source pixels per output pixel of the resize `resize` performs: 1 / scale -- and exactly 1.0 where it copies the frame,
    which is at scale 1 and ALSO where the rounded size equals the frame's (`_resize_bilinear` returns its input then)."""
    return 1.0 if scale == 1.0 or (int(out_h), int(out_w)) == (int(rows), int(cols)) else 1.0 / scale


def nearest_index(dst, src):
    """The row (or column) of a `src`-pixel map that each of `dst` output rows takes under nearest-neighbour resizing, in integer
    arithmetic: min(i * src // dst, src - 1).  Equal to the float64 expression of dataset/cityscape._nearest_resize (the
    reference's evaluator, lib/dataset/cityscape.py:227) for every size pair the tests walk; the form csrc/results_u8.hip computes."""
    return np.minimum(np.arange(int(dst), dtype=np.int64) * int(src) // int(dst), int(src) - 1)


def labels_to_source_host(labels, out_h, out_w, h, w):
    """The specification of accel_labels_to_source: label maps [n x] H x W whose valid (unpadded) region is out_h x out_w in the
    top-left corner -- what a network fed with resize(frame) produces -- taken back to the frame's own size h x w: the crop,
    resized with nearest neighbour.  Undoes `resize` for a label map (RawFrames.geometry holds out_h, out_w)."""
    a = np.asarray(labels)
    ys, xs = nearest_index(h, out_h), nearest_index(w, out_w)
    return np.ascontiguousarray(a[..., :int(out_h), :int(out_w)][..., ys, :][..., xs])


def colour_host(labels, palette, frames=None, alpha=256, rgb=True):
    """The specification of accel_labels_colour: `palette` (256 x 3 R, G, B, flat or not) looked up per label, [n x] h x w x 3 in
    R, G, B order (rgb=True, what PIL wants) or B, G, R (what the frames are).  With `frames` (uint8 B, G, R of the same size)
    every channel is (alpha * colour + (256 - alpha) * frame + 128) >> 8, alpha in 0 .. 256; 256 is the pure colour."""
    if not 0 <= int(alpha) <= 256:
        raise ValueError("alpha = %r, must be in 0 .. 256" % (alpha,))
    out = np.asarray(palette, np.uint8).reshape(-1, 3)[np.asarray(labels)]
    if not rgb:
        out = out[..., ::-1]
    if frames is not None and int(alpha) < 256:
        f = np.asarray(frames, np.uint8)
        f = f[..., ::-1] if rgb else f
        out = ((int(alpha) * out.astype(np.int64) + (256 - int(alpha)) * f.astype(np.int64) + 128) >> 8).astype(np.uint8)
    return np.ascontiguousarray(out)


def confidence_host(scores, out_h, out_w, h, w, is_prob=False):
    """The specification of accel_scores_confidence, in float64: scores n x ncls x H x W fp32 (valid region out_h x out_w in the
    top-left corner) -> (conf, margin, second, hist) at the source size h x w, pixel for pixel where labels_to_source_host puts
    the labels.
      conf    uint8    min(255, floor(256 * p)), p = 1 / sum_k exp(l_k - l_max) the largest softmax probability (classes summed in
                       ascending order); is_prob: the scores are probabilities already, min(255, floor(256 * float64(top1)))
      margin  float32  l_top1 - l_top2: one fp32 subtraction of two stored values, 0 on a tie at the top
      second  uint8    the first maximal index among the classes other than `best`, the first-max argmax
      hist    uint64   n x 256: the number of source pixels of each frame at each conf level"""
    s = np.asarray(scores, np.float32)
    if s.ndim != 4 or s.shape[1] < 2:
        raise ValueError("scores must be n x ncls x H x W with ncls >= 2, got shape %s" % (s.shape,))
    ys, xs = nearest_index(h, out_h), nearest_index(w, out_w)
    s = np.ascontiguousarray(s[:, :, :int(out_h), :int(out_w)][:, :, ys, :][:, :, :, xs])
    n, ncls = s.shape[:2]
    best = np.argmax(s, axis=1)                                   # the first maximal index
    top1 = np.take_along_axis(s, best[:, None], axis=1)[:, 0]
    is_best = np.arange(ncls).reshape(1, ncls, 1, 1) == best[:, None]
    others = np.where(is_best, -np.inf, s)
    # (a class at -inf can still be the runner-up: when every other class is at -inf the first of them is)
    second = np.argmax((others == others.max(axis=1, keepdims=True)) & ~is_best, axis=1)
    top2 = np.take_along_axis(s, second[:, None], axis=1)[:, 0]
    with np.errstate(invalid="ignore"):
        margin = (top1 - top2).astype(np.float32)
    if is_prob:
        scaled = 256.0 * top1.astype(np.float64)
    else:
        total = np.zeros(top1.shape, np.float64)
        for k in range(ncls):
            total += np.exp(s[:, k].astype(np.float64) - top1.astype(np.float64))
        scaled = 256.0 * (1.0 / total)
    conf = np.minimum(255.0, np.floor(scaled)).astype(np.uint8)
    hist = np.stack([np.bincount(c.reshape(-1), minlength=256) for c in conf]).astype(np.uint64)
    return conf, margin, second.astype(np.uint8), hist


def interpolation_taps(dst, src):
    """(i0, i1, f): the two rows (or columns) of a `src`-pixel region that each of `dst` output rows blends under bilinear resizing
    with half-pixel centres, and the float64 weight of the second.  The coordinate (i + 0.5) * src / dst - 0.5 clamped to the region,
    in integer arithmetic with ONE division in float64 -- the inverse of the resize `_resize_bilinear` applies on the way in, and the
    form csrc/scores_labels.hip computes (every intermediate is below 2^31 for sizes up to 32768)."""
    dst, src = int(dst), int(src)
    num = np.clip((2 * np.arange(dst, dtype=np.int64) + 1) * src - dst, 0, 2 * dst * (src - 1))
    i0 = num // (2 * dst)
    i1 = np.minimum(i0 + 1, src - 1)
    f = (num - 2 * dst * i0).astype(np.float64) / np.float64(2 * dst)
    return i0, i1, f


def labels_interpolated_host(scores, out_h, out_w, h, w):
    """The specification of accel_scores_labels: scores n x ncls x H x W fp32 (valid region out_h x out_w in the top-left corner) ->
    labels n x h x w uint8 at the source size: every class plane interpolated bilinearly to the source pixel (interpolation_taps; the
    padding is never read), the argmax taken there.  The blend is float64 with every operation rounded on its own, in the order of
    `_resize_bilinear`: top = a00 * (1 - fx) + a01 * fx, bot = a10 * (1 - fx) + a11 * fx, v = top * (1 - fy) + bot * fy.  The label
    is the first class with the largest v (ascending scan, strict >: np.argmax).  At h x w == out_h x out_w every weight is 0 and v
    is the stored score: the crop of the argmax.  Scores are assumed finite."""
    s = np.asarray(scores, np.float32)
    if s.ndim != 4:
        raise ValueError("scores must be n x ncls x H x W, got shape %s" % (s.shape,))
    n, ncls = s.shape[:2]
    if not (1 <= int(out_h) <= s.shape[2] and 1 <= int(out_w) <= s.shape[3]):
        raise ValueError("the valid region %d x %d does not lie in the %d x %d map" % (out_h, out_w, s.shape[2], s.shape[3]))
    y0, y1, fy = interpolation_taps(h, out_h)
    x0, x1, fx = interpolation_taps(w, out_w)
    fy, fx = fy[None, :, None], fx[None, None, :]
    gy, gx = 1 - fy, 1 - fx
    best = None
    label =np.zeros((n, int(h), int(w)), np.uint8)
    for k in range(ncls):
        a = s[:, k, :int(out_h), :int(out_w)].astype(np.float64)
        r0, r1 = a[:, y0], a[:, y1]
        top = r0[:, :, x0] * gx + r0[:, :, x1] * fx
        bot = r1[:, :, x0] * gx + r1[:, :, x1] * fx
        v = top * gy + bot * fy
        if k == 0:
            best = v
        else:
            better = v > best
            best = np.where(better, v, best)
            label[better] = k
    return label


def confidence_interpolated_host(scores, out_h, out_w, h, w, is_prob=False):
    """The specification of accel_scores_confidence_interp, in float64: scores n x ncls x H x W fp32 (valid region out_h x out_w in the
    top-left corner) -> (labels, conf, margin, second, hist) at the source size h x w, from the values v_k every class plane takes when it is
    interpolated to the source pixel exactly as labels_interpolated_host does it (interpolation_taps clamped to the region -- the padding is
    never read; the float64 blend with every operation rounded on its own, in that function's order).  Scores are assumed finite.
      labels  uint8    the first k with the largest v_k: labels_interpolated_host
      conf    uint8    min(255, floor(256 * p)), p = 1 / sum_k exp(v_k - v_best), classes summed in ascending order: the softmax of the
                       interpolated logits, whose argmax is the label; is_prob: the stored values are probabilities, blended the same way,
                       min(255, floor(256 * v_best)) -- no exponential, exact everywhere
      margin  float32  float32(v_best - v_second): one float64 subtraction, rounded once to fp32; 0 on a tie at the top
      second  uint8    the first maximal index among the classes other than the label, compared on the float64 v_k
      hist    uint64   n x 256: the number of source pixels of each frame at each conf level
    At h x w == out_h x out_w every weight is 0 and v_k is the stored score: confidence_host plus the crop of the argmax."""
    s = np.asarray(scores, np.float32)
    if s.ndim != 4 or s.shape[1] < 2:
        raise ValueError("scores must be n x ncls x H x W with ncls >= 2, got shape %s" % (s.shape,))
    n, ncls = s.shape[:2]
    if not (1 <= int(out_h) <= s.shape[2] and 1 <= int(out_w) <= s.shape[3]):
        raise ValueError("the valid region %d x %d does not lie in the %d x %d map" % (out_h, out_w, s.shape[2], s.shape[3]))
    y0, y1, fy = interpolation_taps(h, out_h)
    x0, x1, fx = interpolation_taps(w, out_w)
    fy, fx = fy[None, :, None], fx[None, None, :]
    gy, gx = 1 - fy, 1 - fx
    v = np.empty((n, ncls, int(h), int(w)), np.float64)
    for k in range(ncls):
        a = s[:, k, :int(out_h), :int(out_w)].astype(np.float64)
        r0, r1 = a[:, y0], a[:, y1]
        top = r0[:, :, x0] * gx + r0[:, :, x1] * fx
        bot = r1[:, :, x0] * gx + r1[:, :, x1] * fx
        v[:, k] = top * gy + bot * fy
    best = np.argmax(v, axis=1)                                   # the first maximal index
    top1 = np.take_along_axis(v, best[:, None], axis=1)[:, 0]
    is_best = np.arange(ncls).reshape(1, ncls, 1, 1) == best[:, None]
    others = np.where(is_best, -np.inf, v)
    second = np.argmax((others == others.max(axis=1, keepdims=True)) & ~is_best, axis=1)
    top2 = np.take_along_axis(v, second[:, None], axis=1)[:, 0]
    margin = (top1 - top2).astype(np.float32)
    if is_prob:
        scaled = 256.0 * top1
    else:
        total = np.zeros(top1.shape, np.float64)
        for k in range(ncls):
            total += np.exp(v[:, k] - top1)
        scaled = 256.0 * (1.0 / total)
    conf = np.minimum(255.0, np.floor(scaled)).astype(np.uint8)
    hist = np.stack([np.bincount(c.reshape(-1), minlength=256) for c in conf]).astype(np.uint64)
    return best.astype(np.uint8), conf, margin, second.astype(np.uint8), hist


def transform(im, pixel_means):
    """Contract of lib/utils/image.py:224-235: a BGR H x W x 3 frame becomes the 1 x 3 x H x W RGB tensor with the per-channel
    mean removed (`pixel_means` is given in B, G, R order like the frame).  float64 like the reference; arrays become fp32
    when they are handed to the predictor (demo.py:186)."""
    centred = np.asarray(im, np.float64) - np.asarray(pixel_means, np.float64).reshape(1, 1, 3)
    return np.ascontiguousarray(centred[:, :, ::-1].transpose(2, 0, 1))[None]


# ---- NV12 frames ------------------------------------------------------------------------------------------------------------------------------
# What a video decoder hands out: h rows of w luma bytes, then h/2 rows of w/2 interleaved (Cb, Cr) byte pairs, every row `pitch` bytes
# apart; the chroma plane starts at byte `uv_offset` of the frame and frame i at byte i * frame_bytes.  h and w are even.
NV12_COLOURS = {"bt601": 0, "bt601-full": 1, "bt709": 2, "bt709-full": 3}


def nv12_colour(colour):
    """the number 0 .. 3 of a colour mode given by name (NV12_COLOURS) or by number"""
    if isinstance(colour, str):
        if colour not in NV12_COLOURS:
            raise ValueError("colour = %r, must be one of %s" % (colour, ", ".join(sorted(NV12_COLOURS))))
        return NV12_COLOURS[colour]
    if isinstance(colour, (int, np.integer)) and not isinstance(colour, bool) and 0 <= int(colour) <= 3:
        return int(colour)
    raise ValueError("colour = %r, must be in 0 .. 3 or one of %s" % (colour, ", ".join(sorted(NV12_COLOURS))))


def _nv12_standard(colour):
    """(Kr, Kg, Kb, luma offset, luma scale, chroma scale) of a colour mode: BT.601 or BT.709, limited (16 .. 235 / 16 .. 240) or full range"""
    c = nv12_colour(colour)
    kr, kb = (0.299, 0.114) if c < 2 else (0.2126, 0.0722)
    limited = c in (0, 2)
    return kr, 1.0 - kr - kb, kb, (16 if limited else 0), (255.0 / 219.0 if limited else 1.0), (255.0 / 224.0 if limited else 1.0)


def nv12_matrix(colour):
    """the standard's own float64 values (yoff, ky, krv, kgu, kgv, kbu): R = ky (Y - yoff) + krv (Cr - 128), G = ky (Y - yoff) - kgu (Cb - 128)
    - kgv (Cr - 128), B = ky (Y - yoff) + kbu (Cb - 128)"""
    kr, kg, kb, yoff, ky, s = _nv12_standard(colour)
    krv, kbu = 2.0 * (1.0 - kr) * s, 2.0 * (1.0 - kb) * s
    return yoff, ky, krv, kbu * kb / kg, krv * kr / kg, kbu


def nv12_coefficients(colour):
    """(yoff, ky, krv, kgu, kgv, kbu) of the integer rule: round(65536 x the standard's value); what accel_nv12_coefficients returns"""
    m = nv12_matrix(colour)
    return (m[0],) + tuple(int(round(65536.0 * v)) for v in m[1:])


def nv12_layout(h, w, pitch=None, uv_offset=None, frame_bytes=None):
    """The layout dict the C ABI takes (h, w, pitch, uv_offset, frame_bytes), checked: tightly packed where nothing is given -- pitch = w,
    the chroma plane right behind the luma plane, the next frame right behind the chroma plane."""
    h, w = int(h), int(w)
    if h < 2 or h > 32768 or h % 2:
        raise ValueError("h = %d, must be even and in 2 .. 32768" % h)
    if w < 2 or w > 32768 or w % 2:
        raise ValueError("w = %d, must be even and in 2 .. 32768" % w)
    pitch = w if pitch is None else int(pitch)
    if pitch < w:
        raise ValueError("pitch = %d bytes, a row of w = %d pixels has %d" % (pitch, w, w))
    uv_offset = h * pitch if uv_offset is None else int(uv_offset)
    if uv_offset < h * pitch:
        raise ValueError("uv_offset = %d bytes, the luma plane ends at %d" % (uv_offset, h * pitch))
    end = uv_offset + (h // 2) * pitch
    frame_bytes = end if frame_bytes is None else int(frame_bytes)
    if frame_bytes < end:
        raise ValueError("frame_bytes = %d, the chroma plane ends at %d" % (frame_bytes, end))
    return dict(h=h, w=w, pitch=pitch, uv_offset=uv_offset, frame_bytes=frame_bytes)


def nv12_bytes(buf, layout):
    """`buf` (uint8, flat or n x frame_bytes) as an n x frame_bytes array of whole frames, or ValueError"""
    a = np.asarray(buf)
    if a.dtype != np.uint8:
        raise ValueError("NV12 bytes must be uint8, got %s" % a.dtype)
    fb = layout["frame_bytes"]
    if a.ndim not in (1, 2) or a.size == 0 or a.size % fb or (a.ndim == 2 and a.shape[1] != fb):
        raise ValueError("NV12 bytes must be flat or n x frame_bytes = n x %d, got shape %s" % (fb, a.shape))
    return a.reshape(-1, fb)


# ---- chroma siting ------------------------------------------------------------------------------------------------------------------------------
# Where the chroma samples of a subsampled frame lie against the luma grid (H.273 chroma_sample_loc_type 0, 1, 2), and the rule that brings
# them back to every luma pixel.  `replicate` is the nearest-neighbour rule of the routes above: pixel (x, y) takes sample (x >> 1, y >> 1).
# The others interpolate in integers, per axis with two neighbouring samples and weights that sum to 4 (k = coordinate >> 1):
#   co-sited (sample k lies on luma 2k)         even coordinate: (k: 4)            odd: (k: 2, k+1: 2)
#   centred  (sample k lies on luma 2k + 0.5)   even coordinate: (k-1: 1, k: 3)    odd: (k: 3, k+1: 1)
# indices clamped to the plane, and C = (sum_rows sum_cols wy wx c[row][col] + 8) >> 4: one rounding, none between the axes.  YUY2 has no
# vertical step (weight 4 on the pixel's own row).  Interlaced siting is not offered.
#                 horizontal   vertical
#   1 left        co-sited     centred      H.264 / HEVC default (type 0)
#   2 centre      centred      centred      JPEG, MPEG-1 (type 1)
#   3 topleft     co-sited     co-sited     BT.2020 / P010 (type 2)
CHROMA_SITINGS = {"replicate": 0, "left": 1, "centre": 2, "topleft": 3}
_SITING_MODES = {1: (0, 1), 2: (1, 1), 3: (0, 0)}      # siting -> (horizontal, vertical): 0 co-sited, 1 centred


def chroma_siting(siting):
    """the number 0 .. 3 of a chroma siting given by name (CHROMA_SITINGS) or by number"""
    if isinstance(siting, str):
        if siting not in CHROMA_SITINGS:
            raise ValueError("siting = %r, must be one of %s" % (siting, ", ".join(sorted(CHROMA_SITINGS))))
        return CHROMA_SITINGS[siting]
    if isinstance(siting, (int, np.integer)) and not isinstance(siting, bool) and 0 <= int(siting) <= 3:
        return int(siting)
    raise ValueError("siting = %r, must be in 0 .. 3 or one of %s" % (siting, ", ".join(sorted(CHROMA_SITINGS))))


def _siting_taps(size, count, mode):
    """The two taps of every luma coordinate 0 .. size - 1 on an axis with `count` chroma samples: (i0, w0, i1, w1), int64 arrays, indices
    clamped to [0, count - 1], w0 + w1 == 4.  mode 0 co-sited, 1 centred, None: no step on this axis (sample = coordinate, weight 4)."""
    x = np.arange(size, dtype=np.int64)
    if mode is None:
        return x, np.full(size, 4, np.int64), x, np.zeros(size, np.int64)
    k, odd = x >> 1, (x & 1).astype(bool)
    if mode == 0:
        i0, w0, i1, w1 = k, np.where(odd, 2, 4), np.where(odd, k + 1, k), np.where(odd, 2, 0)
    else:
        i0, w0, i1, w1 = np.where(odd, k, k - 1), np.where(odd, 3, 1), np.where(odd, k + 1, k), np.where(odd, 1, 3)
    return np.clip(i0, 0, count - 1), w0.astype(np.int64), np.clip(i1, 0, count - 1), w1.astype(np.int64)


def _sited(fetch, h, w, cw, ch, siting, vertical=True):
    """the h x w (leading axes kept) int64 array of interpolated chroma: fetch(rows, cols) returns the samples at chroma rows `rows` (h x 1) and
    columns `cols` (1 x w) -- every sample from wherever the caller keeps it"""
    hm, vm = _SITING_MODES[siting]
    x0, wx0, x1, wx1 = (t[None, :] for t in _siting_taps(w, cw, hm))
    y0, wy0, y1, wy1 = (t[:, None] for t in _siting_taps(h, ch, vm if vertical else None))
    f = lambda r, c: fetch(r, c).astype(np.int64)
    total = wy0 * (wx0 * f(y0, x0) + wx1 * f(y0, x1)) + wy1 * (wx0 * f(y1, x0) + wx1 * f(y1, x1))
    return (total + 8) >> 4


def chroma_upsample(plane, h, w, siting, vertical=True):
    """One chroma plane ([n x] ch x cw, integer samples; cw = w / 2, ch = h / 2, or ch = h where `vertical` is False: YUY2) brought to the
    h x w luma grid under a siting (the table above).  `replicate`: sample (x >> 1, y >> 1).  Returns int64 in the range of the samples."""
    s = chroma_siting(siting)
    p = np.asarray(plane)
    h, w = int(h), int(w)
    if p.ndim < 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError("plane must be an integer array [n x] ch x cw, got %s %s" % (p.dtype, p.shape))
    ch, cw = p.shape[-2:]
    if h < 1 or w < 2 or w % 2 or cw != w // 2 or ch != (h // 2 if vertical else h) or (vertical and h % 2):
        raise ValueError("a %d x %d chroma plane does not belong to a %d x %d frame%s" % (ch, cw, h, w, "" if vertical else " without a vertical step"))
    p = p.astype(np.int64)
    if s == 0:
        rows = np.arange(h) >> 1 if vertical else np.arange(h)
        return np.ascontiguousarray(p[..., rows[:, None], (np.arange(w) >> 1)[None, :]])
    return _sited(lambda r, c: p[..., r, c], h, w, cw, ch, s, vertical)


def yuv_to_bgr(y, cb, cr, colour=0):
    """The integer rule, the specification of csrc/frames_yuv.h: arrays of Y, Cb, Cr bytes -> (B, G, R) uint8 arrays.  With c = Y - yoff,
    d = Cb - 128, e = Cr - 128 in int32 and arithmetic right shifts: R = clip((ky c + krv e + 32768) >> 16), G = clip((ky c - kgu d - kgv e +
    32768) >> 16), B = clip((ky c + kbu d + 32768) >> 16)."""
    yoff, ky, krv, kgu, kgv, kbu = nv12_coefficients(colour)
    c = ky * (np.asarray(y).astype(np.int32) - yoff) + 32768
    d = np.asarray(cb).astype(np.int32) - 128
    e = np.asarray(cr).astype(np.int32) - 128
    clip = lambda v: np.clip(v >> 16, 0, 255).astype(np.uint8)
    return clip(c + kbu * d), clip(c - kgu * d - kgv * e), clip(c + krv * e)


def nv12_to_bgr_host(buf, h, w, pitch=None, uv_offset=None, frame_bytes=None, colour=0, siting="replicate"):
    """The specification of accel_nv12_to_bgr, and with resize + transform behind it of accel_frame_nv12: NV12 bytes (uint8, flat or
    n x frame_bytes) -> n x h x w x 3 uint8 BGR.  Pixel (x, y) takes Y at (x, y) and Cb, Cr at (x >> 1, y >> 1) (replicated chroma) through
    yuv_to_bgr.  Bytes in the gaps -- between rows, between the planes, after a frame -- are not interpreted.  With another `siting`
    (chroma_siting) Cb and Cr are interpolated by chroma_upsample first: the specification of the _sited entry points with format 3."""
    siting = chroma_siting(siting)
    lay = nv12_layout(h, w, pitch, uv_offset, frame_bytes)
    h, w, pitch, uv_offset = lay["h"], lay["w"], lay["pitch"], lay["uv_offset"]
    a = nv12_bytes(buf, lay)
    n = a.shape[0]
    luma = a[:, :h * pitch].reshape(n, h, pitch)[:, :, :w]
    uv = a[:, uv_offset:uv_offset + (h // 2) * pitch].reshape(n, h // 2, pitch)[:, :, :w].reshape(n, h // 2, w // 2, 2)
    up = (lambda p: np.repeat(np.repeat(p, 2, axis=1), 2, axis=2)) if siting == 0 else (lambda p: chroma_upsample(p, h, w, siting))
    return np.ascontiguousarray(np.stack(yuv_to_bgr(luma, up(uv[..., 0]), up(uv[..., 1]), colour), axis=-1))


def _subsample(p, siting, vertical=True):
    """a float64 n x h x w chroma plane at full resolution -> n x h/2 x w/2 (n x h x w/2 without the vertical step) samples sited as `siting`
    says: centre is the block mean; a co-sited axis takes [1 2 1] / 4 around the even coordinate, the edge replicated"""
    s = chroma_siting(siting)
    if s == 0:
        raise ValueError("frames are fabricated with a siting of their samples: left, centre or topleft, not replicate")
    hm, vm = _SITING_MODES[s]
    def axis(q, ax, mode):
        q = np.moveaxis(q, ax, -1)
        if mode == 1:
            q = 0.5 * (q[..., 0::2] + q[..., 1::2])
        else:
            e = np.concatenate([q[..., :1], q], axis=-1)
            q = 0.25 * e[..., 0:-1:2] + 0.5 * q[..., 0::2] + 0.25 * q[..., 1::2]
        return np.moveaxis(q, -1, ax)
    p = axis(p, 2, hm)
    return axis(p, 1, vm) if vertical else p


def bgr_to_nv12_host(frames, colour=0, siting="centre"):
    """Tightly packed NV12 bytes (n x h * w * 3 / 2 uint8) of uint8 BGR frames ([n x] h x w x 3, h and w even): the standard's forward matrix
    in float64, chroma the mean of each 2 x 2 block, rint, clip.  `siting` left or topleft: chroma sampled on the even column ([1 2 1] / 4, the
    edge replicated) and, for topleft, on the even row likewise.  A tool for fabricating inputs (the demo's stand-in for a decoder), NOT the
    specification of anything on the GPU, and not an inverse of nv12_to_bgr_host."""
    f = np.asarray(frames)
    if f.ndim == 3:
        f = f[None]
    if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3:
        raise ValueError("frames must be uint8 n x h x w x 3 (BGR), got %s %s" % (f.dtype, f.shape))
    n, h, w = f.shape[:3]
    if h % 2 or w % 2 or h < 2 or w < 2:
        raise ValueError("NV12 frames have an even height and width, got %d x %d" % (h, w))
    kr, kg, kb, yoff, ky, s = _nv12_standard(colour)
    b, g, r = (f[..., i].astype(np.float64) for i in range(3))
    y = kr * r + kg * g + kb * b
    block = lambda p: p.reshape(n, h // 2, 2, w // 2, 2).mean(axis=(2, 4))
    if chroma_siting(siting) != 2:
        block = lambda p: _subsample(p, siting)
    cb = 128.0 + block((b - y) / (2.0 * (1.0 - kb))) / s
    cr = 128.0 + block((r - y) / (2.0 * (1.0 - kr))) / s
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    out = np.empty((n, h * w * 3 // 2), np.uint8)
    out[:, :h * w] = q(yoff + y / ky).reshape(n, h * w)
    out[:, h * w:] = np.stack([q(cb), q(cr)], axis=-1).reshape(n, h * w // 2)
    return out


# ---- I420, P010 and YUY2 frames -----------------------------------------------------------------------------------------------------------------
# What a software decoder (I420; YV12 is I420 with the chroma planes in the other order), a 10-bit hardware decoder (P010) and a capture card
# or USB camera (YUY2) hand out.  Frame i starts at byte i * frame_bytes; chroma is replicated, as on the NV12 route, unless a siting is given.
#   I420   h rows of w luma bytes `pitch` apart from byte 0; the Cb plane at `u_offset` and the Cr plane at `v_offset`, each h/2 rows of w/2 bytes
#          `pitch_c` apart; pixel (x, y) takes chroma at (x >> 1, y >> 1); h, w even.  The chroma planes start at or after h * pitch and need
#          not be disjoint from each other (rows interleaved: pitch_c == pitch, v_offset == u_offset + pitch / 2)
#   YUY2   h rows `pitch` (>= 2 w) apart of Y0 Cb Y1 Cr quads; pixel (x, y) takes the chroma of quad x >> 1 of its own row; w even, h >= 1
#   P010   NV12's shape in little-endian 16-bit words: rows `pitch` (>= 2 w) bytes apart, a (Cb, Cr) word-pair plane at `u_offset`; the sample
#          is word >> 6, the low six bits are never looked at; h, w even; pitch, u_offset and frame_bytes are multiples of 2
YUV_FORMATS = {"i420": 0, "p010": 1, "yuy2": 2}


def yuv_format(fmt):
    """the number 0 .. 2 of a format given by name (YUV_FORMATS) or by number"""
    if isinstance(fmt, str):
        if fmt.lower() not in YUV_FORMATS:
            raise ValueError("format = %r, must be one of %s" % (fmt, ", ".join(sorted(YUV_FORMATS))))
        return YUV_FORMATS[fmt.lower()]
    if isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool) and 0 <= int(fmt) <= 2:
        return int(fmt)
    raise ValueError("format = %r, must be in 0 .. 2 or one of %s" % (fmt, ", ".join(sorted(YUV_FORMATS))))


def yuv_extent(layout):
    """the bytes one frame of a yuv_layout occupies: one past the last byte of the last row of its last plane"""
    f, h, w, pitch = layout["format"], layout["h"], layout["w"], layout["pitch"]
    if f == 0:
        return max(layout["u_offset"], layout["v_offset"]) + (h // 2 - 1) * layout["pitch_c"] + w // 2
    if f == 1:
        return layout["u_offset"] + (h // 2 - 1) * pitch + 2 * w
    return (h - 1) * pitch + 2 * w


def yuv_layout(fmt, h, w, pitch=None, pitch_c=None, u_offset=None, v_offset=None, frame_bytes=None):
    """The accel_yuv_layout the C ABI takes (format, h, w, pitch, pitch_c, u_offset, v_offset, frame_bytes), checked as the C ABI checks it.
    Tightly packed where nothing is given: pitch = a row (w bytes; 2 w for P010 and YUY2), I420's pitch_c = (pitch + 1) // 2, the Cb plane (the
    chroma plane of P010) right behind the luma plane, I420's Cr plane right behind its Cb plane, the next frame right behind the last byte of
    this one (yuv_extent).  A field the format does not use is 0, and giving it another value is an error."""
    f = yuv_format(fmt)
    name = sorted(YUV_FORMATS, key=YUV_FORMATS.get)[f].upper()
    h, w = int(h), int(w)
    even_h = f != 2
    if h < 1 or h > 32768 or (even_h and h % 2):
        raise ValueError("h = %d, must be %sin 1 .. 32768 for %s" % (h, "even and " if even_h else "", name))
    if w < 1 or w > 32768 or w % 2:
        raise ValueError("w = %d, must be even and in 1 .. 32768 for %s" % (w, name))
    row = w if f == 0 else 2 * w
    pitch = row if pitch is None else int(pitch)
    if pitch < row:
        raise ValueError("pitch = %d bytes, a row of w = %d %s pixels has %d" % (pitch, w, name, row))
    if f == 0:
        pitch_c = (pitch + 1) // 2 if pitch_c is None else int(pitch_c)
        if pitch_c < w // 2:
            raise ValueError("pitch_c = %d bytes, a chroma row of w = %d I420 pixels has %d" % (pitch_c, w, w // 2))
        u_offset = h * pitch if u_offset is None else int(u_offset)
        v_offset = u_offset + (h // 2) * pitch_c if v_offset is None else int(v_offset)
    else:
        for field, value in (("pitch_c", pitch_c), ("v_offset", v_offset)) + ((("u_offset", u_offset),) if f == 2 else ()):
            if value is not None and int(value) != 0:
                raise ValueError("%s = %d, but %s has no such field: it must be 0" % (field, int(value), name))
        pitch_c = v_offset = 0
        u_offset = 0 if f == 2 else (h * pitch if u_offset is None else int(u_offset))
    for field, value in (("u_offset", u_offset), ("v_offset", v_offset))[:(2, 1, 0)[f]]:
        if value < h * pitch:
            raise ValueError("%s = %d bytes, the luma plane ends at %d" % (field, value, h * pitch))
    lay = dict(format=f, h=h, w=w, pitch=pitch, pitch_c=pitch_c, u_offset=u_offset, v_offset=v_offset, frame_bytes=0)
    end = yuv_extent(lay)
    lay["frame_bytes"] = end if frame_bytes is None else int(frame_bytes)
    if lay["frame_bytes"] < end:
        raise ValueError("frame_bytes = %d, the last plane of a frame ends at %d" % (lay["frame_bytes"], end))
    if f == 1:
        for field in ("pitch", "u_offset", "frame_bytes"):
            if lay[field] % 2:
                raise ValueError("%s = %d, P010 words are 2-byte aligned: it must be even" % (field, lay[field]))
    return lay


def yuv_bytes(buf, layout):
    """`buf` as (flat uint8 array, n): n frames laid out `frame_bytes` apart.  uint8, flat or n x frame_bytes; a flat buffer may end with the last
    byte of its last frame ((n - 1) * frame_bytes + yuv_extent bytes).  uint16 is accepted for P010 and viewed as little-endian bytes."""
    a = np.asarray(buf)
    if a.dtype == np.uint16 and layout["format"] == 1:
        a = np.ascontiguousarray(np.atleast_1d(a).astype("<u2", copy=False)).view(np.uint8)
    if a.dtype != np.uint8:
        raise ValueError("frame bytes must be uint8%s, got %s" % (" or uint16" if layout["format"] == 1 else "", a.dtype))
    fb, end = layout["frame_bytes"], yuv_extent(layout)
    if a.ndim == 2 and a.shape[0] >= 1 and a.shape[1] == fb:
        return np.ascontiguousarray(a).reshape(-1), a.shape[0]
    n = (a.size - end) // fb + 1 if a.size >= end else 0
    if a.ndim != 1 or n < 1 or a.size > n * fb:
        raise ValueError("frame bytes must be n x frame_bytes = n x %d, or flat: (n - 1) x %d + %d .. n x %d bytes; got shape %s"
                         % (fb, fb, end, fb, a.shape))
    return np.ascontiguousarray(a), n


def yuv10_matrix(colour):
    """the standard's float64 values at 10 bits (yoff10, ky, krv, kgu, kgv, kbu) that take (Y10 - yoff10, Cb10 - 512, Cr10 - 512) to R, G, B on the
    0 .. 255 scale: the limited-range signal is 4 times the 8-bit one (nv12_matrix / 4), full range maps 1023 to 255 (nv12_matrix x 255 / 1023)"""
    m = nv12_matrix(colour)
    s = 0.25 if nv12_colour(colour) in (0, 2) else 255.0 / 1023.0
    return (4 * m[0],) + tuple(v * s for v in m[1:])


def yuv10_coefficients(colour):
    """(yoff, ky, krv, kgu, kgv, kbu) of P010's integer rule, what accel_yuv10_coefficients returns: with c = Y10 - 4 * yoff, d = Cb10 - 512,
    e = Cr10 - 512, R = clip((ky c + krv e + (1 << 17)) >> 18) and G, B alike.  Limited range (modes 0, 2): the integers of nv12_coefficients;
    full range (1, 3): round(65536 x the standard's value x 1020 / 1023) -- 1023, not 1020, is white."""
    if nv12_colour(colour) in (0, 2):
        return nv12_coefficients(colour)
    m = nv12_matrix(colour)
    return (m[0],) + tuple(int(round(65536.0 * v * 1020.0 / 1023.0)) for v in m[1:])


def yuv10_to_bgr(y, cb, cr, colour=0):
    """P010's integer rule, the specification of csrc/frames_yuv.hip for 10-bit samples: arrays of Y10, Cb10, Cr10 -> (B, G, R) uint8 arrays"""
    yoff, ky, krv, kgu, kgv, kbu = yuv10_coefficients(colour)
    c = ky * (np.asarray(y).astype(np.int32) - 4 * yoff) + (1 << 17)
    d = np.asarray(cb).astype(np.int32) - 512
    e = np.asarray(cr).astype(np.int32) - 512
    clip = lambda v: np.clip(v >> 18, 0, 255).astype(np.uint8)
    return clip(c + kbu * d), clip(c - kgu * d - kgv * e), clip(c + krv * e)


def yuv_to_bgr_host(buf, fmt, h, w, colour=0, siting="replicate", **layout):
    """The specification of accel_yuv_to_bgr, and with resize + transform behind it of accel_frame_yuv: I420, P010 or YUY2 bytes (see yuv_bytes;
    the layout keywords are those of yuv_layout) -> n x h x w x 3 uint8 BGR.  Every sample is fetched from its own byte address, so planes may
    interleave or overlap as the layout says; bytes in the gaps are not interpreted.  8-bit samples go through yuv_to_bgr, P010's word >> 6
    through yuv10_to_bgr.  With another `siting` (chroma_siting) Cb and Cr are interpolated first -- the rule of chroma_upsample, P010's on the
    10-bit samples, YUY2's without the vertical step: the specification of the _sited entry points."""
    siting = chroma_siting(siting)
    lay = yuv_layout(fmt, h, w, **layout)
    a, n = yuv_bytes(buf, lay)
    f, h, w, pitch = lay["format"], lay["h"], lay["w"], lay["pitch"]
    base = (np.arange(n, dtype=np.int64) * lay["frame_bytes"])[:, None, None]
    ys, xs = np.arange(h, dtype=np.int64)[None, :, None], np.arange(w, dtype=np.int64)[None, None, :]
    word = lambda i: (a[i].astype(np.int32) | a[i + 1].astype(np.int32) << 8) >> 6
    if siting:
        # the address of chroma sample (row, col) of every frame: n x rows x cols for index arrays rows (h x 1) and cols (1 x w)
        cw, ch, vertical = w // 2, (h if f == 2 else h // 2), f != 2
        if f == 0:
            at = lambda off: (lambda r, c: a[base + off + r[None] * lay["pitch_c"] + c[None]])
            cb, cr = at(lay["u_offset"]), at(lay["v_offset"])
        elif f == 2:
            at = lambda off: (lambda r, c: a[base + r[None] * pitch + 4 * c[None] + off])
            cb, cr = at(1), at(3)
        else:
            at = lambda off: (lambda r, c: word(base + lay["u_offset"] + r[None] * pitch + 4 * c[None] + off))
            cb, cr = at(0), at(2)
        cb, cr = (_sited(g, h, w, cw, ch, siting, vertical) for g in (cb, cr))
        if f == 1:
            bgr = yuv10_to_bgr(word(base + ys * pitch + 2 * xs), cb, cr, colour)
        else:
            bgr = yuv_to_bgr(a[base + ys * pitch + (xs if f == 0 else 2 * xs)], cb, cr, colour)
    elif f == 0:
        c = base + (ys >> 1) * lay["pitch_c"] + (xs >> 1)
        bgr = yuv_to_bgr(a[base + ys * pitch + xs], a[lay["u_offset"] + c], a[lay["v_offset"] + c], colour)
    elif f == 2:
        quad = base + ys * pitch + 4 * (xs >> 1)
        bgr = yuv_to_bgr(a[base + ys * pitch + 2 * xs], a[quad + 1], a[quad + 3], colour)
    else:
        uv = base + lay["u_offset"] + (ys >> 1) * pitch + 4 * (xs >> 1)
        bgr = yuv10_to_bgr(word(base + ys * pitch + 2 * xs), word(uv), word(uv + 2), colour)
    return np.ascontiguousarray(np.stack(bgr, axis=-1))


def bgr_to_yuv_host(frames, fmt, colour=0, siting="centre"):
    """Tightly packed I420, P010 or YUY2 bytes (n x frame_bytes uint8) of uint8 BGR frames ([n x] h x w x 3, h and w even): the standard's forward
    matrix in float64, chroma the mean of each 2 x 2 block (of each pair for YUY2), rint, clip; P010 samples sit in the top ten bits of their
    words.  `siting` left or topleft: chroma sampled as in bgr_to_nv12_host (for YUY2 both are [1 2 1] / 4 on the even column).  A tool for
    fabricating inputs (the demo's stand-in for a decoder), NOT the specification of anything on the GPU."""
    fm = yuv_format(fmt)
    f = np.asarray(frames)
    if f.ndim == 3:
        f = f[None]
    if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3:
        raise ValueError("frames must be uint8 n x h x w x 3 (BGR), got %s %s" % (f.dtype, f.shape))
    n, h, w = f.shape[:3]
    if h % 2 or w % 2 or h < 2 or w < 2:
        raise ValueError("%s frames have an even height and width, got %d x %d" % (sorted(YUV_FORMATS, key=YUV_FORMATS.get)[fm].upper(), h, w))
    kr, kg, kb, yoff, ky, s = _nv12_standard(colour)
    b, g, r = (f[..., i].astype(np.float64) for i in range(3))
    y = kr * r + kg * g + kb * b
    block = (lambda p: p.reshape(n, h, w // 2, 2).mean(axis=3)) if fm == 2 else (lambda p: p.reshape(n, h // 2, 2, w // 2, 2).mean(axis=(2, 4)))
    if chroma_siting(siting) != 2:
        block = lambda p: _subsample(p, siting, vertical=fm != 2)
    luma = yoff + y / ky
    cb = 128.0 + block((b - y) / (2.0 * (1.0 - kb))) / s
    cr = 128.0 + block((r - y) / (2.0 * (1.0 - kr))) / s
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    if fm == 0:
        return np.concatenate([q(luma).reshape(n, -1), q(cb).reshape(n, -1), q(cr).reshape(n, -1)], axis=1)
    if fm == 2:
        out = np.empty((n, h, w // 2, 4), np.uint8)
        out[..., 0], out[..., 2] = q(luma[:, :, 0::2]), q(luma[:, :, 1::2])
        out[..., 1], out[..., 3] = q(cb), q(cr)
        return out.reshape(n, -1)
    if yoff:        # limited range: the 10-bit signal is 4 times the 8-bit one
        luma, cb, cr = 4.0 * luma, 4.0 * cb, 4.0 * cr
    else:           # full range: 1023 is white, 512 is no chroma
        luma, cb, cr = luma * (1023.0 / 255.0), 512.0 + (cb - 128.0) * (1023.0 / 255.0), 512.0 + (cr - 128.0) * (1023.0 / 255.0)
    q10 = lambda p: (np.clip(np.rint(p), 0, 1023).astype("<u2") << 6)
    words = np.concatenate([q10(luma).reshape(n, -1), np.stack([q10(cb), q10(cr)], axis=-1).reshape(n, -1)], axis=1)
    return np.ascontiguousarray(words).view(np.uint8).reshape(n, -1)


# ---- the overlay in the frame's own format --------------------------------------------------------------------------------------------------------
# A label map blended over NV12, I420 / YV12, P010 or YUY2 frames and written back as the same format in the same layout (csrc/overlay_yuv.hip):
# the palette goes to (Y, Cb, Cr) ONCE, on the host, in float64 (palette_ycbcr); everything per sample is integer arithmetic with one rounding
# (overlay_yuv_host).  The overlay's chroma is the mean of the palette colours over the luma pixels a chroma sample covers -- whatever the siting
# of the frame's own samples, which are blended where they are and are not resited.
def palette_ycbcr(palette, colour, bits=8):
    """A 256 x 3 R, G, B palette as the 256 x 3 uint16 table (Y, Cb, Cr) accel_labels_overlay_yuv takes, in the units of the samples: the float64
    forward matrix of bgr_to_nv12_host for `colour` (NV12_COLOURS) -- y = kr r + kg g + kb b, Y = yoff + y / ky, Cb = 128 + (b - y) / (2 (1 - kb)) / s,
    Cr likewise with r and kr -- then rint and a clip to 0 .. 255.  bits=10 (P010): everything before the rounding, the luma offset and the 128
    included, times 4 in the limited-range modes and times 1023 / 255 in the full-range ones, then rint and a clip to 0 .. 1023 (so a grey is
    (.., 512, 512) in the limited modes and (.., 514, 514) in the full-range ones: 128 x 1023 / 255 = 513.5)."""
    if bits not in (8, 10):
        raise ValueError("bits = %r, must be 8 or 10" % (bits,))
    p = np.asarray(palette, np.uint8).reshape(-1)
    if p.size != 768:
        raise ValueError("the palette must hold 256 x 3 bytes (R, G, B), got %d" % p.size)
    kr, kg, kb, yoff, ky, s = _nv12_standard(colour)
    r, g, b = (p.reshape(256, 3)[:, i].astype(np.float64) for i in range(3))
    y = kr * r + kg * g + kb * b
    ycc = np.stack([yoff + y / ky, 128.0 + (b - y) / (2.0 * (1.0 - kb)) / s, 128.0 + (r - y) / (2.0 * (1.0 - kr)) / s], axis=1)
    if bits == 10:
        ycc = ycc * (4.0 if yoff else 1023.0 / 255.0)
    return np.clip(np.rint(ycc), 0, (1 << bits) - 1).astype(np.uint16)


def overlay_format(fmt):
    """the number 0 .. 3 of a format an overlay is written in: those of yuv_format, and "nv12" or 3 for NV12"""
    if (isinstance(fmt, str) and fmt.lower() == "nv12") or (isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool) and int(fmt) == 3):
        return 3
    return yuv_format(fmt)


def overlay_layout(fmt, h, w, **layout):
    """the layout dict of overlay_yuv_host and accel_labels_overlay_yuv: yuv_layout for formats 0 .. 2; for NV12 (format 3) the fields of nv12_layout
    under the names of the C struct -- pitch, u_offset (the chroma plane; `uv_offset` is accepted too), frame_bytes, pitch_c = v_offset = 0"""
    f = overlay_format(fmt)
    if f != 3:
        return yuv_layout(f, h, w, **layout)
    layout = dict(layout)
    uv = layout.pop("u_offset", None)
    uv = layout.pop("uv_offset", None) if uv is None else uv
    for field in ("pitch_c", "v_offset"):
        value = layout.pop(field, None)
        if value is not None and int(value) != 0:
            raise ValueError("%s = %d, but NV12 has no such field: it must be 0" % (field, int(value)))
    lay = nv12_layout(h, w, layout.pop("pitch", None), uv, layout.pop("frame_bytes", None))
    if layout:
        raise TypeError("unknown layout keywords for NV12: %s" % ", ".join(sorted(layout)))
    return dict(format=3, h=lay["h"], w=lay["w"], pitch=lay["pitch"], pitch_c=0, u_offset=lay["uv_offset"], v_offset=0, frame_bytes=lay["frame_bytes"])


def overlay_yuv_host(buf, fmt, h, w, labels_at_source, table, alpha, **layout):
    """The specification of accel_labels_overlay_yuv: the frames in `buf` (I420 / YV12, P010, YUY2 as for yuv_to_bgr_host; "nv12" or 3: NV12 with the
    keywords pitch, u_offset, frame_bytes) blended with the colours table[label] of `labels_at_source` ([n x] h x w, the labels of the source pixels:
    labels_to_source_host or labels_interpolated_host) and returned as a uint8 copy of `buf` in which only the samples differ.  `table` is 256 x 3
    (Y, Cb, Cr) in the units of the samples (palette_ycbcr), a = alpha in 0 .. 256.  Integers, one rounding per sample:
        luma            Y'  = (a * T[L].Y + (256 - a) * Y + 128) >> 8
        4:2:0 chroma    Cb' = (a * S + (256 - a) * 4 * Cb + 512) >> 10, S = the sum of T[L].Cb over the sample's 2 x 2 luma pixels; Cr alike
        4:2:2 chroma    Cb' = (a * S2 + (256 - a) * 2 * Cb + 256) >> 9, S2 over the two pixels of the quad (YUY2)
        P010            the operands are word >> 6; the stored word is sample << 6
    The overlay's chroma is the block mean of the table's colours whatever the siting of the frame's samples, which are not resited."""
    a = int(alpha)
    if not 0 <= a <= 256:
        raise ValueError("alpha = %r, must be in 0 .. 256" % (alpha,))
    lay = overlay_layout(fmt, h, w, **layout)
    f, h, w, pitch = lay["format"], lay["h"], lay["w"], lay["pitch"]
    src = np.asarray(buf)
    if f == 3:
        flat = np.ascontiguousarray(nv12_bytes(src, dict(frame_bytes=lay["frame_bytes"]))).reshape(-1)
        n = flat.size // lay["frame_bytes"]
    else:
        flat, n = yuv_bytes(src, lay)
    T = np.asarray(table).astype(np.int64).reshape(-1)
    top = 1023 if f == 1 else 255
    if T.size != 768 or T.min() < 0 or T.max() > top:
        raise ValueError("the table must hold 256 x 3 values (Y, Cb, Cr) in 0 .. %d" % top)
    T = T.reshape(256, 3)
    L = np.asarray(labels_at_source)
    if L.ndim == 2:
        L = L[None]
    if L.shape != (n, h, w):
        raise ValueError("labels of shape %s for %d frames of %d x %d" % (L.shape, n, h, w))
    out = flat.copy()
    ia = 256 - a
    base = (np.arange(n, dtype=np.int64) * lay["frame_bytes"])[:, None, None]
    ys, xs = np.arange(h, dtype=np.int64)[None, :, None], np.arange(w, dtype=np.int64)[None, None, :]
    cxs = np.arange(w // 2, dtype=np.int64)[None, None, :]
    if f == 1:
        fetch = lambda i: (flat[i].astype(np.int64) | flat[i + 1].astype(np.int64) << 8) >> 6
        def store(i, v):
            out[i], out[i + 1] = ((v << 6) & 255).astype(np.uint8), (v >> 2).astype(np.uint8)
    else:
        fetch = lambda i: flat[i].astype(np.int64)
        def store(i, v):
            out[i] = v.astype(np.uint8)
    luma = base + ys * pitch + xs * (1 if f in (0, 3) else 2)
    store(luma, (a * T[L, 0] + ia * fetch(luma) + 128) >> 8)
    if f == 2:
        quad = base + ys * pitch + 4 * cxs
        for ch, at in ((1, quad + 1), (2, quad + 3)):
            s = T[L, ch].reshape(n, h, w // 2, 2).sum(axis=3)
            store(at, (a * s + ia * 2 * fetch(at) + 256) >> 9)
        return out.reshape(src.shape) if src.dtype == np.uint8 else out
    cys = np.arange(h // 2, dtype=np.int64)[None, :, None]
    if f == 0:
        c = base + cys * lay["pitch_c"] + cxs
        planes = ((1, lay["u_offset"] + c), (2, lay["v_offset"] + c))
    elif f == 3:
        c = base + lay["u_offset"] + cys * pitch + 2 * cxs
        planes = ((1, c), (2, c + 1))
    else:
        c = base + lay["u_offset"] + cys * pitch + 4 * cxs
        planes = ((1, c), (2, c + 2))
    for ch, at in planes:
        s = T[L, ch].reshape(n, h // 2, 2, w // 2, 2).sum(axis=(2, 4))
        store(at, (a * s + ia * 4 * fetch(at) + 512) >> 10)
    return out.reshape(src.shape) if src.dtype == np.uint8 else out


# ---- frame change: the measure behind content-adaptive key frames (csrc/frame_change.hip restates both functions bit for bit) ----------------
FRAME_CELLS = (8, 16, 32, 64)


def frame_cells(out_h, out_w, cell):
    """(gh, gw): the grid of cell x cell cells that covers a valid region of out_h x out_w pixels; the last row / column of cells may be smaller"""
    cell = int(cell)
    if cell not in FRAME_CELLS:
        raise ValueError("cell = %r, must be one of %s" % (cell, ", ".join(str(c) for c in FRAME_CELLS)))
    return -(-int(out_h) // cell), -(-int(out_w) // cell)


def frame_cell_areas(out_h, out_w, cell):
    """gh x gw int64: the number of valid pixels of every cell"""
    gh, gw = frame_cells(out_h, out_w, cell)
    hs = np.minimum(cell, int(out_h) - cell * np.arange(gh, dtype=np.int64))
    ws = np.minimum(cell, int(out_w) - cell * np.arange(gw, dtype=np.int64))
    return hs[:, None] * ws[None, :]


def frame_level_q(level):
    """the public `level` (grey levels of mean absolute change per pixel of a cell) in the kernel's units, 64 per grey level"""
    q = int(round(float(level) * 64))
    if not 0 <= q <= 32768:
        raise ValueError("level = %r, must be in 0 .. 512 grey levels" % (level,))
    return q


def frame_signature_host(x, out_h, out_w, cell):
    """The specification of the signature half of accel_frame_change.  `x` is the image input, n x 3 x H x W fp32 (planes R, G, B, mean-subtracted,
    padded), of which only the valid region out_h x out_w in the top-left corner is looked at.  Integers throughout:
        q = int(rint(fmin(fmax(x, -512), 512) * 8))     fp32, round half to even; C fmaxf / fminf: NaN gives -4096, +-inf gives +-4096
        v = 2 qR + 5 qG + qB                            64 units per grey level
        S[cy][cx] = the sum of v over the valid pixels of cell (cy, cx)
    -> n x gh x gw int32 (|S| <= 64 * 64 * 8 * 4096 = 2^27)."""
    x = np.asarray(x, np.float32)
    if x.ndim != 4 or x.shape[1] != 3:
        raise ValueError("x must be n x 3 x H x W fp32, got shape %s" % (x.shape,))
    n, _, H, W = x.shape
    out_h, out_w = int(out_h), int(out_w)
    if not (1 <= out_h <= H and 1 <= out_w <= W):
        raise ValueError("out_h x out_w = %d x %d, must be in 1 x 1 .. H x W = %d x %d" % (out_h, out_w, H, W))
    gh, gw = frame_cells(out_h, out_w, cell)
    valid = x[:, :, :out_h, :out_w]
    clamped = np.fmin(np.fmax(valid, np.float32(-512.0)), np.float32(512.0))
    q = np.rint(clamped * np.float32(8.0)).astype(np.int64)
    v = 2 * q[:, 0] + 5 * q[:, 1] + q[:, 2]
    full = np.zeros((n, gh * cell, gw * cell), np.int64)
    full[:, :out_h, :out_w] = v
    return full.reshape(n, gh, cell, gw, cell).sum(axis=(2, 4)).astype(np.int32)


def frame_change_host(sig, sig_key, out_h, out_w, cell, level_q):
    """The specification of the comparing half of accel_frame_change: two signatures (frame_signature_host) of the same geometry, frame i with frame
    i.  Per cell d = |S - S_key| and the cell is CHANGED iff d > level_q * area (strict, int64; area = its valid pixels).  Returns per frame
    (changed uint32: the number of changed cells, sad uint64: the sum of d, mask n x gh x gw uint8: 1 where a cell changed)."""
    level_q = int(level_q)
    if not 0 <= level_q <= 32768:
        raise ValueError("level_q = %d, must be in 0 .. 32768" % level_q)
    a, b = np.asarray(sig).astype(np.int64), np.asarray(sig_key).astype(np.int64)
    gh, gw = frame_cells(out_h, out_w, cell)
    if a.ndim != 3 or a.shape[1:] != (gh, gw) or a.shape != b.shape:
        raise ValueError("signatures of shapes %s and %s for a grid of %d x %d cells" % (a.shape, b.shape, gh, gw))
    d = np.abs(a - b)
    mask = d > level_q * frame_cell_areas(out_h, out_w, cell)[None]
    return mask.sum(axis=(1, 2)).astype(np.uint32), d.sum(axis=(1, 2)).astype(np.uint64), mask.astype(np.uint8)


# ---- summary of finished frames: areas, coordinate sums, boxes and class transitions (csrc/labels_summary.hip restates it bit for bit) --------
def labels_summary_host(labels, out_h, out_w, h, w, ncls, prev=None):
    """The specification of accel_labels_summary.  `labels` is [n x] H x W uint8 with the valid region out_h x out_w; with
        L(f, y, x) = labels[f][min(y * out_h // h, out_h - 1)][min(x * out_w // w, out_w - 1)]       (labels_to_source_host)
    it returns (stats, box, trans, kept) for every frame f and class k in 0 .. ncls - 1 (ncls in 1 .. 32; ids >= ncls are ignored):
        stats  n x ncls x 3 uint64: (area, sum_x, sum_y) over the source pixels (y, x) with L == k
        box    n x ncls x 4 int32: (x0, y0, x1, y1), their inclusive extremes; (w, h, -1, -1) for a class without a pixel
        trans  n x (ncls * ncls) uint64, or None without `prev` (n x h x w uint8, the previous frame's labels at the source size):
               trans[f, p * ncls + c] = the source pixels with prev == p < ncls and L == c < ncls (rows: the previous frame)
        kept   n x h x w uint8: the current map at the source size (labels_to_source_host), the `prev` of the next frame"""
    a = np.asarray(labels, np.uint8)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("labels must be [n x] H x W uint8, got shape %s" % (a.shape,))
    n, H, W = a.shape
    out_h, out_w, h, w, ncls = int(out_h), int(out_w), int(h), int(w), int(ncls)
    if not (1 <= out_h <= H and 1 <= out_w <= W):
        raise ValueError("out_h x out_w = %d x %d, must be in 1 x 1 .. H x W = %d x %d" % (out_h, out_w, H, W))
    if not (1 <= h <= 32768 and 1 <= w <= 32768):
        raise ValueError("h x w = %d x %d, must be in 1 .. 32768" % (h, w))
    if not 1 <= ncls <= 32:
        raise ValueError("ncls = %d, must be in 1 .. 32" % ncls)
    kept = labels_to_source_host(a, out_h, out_w, h, w)
    stats = np.zeros((n, ncls, 3), np.uint64)
    box = np.empty((n, ncls, 4), np.int32)
    box[...] = (w, h, -1, -1)
    xs, ys = np.arange(w, dtype=np.uint64), np.arange(h, dtype=np.uint64)
    for f in range(n):
        for k in range(ncls):
            mask = kept[f] == k
            cols, rows = mask.sum(axis=0, dtype=np.uint64), mask.sum(axis=1, dtype=np.uint64)       # pixels of the class per column / per row
            area = int(cols.sum())
            if not area:
                continue
            stats[f, k] = (area, int((cols * xs).sum()), int((rows * ys).sum()))
            cx, cy = np.nonzero(cols)[0], np.nonzero(rows)[0]
            box[f, k] = (cx[0], cy[0], cx[-1], cy[-1])
    trans = None
    if prev is not None:
        p = np.asarray(prev, np.uint8)
        if p.ndim == 2:
            p = p[None]
        if p.shape != kept.shape:
            raise ValueError("prev of shape %s for a source-size map of shape %s" % (p.shape, kept.shape))
        trans = np.zeros((n, ncls * ncls), np.uint64)
        for f in range(n):
            ok = (p[f] < ncls) & (kept[f] < ncls)
            pair = p[f][ok].astype(np.int64) * ncls + kept[f][ok].astype(np.int64)
            trans[f] = np.bincount(pair, minlength=ncls * ncls).astype(np.uint64)
    return stats, box, trans, kept


def summary_centroids(stats):
    """(sum_x / area, sum_y / area) of labels_summary_host's stats: float64 [...] x ncls x 2, NaN where the class is empty"""
    s = np.asarray(stats).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s[..., :1] > 0, s[..., 1:3] / s[..., :1], np.nan)


def summary_churn(trans):
    """the label churn per frame: 1 - trace / total of labels_summary_host's trans ([n x] ncls * ncls counts, one flat matrix per frame), the
    share of counted pixels whose class changed; NaN where nothing was counted"""
    t = np.asarray(trans).astype(np.float64)
    ncls = int(round(t.shape[-1] ** 0.5))
    if ncls * ncls != t.shape[-1]:
        raise ValueError("trans must hold ncls * ncls counts per frame, got shape %s" % (t.shape,))
    total = t.sum(axis=-1)
    trace = t[..., ::ncls + 1].sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total > 0, 1.0 - trace / total, np.nan)


# ---- connected components of finished frames: objects per class (csrc/labels_components.hip restates it bit for bit) ---------------------------
def labels_components_host(labels, out_h, out_w, h, w, ncls, connectivity=8, min_area=1, max_components=1024, ids=False):
    """The specification of accel_labels_components.  `labels` is [n x] H x W uint8 with the valid region out_h x out_w; L is the map at the source
    size h x w under the nearest rule (labels_to_source_host).  A pixel with L >= ncls is background: it belongs to no component and separates
    components.  Two other pixels of one frame are joined when their labels are equal and they are 4-adjacent (connectivity=8: or diagonally
    adjacent); a component is a class of the transitive closure, its anchor its first pixel in raster order (the smallest y * w + x).  The
    REPORTED components of a frame are those with area >= min_area, in ascending anchor order.  Returns (count, comp, sums[, ids]):
        count  n int32: the reported components of the frame -- the full number, also above max_components
        comp   n x max_components x 8 int32: (class, area, x0, y0, x1, y1, ax, ay) of the first min(count, max_components) of them -- the
               inclusive box and the anchor -- and -1 in the records after them
        sums   n x max_components x 2 uint64: (sum_x, sum_y) over the component's source pixels; 0 in the unused records
        ids    n x h x w int32 (ids=True): per source pixel the index of its component's record; -1 for background, for components below
               min_area and for components beyond max_components
    Pure integer arithmetic: rows are cut into runs, runs of adjacent rows are united towards the smaller run (a union-find over runs)."""
    a = np.asarray(labels, np.uint8)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("labels must be [n x] H x W uint8, got shape %s" % (a.shape,))
    n, H, W = a.shape
    out_h, out_w, h, w, ncls = int(out_h), int(out_w), int(h), int(w), int(ncls)
    connectivity, min_area, max_components = int(connectivity), int(min_area), int(max_components)
    if not (1 <= out_h <= H and 1 <= out_w <= W):
        raise ValueError("out_h x out_w = %d x %d, must be in 1 x 1 .. H x W = %d x %d" % (out_h, out_w, H, W))
    if not (1 <= h <= 32768 and 1 <= w <= 32768):
        raise ValueError("h x w = %d x %d, must be in 1 .. 32768" % (h, w))
    if not 1 <= ncls <= 32:
        raise ValueError("ncls = %d, must be in 1 .. 32" % ncls)
    if connectivity not in (4, 8):
        raise ValueError("connectivity = %d, must be 4 or 8" % connectivity)
    if min_area < 1:
        raise ValueError("min_area = %d, must be >= 1" % min_area)
    if not 1 <= max_components <= 65536:
        raise ValueError("max_components = %d, must be in 1 .. 65536" % max_components)
    src = labels_to_source_host(a, out_h, out_w, h, w)
    reach = 1 if connectivity == 8 else 0
    count = np.zeros(n, np.int32)
    comp = np.full((n, max_components, 8), -1, np.int32)
    sums = np.zeros((n, max_components, 2), np.uint64)
    pix = np.full((n, h, w), -1, np.int32) if ids else None
    for f in range(n):
        L = src[f]
        start = L < ncls
        start[:, 1:] &= L[:, 1:] != L[:, :-1]
        ry, rx0 = np.nonzero(start)                              # the runs, in raster order of their first pixels
        nr = ry.size
        if not nr:
            continue
        stop = L < ncls
        stop[:, :-1] &= L[:, :-1] != L[:, 1:]
        rx1 = np.nonzero(stop)[1]
        rl = L[ry, rx0]
        first = np.searchsorted(ry, np.arange(h + 1))            # the first run of every row
        parent = list(range(nr))
        y_, x0_, x1_, l_, first_ = ry.tolist(), rx0.tolist(), rx1.tolist(), rl.tolist(), first.tolist()

        def join(i, j):
            if x0_[i] <= x1_[j] + reach and x0_[j] <= x1_[i] + reach and l_[i] == l_[j]:
                while parent[i] != i:
                    i = parent[i]
                while parent[j] != j:
                    j = parent[j]
                if i < j:
                    parent[j] = i
                elif j < i:
                    parent[i] = j

        for y in range(1, h):
            i, i_end, j, j_end = first_[y - 1], first_[y], first_[y], first_[y + 1]
            while i < i_end and j < j_end:                       # the run that ends first has met every run of the other row it can touch
                join(i, j)
                if x1_[i] < x1_[j]:
                    i += 1
                elif x1_[j] < x1_[i]:
                    j += 1
                else:                                            # both end here: the next run of either row may still touch the other diagonally
                    if i + 1 < i_end:
                        join(i + 1, j)
                    j += 1
        for i in range(nr):                                      # parent[i] <= i: one pass in raster order makes every run point at its root
            parent[i] = parent[parent[i]]
        root = np.asarray(parent, np.int64)
        x0, x1, yy = rx0.astype(np.int64), rx1.astype(np.int64), ry.astype(np.int64)
        length = x1 - x0 + 1
        area, sx, sy = np.zeros(nr, np.int64), np.zeros(nr, np.int64), np.zeros(nr, np.int64)
        np.add.at(area, root, length)
        np.add.at(sx, root, (x0 + x1) * length // 2)
        np.add.at(sy, root, yy * length)
        bx0, by0, bx1, by1 = np.full(nr, w, np.int64), np.full(nr, h, np.int64), np.full(nr, -1, np.int64), np.full(nr, -1, np.int64)
        np.minimum.at(bx0, root, x0)
        np.minimum.at(by0, root, yy)
        np.maximum.at(bx1, root, x1)
        np.maximum.at(by1, root, yy)
        keep = np.nonzero((root == np.arange(nr)) & (area >= min_area))[0]      # ascending run index: ascending anchor
        count[f] = keep.size
        keep = keep[:max_components]
        k = keep.size
        comp[f, :k] = np.stack([rl[keep].astype(np.int64), area[keep], bx0[keep], by0[keep], bx1[keep], by1[keep], x0[keep], yy[keep]], axis=1)
        sums[f, :k, 0] = sx[keep].astype(np.uint64)
        sums[f, :k, 1] = sy[keep].astype(np.uint64)
        if ids:
            slot = np.full(nr, -1, np.int32)
            slot[keep] = np.arange(k, dtype=np.int32)
            per_run = slot[root]
            flat = pix[f].reshape(-1)
            at = np.repeat(yy * w + x0 - np.cumsum(length) + length, length) + np.arange(int(length.sum()))
            flat[at] = np.repeat(per_run, length)
    return (count, comp, sums, pix) if ids else (count, comp, sums)


def components_centroids(comp, sums):
    """(sum_x / area, sum_y / area) of labels_components_host's records: float64 [...] x max_components x 2, NaN in the unused records"""
    area = np.asarray(comp)[..., 1:2].astype(np.float64)
    s = np.asarray(sums).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(area > 0, s / area, np.nan)


def components_of(result, frame):
    """the trimmed records of one frame of a (count, comp, sums[, ids]) result: (comp k x 8, sums k x 2) with k = min(count, max_components)"""
    count, comp, sums = result[0], result[1], result[2]
    k = min(int(count[frame]), comp.shape[1])
    return comp[frame, :k], sums[frame, :k]


# ---- trimap evaluation: the confusion matrix in bands around the ground truth's boundaries (csrc/labels_band.hip restates it bit for bit) --------
def _u8_batch(maps, what):
    a = np.asarray(maps, np.uint8)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("%s must be [n x] h x w uint8, got shape %s" % (what, a.shape))
    return a


def band_widths(widths):
    """the widths of a trimap as a tuple of ints: 1 to 4 strictly ascending values in 1 .. 16, or ValueError"""
    try:
        ws = tuple(int(v) for v in widths)
    except (TypeError, ValueError):
        raise ValueError("widths must be a sequence of 1 to 4 integers, got %r" % (widths,))
    if not 1 <= len(ws) <= 4:
        raise ValueError("widths holds %d values, must hold 1 .. 4" % len(ws))
    if any(not 1 <= v <= 16 for v in ws):
        raise ValueError("widths = %s, every width must be in 1 .. 16" % (ws,))
    if any(b <= a for a, b in zip(ws, ws[1:])):
        raise ValueError("widths = %s, must be strictly ascending" % (ws,))
    return ws


def boundary_edges_host(maps):
    """[n x] h x w uint8 -> n x h x w bool: the pixels with a 4-neighbour INSIDE the frame that holds another byte.  Raw bytes: the border between a
    class and an ignored id is an edge.  The frames of a batch are independent"""
    g = _u8_batch(maps, "maps")
    e = np.zeros(g.shape, bool)
    dy, dx = g[:, 1:, :] != g[:, :-1, :], g[:, :, 1:] != g[:, :, :-1]
    e[:, 1:, :] |= dy
    e[:, :-1, :] |= dy
    e[:, :, 1:] |= dx
    e[:, :, :-1] |= dx
    return e


def boundary_distance_host(maps, cap):
    """The specification of accel_boundary_distance: n x h x w uint8,
        d(y, x) = min(cap, min over edge pixels (y', x') of max(|y - y'|, |x - x'|))        (boundary_edges_host; cap in 1 .. 16)
    the Chebyshev distance to the nearest edge pixel: 0 on one, cap where none lies closer and where the map has no edge.  Written as cap - 1
    rounds of 3 x 3 dilation of the edge set: a pixel first reached in round r has d = r."""
    cap = int(cap)
    if not 1 <= cap <= 16:
        raise ValueError("cap = %d, must be in 1 .. 16" % cap)
    reached = boundary_edges_host(maps)
    d = np.where(reached, 0, cap).astype(np.uint8)
    for r in range(1, cap):
        grown = reached.copy()
        grown[:, 1:, :] |= reached[:, :-1, :]
        grown[:, :-1, :] |= reached[:, 1:, :]
        rows = grown.copy()
        rows[:, :, 1:] |= grown[:, :, :-1]
        rows[:, :, :-1] |= grown[:, :, 1:]
        d[rows & ~reached] = r
        reached = rows
    return d


def band_buckets_host(d, widths):
    """the bucket of every distance: the number of widths[i] <= d, so that bucket k < K holds widths[k - 1] <= d < widths[k] and bucket K the rest"""
    ws = band_widths(widths)
    return np.searchsorted(np.asarray(ws, np.int64), np.asarray(d, np.int64), side="right")


def band_hist_host(labels, out_h, out_w, gt, ncls, widths):
    """The specification of accel_labels_band_hist: (K + 1) x ncls x ncls uint64 BUCKETS.  `labels` is [n x] H x W uint8 with the valid region
    out_h x out_w, `gt` [n x] h x w uint8; with pred = labels_to_source_host(labels, out_h, out_w, h, w) and d = boundary_distance_host(gt, widths[-1]),
    a source pixel adds 1 to [bucket(d)][gt][pred] when gt < ncls and pred < ncls.  The band of width widths[k] is the sum of the buckets 0 .. k
    (band_cumulative); the sum of all K + 1 is the whole-frame confusion matrix."""
    ws = band_widths(widths)
    ncls = int(ncls)
    if not 1 <= ncls <= 32:
        raise ValueError("ncls = %d, must be in 1 .. 32" % ncls)
    g = _u8_batch(gt, "gt")
    a = _u8_batch(labels, "labels")
    if a.shape[0] != g.shape[0]:
        raise ValueError("%d label maps but %d ground-truth maps" % (a.shape[0], g.shape[0]))
    pred = labels_to_source_host(a, out_h, out_w, g.shape[1], g.shape[2])
    bucket = band_buckets_host(boundary_distance_host(g, ws[-1]), ws)
    ok = (g < ncls) & (pred < ncls)
    at = (bucket[ok] * ncls + g[ok].astype(np.int64)) * ncls + pred[ok].astype(np.int64)
    return np.bincount(at, minlength=(len(ws) + 1) * ncls * ncls).astype(np.uint64).reshape(len(ws) + 1, ncls, ncls)


def band_cumulative(buckets):
    """(K + 1) x ncls x ncls buckets -> the same shape, int64: [k] is the band of width widths[k] (the sum of the buckets 0 .. k), [K] the whole frame"""
    return np.cumsum(np.asarray(buckets).astype(np.int64), axis=0)
