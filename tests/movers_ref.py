"""float64 restatements of the bandwidth-bound kernels (csrc/misc.hip) and the inputs of their operator suite
(test_movers_ref_cpu.py checks both against the oracle, test_movers_gpu.py runs them on the device).  Activations are NHWC
(N, H, W, C) as the kernels hold them, image inputs NCHW.  Every function returns the exact value; where a tolerance is needed it
also returns S, the same expression evaluated on |operands|.  No tests in here."""
import numpy as np

from plan_helpers import pair

U = 2.0 ** -24          # unit roundoff of fp32

# what a dcn_cols tap did (bit flags of the branch record)
OUT_TOP, OUT_BOTTOM, OUT_LEFT, OUT_RIGHT, ON_H0, ON_W0, CLAMP_H, CLAMP_W, INTERIOR = 1, 2, 4, 8, 16, 32, 64, 128, 256
BRANCHES = (("outside above", OUT_TOP), ("outside below", OUT_BOTTOM), ("outside left", OUT_LEFT), ("outside right", OUT_RIGHT),
            ("h_im == 0", ON_H0), ("w_im == 0", ON_W0), ("clamp in h", CLAMP_H), ("clamp in w", CLAMP_W), ("interior fractional", INTERIOR))


def f64(a):
    return np.asarray(a, np.float64)


# ---- warp -------------------------------------------------------------------------------------------------------------------------
def warp_coords(flow):
    """sampling position (x + fx, y + fy) of every output pixel: the GridGenerator round trip is the identity in exact arithmetic"""
    flow = f64(flow)
    N, H, W, _ = flow.shape
    return flow[..., 0] + np.arange(W).reshape(1, 1, W), flow[..., 1] + np.arange(H).reshape(1, H, 1)


def warp64(feat, flow):
    """bilinear sample of feat (N, H, W, C) at (x + fx, y + fy), flow (N, H, W, 2) = (fx, fy); taps outside the map are zero"""
    feat = f64(feat)
    N, H, W, C = feat.shape
    xr, yr = warp_coords(flow)
    tx, ty = np.floor(xr), np.floor(yr)
    wx, wy = 1.0 - (xr - tx), 1.0 - (yr - ty)
    tx, ty = tx.astype(np.int64), ty.astype(np.int64)
    n = np.arange(N).reshape(N, 1, 1)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        v = feat[n, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return np.where(ok[..., None], v, 0.0)

    return (tap(ty, tx) * (wy * wx)[..., None] + tap(ty, tx + 1) * (wy * (1 - wx))[..., None]
            + tap(ty + 1, tx) * ((1 - wy) * wx)[..., None] + tap(ty + 1, tx + 1) * ((1 - wy) * (1 - wx))[..., None])


def warp_bound(feat, flow):
    """(N, H, W, 1) bound of an fp32 evaluation of warp64 at general sizes: the function is continuous and piecewise bilinear with
    slope at most 2 max|feat| per axis (zero padding), the fp32 coordinate carries a few roundings at magnitude max(|x + fx|, W - 1),
    and the weights, products and sums on values below max|feat| add 2^-22 max|feat|"""
    N, H, W, _ = np.shape(flow)
    xr, yr = warp_coords(flow)
    m = float(np.abs(feat).max())
    return (U * (np.maximum(np.abs(xr), W - 1) + np.maximum(np.abs(yr), H - 1)) * 2 * m + 4 * U * m)[..., None]


# ---- deformable im2col ------------------------------------------------------------------------------------------------------------
def conv_out(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def dcn_cols64(x, off, k, s, p, d, dg, grp=None):
    """DCN-v1 sampling (misc.hip dcn_cols_body): x (N, H, W, C), off (N, Ho, Wo, dg * 2 * taps) with (dy, dx) of tap t = i kw + j of
    group g at channels g * 2 taps + 2 t; k, s, p, d each an int or an (h, w) pair; a tap is zero unless 0 <= h_im < H and
    0 <= w_im < W; floor(h) >= height - 1 (relative to the window's first row) clamps both rows to the last one and drops the fraction,
    likewise in w.  grp: deformable group of every channel of x (default: C / dg consecutive channels per group).  Returns col
    (N, Ho, Wo, taps, C), S, and the branch record (N, Ho, Wo, dg, taps) of flags above."""
    x, off = f64(x), f64(off)
    N, H, W, C = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    taps = kh * kw
    Ho, Wo = conv_out(H, kh, sh, ph, dh), conv_out(W, kw, sw, pw, dw)
    grp = np.arange(C) // (C // dg) if grp is None else np.asarray(grp)
    off = off.reshape(N, Ho, Wo, dg, taps, 2)
    oh, ow = off[..., 0], off[..., 1]
    i, j = (np.arange(taps) // kw).reshape(1, 1, 1, 1, taps), (np.arange(taps) % kw).reshape(1, 1, 1, 1, taps)
    h_in, w_in = (np.arange(Ho) * sh - ph).reshape(1, Ho, 1, 1, 1), (np.arange(Wo) * sw - pw).reshape(1, 1, Wo, 1, 1)
    h_im, w_im = h_in + i * dh + oh, w_in + j * dw + ow
    inside = (h_im >= 0) & (w_im >= 0) & (h_im < H) & (w_im < W)

    def axis(rel, size):           # rel: coordinate relative to the window start, size: rows (columns) from there to the border
        low = np.floor(rel)
        cl = low >= size - 1
        low = np.where(cl, size - 1, low)
        rel = np.where(cl, low, rel)
        high = np.where(cl, low, low + 1)
        return low.astype(np.int64), high.astype(np.int64), rel - low, cl

    h_low, h_high, lh, ch = axis(i * dh + oh, H - h_in)
    w_low, w_high, lw, cw = axis(j * dw + ow, W - w_in)
    hh, hw = 1 - lh, 1 - lw
    y0, y1 = np.clip(h_in + h_low, 0, H - 1), np.clip(h_in + h_high, 0, H - 1)
    x0, x1 = np.clip(w_in + w_low, 0, W - 1), np.clip(w_in + w_high, 0, W - 1)
    n = np.arange(N).reshape(N, 1, 1, 1, 1)
    flat = lambda yy, xx: (n * H + yy) * W + xx                                 # pixel index into x as (N H W, C)
    corners = ((hh * hw, flat(y0, x0)), (hh * lw, flat(y0, x1)), (lh * hw, flat(y1, x0)), (lh * lw, flat(y1, x1)))
    xt = np.ascontiguousarray(np.moveaxis(x, 3, 0)).reshape(C, N * H * W)
    col, S = np.zeros((C, N, Ho, Wo, taps)), np.zeros((C, N, Ho, Wo, taps))        # channels first: long contiguous runs
    for g in range(dg):
        cs = np.flatnonzero(grp == g)
        acc, acc_abs = 0.0, 0.0
        for wgt, at in corners:
            v = np.take(xt[cs], at[:, :, :, g], axis=1)                     # (channels of the group, N, Ho, Wo, taps)
            acc = acc + wgt[:, :, :, g] * v
            acc_abs = acc_abs + wgt[:, :, :, g] * np.abs(v)
        col[cs] = np.where(inside[:, :, :, g], acc, 0.0)
        S[cs] = np.where(inside[:, :, :, g], acc_abs, 0.0)
    col, S = np.ascontiguousarray(np.moveaxis(col, 0, 4)), np.ascontiguousarray(np.moveaxis(S, 0, 4))
    rec = ((h_im < 0) * OUT_TOP + (h_im >= H) * OUT_BOTTOM + (w_im < 0) * OUT_LEFT + (w_im >= W) * OUT_RIGHT
           + inside * ((h_im == 0) * ON_H0 + (w_im == 0) * ON_W0 + ch * CLAMP_H + cw * CLAMP_W
                       + (~ch & ~cw & ((lh > 0) | (lw > 0))) * INTERIOR))
    return col, S, rec.astype(np.int64)


# ---- pooling, BatchNorm -----------------------------------------------------------------------------------------------------------
def pool_out(n, k, s, p, full):
    return 1 + (-(-(n + 2 * p - k) // s) if full else (n + 2 * p - k) // s)


def pool64(x, kind, k, s, p, full):
    """mx.symbol.Pooling on (N, H, W, C): max ignores the padding; avg divides by the window's area clipped to [-p, size + p);
    k, s, p each an int or an (h, w) pair"""
    x = f64(x)
    N, H, W, C = x.shape
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(s), pair(p)
    Ho, Wo = pool_out(H, kh, sh, ph, full), pool_out(W, kw, sw, pw, full)
    out, S = np.zeros((N, Ho, Wo, C)), np.zeros((N, Ho, Wo, C))
    for oy in range(Ho):
        for ox in range(Wo):
            hs, ws = oy * sh - ph, ox * sw - pw
            he, we = min(hs + kh, H + ph), min(ws + kw, W + pw)
            area = (he - hs) * (we - ws)
            win = x[:, max(hs, 0):min(he, H), max(ws, 0):min(we, W)].reshape(N, -1, C)
            if kind == "max":
                out[:, oy, ox] = win.max(axis=1)
                S[:, oy, ox] = np.abs(out[:, oy, ox])
            else:
                out[:, oy, ox] = win.sum(axis=1) / area
                S[:, oy, ox] = np.abs(win).sum(axis=1) / area
    return out, S


def bn64(gamma, beta, mean, var, eps, fix_gamma):
    """inference BatchNorm as scale and shift: out = v * scale + shift"""
    g = np.ones_like(f64(beta)) if fix_gamma else f64(gamma)
    scale = g / np.sqrt(f64(var) + float(eps))
    return scale, f64(beta) - f64(mean) * scale


def bn_apply64(v, gamma, beta, mean, var, eps, fix_gamma, relu):
    """v * scale + shift (channels last), optional ReLU, and S = |v scale| + |beta| + |mean scale|"""
    scale, shift = bn64(gamma, beta, mean, var, eps, fix_gamma)
    out = f64(v) * scale + shift
    S = np.abs(f64(v) * scale) + np.abs(f64(beta)) + np.abs(f64(mean) * scale)
    return (np.maximum(out, 0.0) if relu else out), S


# ---- image inputs -----------------------------------------------------------------------------------------------------------------
def prep_rgb64(img, bn=None):
    """(N, 3, H, W) -> NHWC4 with a zero fourth channel; bn: (gamma, beta, mean, var, eps, fix_gamma) of bn_data"""
    v = f64(img).transpose(0, 2, 3, 1)
    S = np.abs(v)
    if bn is not None:
        v, S = bn_apply64(v, *bn, relu=False)
    pad = np.zeros(v.shape[:3] + (1,))
    return np.concatenate([v, pad], axis=3), np.concatenate([S, pad], axis=3)


def prep_flow64(cur, prev):
    """Concat(cur / 255, prev / 255) -> avg pool 2x2/2: (N, 3, H, W) twice -> (N, H/2, W/2, 8), channels 6 and 7 zero"""
    v = np.concatenate([f64(cur), f64(prev)], axis=1).transpose(0, 2, 3, 1)
    N, H, W, _ = v.shape
    q = lambda a: a.reshape(N, H // 2, 2, W // 2, 2, 6).sum(axis=(2, 4)) / 1020.0
    pad = np.zeros((N, H // 2, W // 2, 2))
    return np.concatenate([q(v), pad], axis=3), np.concatenate([q(np.abs(v)), pad], axis=3)


# ---- score tail -------------------------------------------------------------------------------------------------------------------
def upsample64(s, w, H, W):
    """Deconvolution 32x32 / stride 16 / group = classes (no kernel flip: out[16 i + ky] += s[i] w[ky]) + Crop(8, 8) to H x W:
    s (N, Hs, Ws, ncls), w (ncls, 1, 32, 32) -> (N, ncls, H, W)"""
    s, w = f64(s), f64(w).reshape(-1, 32, 32)
    N, Hs, Ws, n = s.shape
    full = np.zeros((N, n, 16 * (Hs - 1) + 32, 16 * (Ws - 1) + 32))
    for i in range(Hs):
        for j in range(Ws):
            full[:, :, 16 * i:16 * i + 32, 16 * j:16 * j + 32] += s[:, i, j, :, None, None] * w[None]
    return full[:, :, 8:8 + H, 8:8 + W]


def tail64(left, wl, right=None, wr=None, cw=None, cb=None):
    """score tail: the upsampled left map, or with a second head (its own map size, one row / column larger at the most) the 1x1
    `correction` over Concat(up(left), up(right)) plus its bias.  Returns the logits (N, ncls, 16 Hs, 16 Ws) and S per logit,
    S = |cb| + sum |cw| sum |w s| -- the same whether the correction runs before or after the upsampling."""
    N, Hs, Ws, n = np.shape(left)
    H, W = 16 * Hs, 16 * Ws
    a, A = upsample64(left, wl, H, W), upsample64(np.abs(left), np.abs(wl), H, W)
    if right is None:
        return a, A
    b, B = upsample64(right, wr, H, W), upsample64(np.abs(right), np.abs(wr), H, W)
    cw, cb = f64(cw).reshape(n, 2 * n), f64(cb)
    lg = np.einsum('kc,nchw->nkhw', cw, np.concatenate([a, b], axis=1)) + cb.reshape(1, n, 1, 1)
    S = np.einsum('kc,nchw->nkhw', np.abs(cw), np.concatenate([A, B], axis=1)) + np.abs(cb).reshape(1, n, 1, 1)
    return lg, S


def softmax64(logits):
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def argmax_first(x):
    return np.argmax(x, axis=1).astype(np.uint8)       # numpy returns the first maximum


# ---- inputs of the suite ----------------------------------------------------------------------------------------------------------
def dyadic(rng, shape, step, lo, hi):
    """multiples of `step` in [lo, hi]"""
    return rng.integers(int(round(lo / step)), int(round(hi / step)) + 1, shape) * float(step)


def gauss(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


WARP_EXACT_SIZES = ((5, 9), (9, 17), (17, 33))          # H - 1 and W - 1 powers of two: the grid round trip is exact
WARP_EXACT_C = (4, 24, 68)
WARP_TARGETS = lambda n: (-1.0, 0.0, n - 1.0, float(n), -2.5, n + 1.25)     # landing exactly on the edges of the support; beyond a side by > 1


def warp_exact_inputs(H, W, C, N=3, seed=0):
    """features on multiples of 1/4 in [-8, 8], flows on multiples of 1/8: every coordinate, weight, product and sum of the warp is
    exact in fp32.  Every third pixel has its x and y sampling position planted on one of WARP_TARGETS (cycling through all pairs)."""
    rng = np.random.default_rng(1000 + seed + 7 * H + W + 131 * C)
    feat = dyadic(rng, (N, H, W, C), 0.25, -8, 8)
    flow = dyadic(rng, (N, H, W, 2), 0.125, -2.5, 2.5)
    tx, ty = WARP_TARGETS(W), WARP_TARGETS(H)
    t = 0
    for n in range(N):
        for pix in range(n, H * W, 3):
            y, x = divmod(pix, W)
            flow[n, y, x] = (tx[t % 6] - x, ty[(t // 6 + t) % 6] - y)
            t += 1
    bias = dyadic(rng, (C,), 0.25, -4, 4)
    return feat.astype(np.float32), flow.astype(np.float32), bias.astype(np.float32)


def warp_landings(flow):
    """how many sampling positions land exactly on each of the first four WARP_TARGETS / beyond each side by more than a pixel"""
    N, H, W, _ = flow.shape
    xr, yr = warp_coords(flow)
    out = {}
    for name, r, n in (("x", xr, W), ("y", yr, H)):
        for v in WARP_TARGETS(n)[:4]:
            out["%s_real == %g" % (name, v)] = int((r == v).sum())
        out["%s below -1" % name] = int((r < -1).sum())
        out["%s above %d" % (name, n)] = int((r > n).sum())
    return out


WARP_BOUNDED = [(H, W, mag) for (H, W) in ((12, 20), (13, 23)) for mag in (0.7, 3.0, 40.0)]


def warp_bounded_inputs(H, W, mag, C=20, N=3):
    seed = 2000 + 31 * H + W + int(mag * 10)
    return gauss(seed, N, H, W, C), gauss(seed + 1, N, H, W, 2, scale=mag), gauss(seed + 2, C)


# (k, s, p, d, dg, C, H, W, seed): the 3x3 cases launch ceil(Ho Wo C / 4 / 256) = 1, 2, 7, 8, 9, 13 blocks per kernel row (the XCD
# swizzle of dcn_cols9 below, at and off a multiple of 8); the 1x1 and 5x5 windows take the one-tap-per-thread kernel
DCN_CASES = [
    (3, 1, 1, 1, 1, 16, 7, 9, 0),
    (3, 1, 2, 2, 4, 32, 7, 9, 0),
    (3, 2, 1, 1, 1, 16, 39, 41, 0),
    (3, 1, 1, 1, 1, 32, 15, 17, 0),
    (3, 1, 2, 2, 4, 16, 23, 25, 0),
    (3, 2, 1, 1, 1, 32, 37, 41, 0),
    (1, 1, 0, 1, 2, 16, 7, 9, 0),
    (5, 1, 2, 1, 1, 32, 9, 11, 0),
]
DCN_BLOCKS = {0: 1, 1: 2, 2: 7, 3: 8, 4: 9, 5: 13}       # case index -> gridDim.x of the 3x3 kernel
DCN_MIN_TAPS = 8                                          # every branch is taken by at least this many taps of every case


def dcn_blocks(case):
    k, s, p, d, dg, C, H, W, _ = case
    return -(-(conv_out(H, k, s, p, d) * conv_out(W, k, s, p, d) * (C // 4)) // 256)


def dcn_offsets(rng, shape):
    """multiples of 1/8 in [-2, 2]; two in five are whole numbers, which is what lands taps exactly on row / column 0 and in the
    clamp branch often enough at the smallest maps"""
    whole = rng.random(shape) < 0.4
    return np.where(whole, dyadic(rng, shape, 1.0, -2, 2), dyadic(rng, shape, 0.125, -2, 2))


def dcn_inputs(case, N=3, gaussian=False):
    k, s, p, d, dg, C, H, W, seed = case
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    rng = np.random.default_rng(3000 + seed + 17 * H + W + 5 * C + (k if np.ndim(k) == 0 else 100 * kh + 10 * kw) + 3 * dg)
    Ho, Wo = conv_out(H, kh, sh, ph, dh), conv_out(W, kw, sw, pw, dw)
    x = rng.standard_normal((N, H, W, C)) if gaussian else dyadic(rng, (N, H, W, C), 0.25, -8, 8)
    off = dcn_offsets(rng, (N, Ho, Wo, dg * 2 * kh * kw))
    return x.astype(np.float32), off.astype(np.float32)


# the generic kernels on unequal pairs: (k, s, p, d, dg, C, H, W, seed), all through dcn_cols_kernel (launch_dcn_cols takes the
# three-taps-per-thread kernel for kh == kw == 3 alone)
DCN_PAIR_CASES = [
    ((1, 3), 1, (0, 2), (1, 2), 1, 16, 7, 9, 0),
    ((1, 3), 1, (0, 2), (1, 2), 2, 16, 7, 9, 0),
    ((3, 1), 1, (0, 2), (1, 2), 1, 16, 7, 9, 0),
    ((3, 1), 1, (0, 2), (1, 2), 2, 32, 7, 9, 0),
]
# (kind, k, s, p, full): through pool_kernel (launch_pool takes the nine-loads kernel for max 3x3 / 2 alone)
# (on the 13 x 19 map both conventions keep the same windows at these strides)
POOL_PAIR_CASES = [("max", (3, 2), (2, 1), (1, 0), False), ("max", (2, 3), (1, 2), (0, 1), False),
                   ("avg", (3, 2), (2, 1), (1, 0), False), ("avg", (2, 3), (1, 2), (0, 1), True)]


def pool_dyadic_inputs(C, N=3, seed=0):
    """multiples of 1/4 in [-8, 8]: window sums are exact in fp32, and so is the division by a window of 1, 2 or 4 elements; the
    division by 3 or 6 rounds once"""
    H, W = POOL_HW
    return dyadic(np.random.default_rng(4200 + seed + C), (N, H, W, C), 0.25, -8, 8).astype(np.float32)


def branch_counts(rec):
    return {name: int(((rec & flag) != 0).sum()) for name, flag in BRANCHES}


# the streaming-store instantiation: the smallest column buffer beyond 256 MB
BIG_DCN = dict(k=3, s=1, p=1, d=1, dg=16, C=512, H=128, W=128)
BIG_DCN_CHANNELS = np.array([16 * i + (5 * i) % 16 for i in range(32)])      # one of every 16 channels, two per deformable group


def big_dcn_inputs():
    rng = np.random.default_rng(3999)
    c = BIG_DCN
    x = dyadic(rng, (1, c["H"], c["W"], c["C"]), 0.25, -8, 8).astype(np.float32)
    off = dcn_offsets(rng, (1, c["H"], c["W"], c["dg"] * 18)).astype(np.float32)
    return x, off


POOL_MAX_CASES = [("max", 3, 2, 0, True), ("max", 3, 2, 1, False), ("max", 2, 2, 0, False)]     # kind, k, s, p, full
POOL_C = (20, 18)
POOL_HW = (13, 19)


def pool_inputs(C, N=3, seed=0):
    H, W = POOL_HW
    return gauss(4000 + seed + C, N, H, W, C)


def bn_inputs(C, seed=0):
    rng = np.random.default_rng(4100 + seed + C)
    return dict(gamma=rng.uniform(0.5, 1.5, C).astype(np.float32) * np.where(rng.random(C) < 0.5, -1, 1).astype(np.float32),
                beta=rng.standard_normal(C).astype(np.float32), mean=rng.standard_normal(C).astype(np.float32),
                var=rng.uniform(0.5, 2.0, C).astype(np.float32))


PREP_RGB_HW = (13, 23)          # 299 pixels: two blocks, the second ragged
PREP_FLOW_HW = (34, 38)         # 17 x 19 = 323 outputs


def image_inputs(H, W, N=3, seed=0):
    return gauss(5000 + seed, N, 3, H, W, scale=60.0), gauss(5001 + seed, N, 3, H, W, scale=60.0)


# score tail: name -> (ncls, N, left map, right map or None, uniform filters, plan options)
TAIL_CASES = {
    "two_heads_per_class": (19, 3, (3, 5), (3, 5), False, ""),
    "two_heads_uniform_lowres": (19, 3, (3, 5), (3, 5), True, ""),
    "two_heads_uniform_general": (19, 3, (3, 5), (3, 5), True, "lowres=0"),
    "one_head_uniform": (19, 3, (3, 5), None, True, ""),
    "one_head_uniform_general": (19, 3, (3, 5), None, True, "lowres=0"),
    "one_head_per_class": (19, 3, (3, 5), None, False, ""),
    "right_4x6": (19, 3, (3, 5), (4, 6), False, ""),
    "right_4x5": (19, 3, (3, 5), (4, 5), True, ""),
    "right_3x6": (19, 3, (3, 5), (3, 6), False, ""),
    "ncls2_lowres": (2, 3, (3, 5), (3, 5), True, ""),
    "ncls2_per_class": (2, 3, (3, 5), (3, 5), False, ""),
    "ncls2_one_head": (2, 3, (3, 5), None, True, ""),
    "ncls21_lowres": (21, 3, (3, 5), (3, 5), True, ""),
    "ncls21_per_class": (21, 3, (3, 5), (4, 6), False, ""),
    "ncls21_one_head": (21, 3, (3, 5), None, False, ""),
    "softmax_two_heads": (19, 3, (3, 5), (3, 5), False, "softmax=1"),
    "softmax_lowres": (19, 3, (3, 5), (3, 5), True, "softmax=1"),
    "softmax_one_head": (21, 3, (3, 5), None, False, "softmax=1"),
    "softmax_ncls2": (2, 3, (3, 5), (4, 6), False, "softmax=1"),
}


# exact ties at the maximum: classes TIE_CLASSES computed by identical arithmetic, the first must win
TIE_CLASSES = (3, 7)
TIE_CASES = {
    "ties_one_head_uniform": (19, 3, (3, 5), None, True, ""),
    "ties_one_head_general": (19, 3, (3, 5), None, True, "lowres=0"),
    "ties_two_heads_lowres": (19, 3, (3, 5), (3, 5), True, ""),
    "ties_two_heads_general": (19, 3, (3, 5), (3, 5), False, ""),
    "ties_softmax": (19, 3, (3, 5), (4, 6), False, "softmax=1"),
}
ALL_TAIL = dict(TAIL_CASES, **TIE_CASES)
# softmax cases: scores large enough for logits beyond 89, where expf overflows unless the maximum is subtracted first
TAIL_SCALE = {"softmax_two_heads": 40.0, "softmax_lowres": 40.0, "softmax_one_head": 40.0, "softmax_ncls2": 200.0, "ties_softmax": 40.0}


def bilinear32():
    """the frozen initialisation of the 32x32 / 16 upsampling filters (one filter for every class)"""
    f, c = 16.0, 15.5
    a = 1 - np.abs(np.arange(32) - c) / f
    return np.outer(a, a).astype(np.float32)


def tail_inputs(name):
    ncls, N, (Hs, Ws), right, uniform, _ = ALL_TAIL[name]
    seed, scale = 6000 + sorted(ALL_TAIL).index(name) * 10, TAIL_SCALE.get(name, 3.0)
    left = gauss(seed, N, Hs, Ws, ncls, scale=scale)
    if uniform:
        wl = wr = np.broadcast_to(bilinear32(), (ncls, 1, 32, 32)).copy()
    else:
        wl, wr = gauss(seed + 1, ncls, 1, 32, 32, scale=0.2), gauss(seed + 2, ncls, 1, 32, 32, scale=0.2)
    d = dict(left=left, wl=wl)
    if right is not None:
        d.update(right=gauss(seed + 3, N, right[0], right[1], ncls, scale=scale), wr=wr,
                 cw=gauss(seed + 4, ncls, 2 * ncls, 1, 1, scale=0.3), cb=gauss(seed + 5, ncls))
    if name in TIE_CASES:
        a, c = TIE_CLASSES
        if right is None:        # the same scores (the largest of their pixel at every other pixel) through the same filter
            left[..., a] = np.where((np.arange(Hs * Ws).reshape(Hs, Ws) % 2) == 0, np.abs(left).max(axis=3) + 1, left[..., a])
            left[..., c] = left[..., a]
            wl[c] = wl[a]
        else:                    # the same correction row and bias
            d["cw"][c] = d["cw"][a]
            d["cb"][a] = d["cb"][c] = np.abs(d["cb"]).max() + np.float32(2.0 if scale == 3.0 else 30.0)
    return d


def tail_bound(ncls, S):
    """4 upsampling taps, 2 ncls correction terms and the bias, in either order: at most 2 ncls + 5 roundings on top of one another"""
    return (2 * ncls + 8) * U * S
