"""Hand-written plans for the operator tests: NHWC views of the arena, a builder of plan text (import_nchw -> convolutions -> export_nchw
with every launch geometry forced; or the byte movers of csrc/misc.hip between sub-views of canvases the host writes and reads raw;
half arena buffers and the reader of their raw bytes),
a float64 convolution and deconvolution, and the BatchNorm constants of the convolution tests.  No tests in here."""
import numpy as np

al = lambda b: (b + 255) // 256 * 256
r4 = lambda c: (c + 3) // 4 * 4
bits = lambda v: int(np.float32(v).view(np.uint32)) & 0x7FFFFFFF


def pair(v):
    """(h, w) of a kernel size, stride, padding or dilation given as an int (both the same) or as a pair"""
    return (int(v),) * 2 if np.ndim(v) == 0 else (int(v[0]), int(v[1]))


class V(object):
    """an NHWC view of the arena: offset, channels, channel stride, H, W, images; half: 2-byte elements (":h"); base: the byte offset
    of the buffer the view lies in (its first pixel's channel 0)"""

    def __init__(self, off, C, Cs, H, W, N, space="A", half=False, base=0):
        self.off, self.C, self.Cs, self.H, self.W, self.N, self.space, self.half, self.base = off, C, Cs, H, W, N, space, half, base

    def ref(self):
        return "%s:%d:%d:%d:%d:%d:%d%s" % (self.space, self.off, self.C, self.Cs, self.H, self.W, self.N, ":h" if self.half else "")

    @property
    def esize(self):
        return 2 if self.half else 4

    def sub(self, c0, C, N=None):
        """channels [c0, c0 + C) of the view's pixels (c0 counts elements: 2 bytes each in a half view), of its first N images"""
        return V(self.off + self.esize * c0, C, self.Cs, self.H, self.W, self.N if N is None else N, self.space, self.half, self.base)

    @property
    def c0(self):
        """first channel of the view inside its buffer's pixel stride (views that start in the buffer's first pixel)"""
        return (self.off - self.base) // self.esize


class Builder(object):
    def __init__(self, N):
        self.N, self.arena, self.head, self.lines, self.params = N, 0, [], [], {}
        self.inputs, self.outputs, self.readers = {}, {}, []
        self.options, self.canvases, self._canary = ["tune=0"], {}, None

    def buf(self, C, H, W, Cs=None):
        v = V(self.arena, C, Cs or r4(C), H, W, self.N)
        self.arena += al(self.N * H * W * v.Cs * 4)
        return v

    def hbuf(self, Cs, H, W, N=None):
        """a HALF arena buffer of N images, as the view of its whole width Cs (Cs % 8 == 0); the host cannot write it: a convolution
        of the plan does, and half_words() reads it back"""
        N = self.N if N is None else N
        v = V(self.arena, Cs, Cs, H, W, N, half=True, base=self.arena)
        self.arena += al(N * H * W * Cs * 2)
        return v

    def inp(self, name, C, H, W, Cs=None, yr=None):
        v = self.buf(C, H, W, Cs)
        self.head.append("pbuf name=%s bytes=%d" % (name, self.N * C * H * W * 4))
        self.lines.append("import_nchw src=%s:0:%d:%d:%d:%d:%d dst=%s%s" % (name, C, C, H, W, self.N, v.ref(), "" if yr is None else " yr=%d" % yr))
        self.inputs[name] = (self.N, C, H, W)
        return v

    def pbuf(self, name, C, H, W, Cs=None):
        """a persistent buffer the host writes (NHWC, channel stride Cs; fed as an (N, H, W, Cs) array)"""
        v = V(0, C, Cs or r4(C), H, W, self.N, space=name)
        self.head.append("pbuf name=%s bytes=%d" % (name, self.N * H * W * v.Cs * 4))
        return v

    def canvas(self, name, Cs, H, W, N=None, tail=64):
        """a persistent buffer the host writes and reads raw (write_canvas / read_canvas) as (N, H, W, Cs) words and `tail` more behind
        them: the operands of the op under test are sub-views of canvases (V.sub: a channel offset, Cs > C), so nothing has to be
        imported or exported.  (import_nchw zero-fills all Cs channels from the view's first one on: it is meant for whole buffers.)"""
        N = self.N if N is None else N
        self.head.append("pbuf name=%s bytes=%d" % (name, (N * H * W * Cs + tail) * 4))
        self.canvases[name] = (N, H, W, Cs, tail)
        return V(0, Cs, Cs, H, W, N, space=name)

    def flat(self, name, words, tail=64):
        """a canvas without a pixel structure (NCHW images, logits, label bytes): `words` 32-bit words and the tail"""
        return self.canvas(name, words, 1, 1, N=1, tail=tail)

    def canary(self, name):
        """what an output canvas holds before a run: a distinct non-zero bit pattern in every word"""
        N, H, W, Cs, tail = self.canvases[name]
        n = N * H * W * Cs + tail
        if self._canary is None or self._canary.size < n:
            self._canary = canary_words(n)
        return self._canary[:n].copy()

    def write_canvas(self, m, name, data=None):
        """data: (N, H, W, Cs) values (the tail stays canary), None: canary everywhere"""
        N, H, W, Cs, tail = self.canvases[name]
        words = self.canary(name)
        if data is not None:
            d = np.ascontiguousarray(data)
            assert d.dtype.itemsize == 4 and d.size == N * H * W * Cs, (name, d.dtype, d.shape)
            words[:d.size] = d.reshape(-1).view(np.uint32)
        m.write(name, words)

    def read_canvas(self, m, name):
        """the canvas as uint32 words: ((N, H, W, Cs), tail)"""
        N, H, W, Cs, tail = self.canvases[name]
        words = m.read(name, (N * H * W * Cs + tail,), np.uint32)
        return words[:N * H * W * Cs].reshape(N, H, W, Cs), words[N * H * W * Cs:]

    def untouched(self, name, words, tail, c0=0, C=0):
        """every word of an output canvas outside channels [c0, c0 + roundup(C, 4)) of every pixel -- the tail included -- still holds
        its canary"""
        N, H, W, Cs, nt = self.canvases[name]
        want = self.canary(name)
        body = want[:N * H * W * Cs].reshape(N, H, W, Cs)
        return np.array_equal(words[..., :c0], body[..., :c0]) and np.array_equal(words[..., c0 + r4(C):], body[..., c0 + r4(C):]) and \
            np.array_equal(tail, want[N * H * W * Cs:])

    # ---- one line per byte mover (csrc/misc.hip) ----
    def warp(self, name, feat, flow, out, out2=None, bias=None):
        self.lines.append("warp name=%s feat=%s flow=%s out=%s%s" % (name, feat.ref(), flow.ref(), out.ref(),
                          "" if out2 is None else " out2=%s bias=%s" % (out2.ref(), bias)))

    def dcn_cols(self, name, x, off, cols, k, s, p, d, dg):
        """k, s, p, d: an int or an (h, w) pair"""
        self.lines.append("dcn_cols name=%s in=%s off=%s out=%s k=%d,%d s=%d,%d p=%d,%d d=%d,%d dg=%d" % (
            (name, x.ref(), off.ref(), cols.ref()) + pair(k) + pair(s) + pair(p) + pair(d) + (dg,)))

    def pool(self, name, x, y, kind, k, s, p, bn=None, eps=2e-5, fixg=0, act=0):
        """k, s, p: an int or an (h, w) pair"""
        self.lines.append("pool name=%s kind=%s k=%d,%d s=%d,%d p=%d,%d in=%s out=%s act=%d%s" % (
            (name, kind) + pair(k) + pair(s) + pair(p) + (x.ref(), y.ref(), act, "" if bn is None else " bn=%s eps=%r fixg=%d" % (bn, eps, fixg))))

    def copy(self, name, src, dst):
        self.lines.append("copy name=%s src=%s dst=%s" % (name, src.ref(), dst.ref()))

    def prep_rgb(self, name, img, dst, H, W, bn=None, eps=2e-5, fixg=1):
        self.lines.append("prep_rgb name=%s src=%s:0:3:3:%d:%d:%d dst=%s H=%d W=%d%s" % (
            name, img, H, W, self.N, dst.ref(), H, W, "" if bn is None else " bn=%s eps=%r fixg=%d" % (bn, eps, fixg)))

    def prep_flow(self, name, cur, prev, dst, H, W):
        self.lines.append("prep_flow name=%s cur=%s:0:3:3:%d:%d:%d prev=%s:0:3:3:%d:%d:%d dst=%s H=%d W=%d" % (
            name, cur, H, W, self.N, prev, H, W, self.N, dst.ref(), H, W))

    def score_tail(self, name, left, logits, labels, ncls, wl, right=None, wr=None, cw=None, cb=None, extra=""):
        H, W = 16 * left.H, 16 * left.W
        self.lines.append("score_tail name=%s left=%s%s wl=%s%s H=%d W=%d ncls=%d logits=%s:0:%d:4:%d:%d:%d labels=%s:0:1:4:%d:%d:%d%s" % (
            name, left.ref(), "" if right is None else " right=%s" % right.ref(), wl,
            "" if right is None else " wr=%s cw=%s cb=%s" % (wr, cw, cb), H, W, ncls, logits, ncls, H, W, self.N, labels, H, W, self.N,
            (" " + extra) if extra else ""))

    def out(self, name, v):
        self.head.append("pbuf name=%s bytes=%d" % (name, self.N * v.C * v.H * v.W * 4))
        self.lines.append("export_nchw src=%s dst=%s:0:%d:%d:%d:%d:%d" % (v.ref(), name, v.C, v.C, v.H, v.W, self.N))
        self.outputs[name] = (self.N, v.C, v.H, v.W)

    def conv(self, name, x, y, w, tile, k=1, s=1, p=0, d=1, act=0, xr=None, yr=None, extra=""):
        self.params[name + "_w"] = w
        self.lines.append("conv name=%s in=%s out=%s w=%s_w act=%d slope=0.1 cin=%d cout=%d mode=conv tile=%d k=%d,%d s=%d,%d p=%d,%d d=%d,%d%s%s%s" % (
            name, x.ref(), y.ref(), name, act, x.C, y.C, tile, k, k, s, s, p, p, d, d,
            "" if xr is None else " xr=%d" % xr, "" if yr is None else " yr=%d" % yr, (" " + extra) if extra else ""))

    def reader(self, name, T, rid, rng, tile=81, K=40, k=1):
        """the fp16x2 reader of T (range id rid) and the export of what it computed"""
        w = (rng.standard_normal((K, T.C, k, k)) / np.sqrt(T.C * k * k)).astype(np.float32)
        y = self.buf(K, T.H, T.W)
        self.conv(name, T, y, w, tile, k=k, p=k // 2, xr=rid, extra="nosplit=1")
        self.out(name + "_y", y)
        self.out(name + "_t", T)
        self.readers.append((name, T, w, tile))

    def text(self):
        return "\n".join(["option " + " ".join(self.options), "arena bytes=%d" % max(self.arena, 256)] + self.head + self.lines) + "\n"


def half_words(arena, v):
    """the half buffer a view v lies in (Builder.hbuf) as (N, H, W, Cs) uint16, from the raw bytes of the arena (Plan.arena())"""
    n = v.N * v.H * v.W * v.Cs * 2
    return arena[v.base:v.base + n].view(np.uint16).reshape(v.N, v.H, v.W, v.Cs)


def canary_words(n):
    """n distinct non-zero 32-bit patterns (an odd multiplier permutes the residues)"""
    return np.arange(1, n + 1, dtype=np.uint32) * np.uint32(2654435761)


def conv64(x, w, s=1, p=0, d=1):
    """float64 NCHW convolution, zero padding; s, p, d: an int or an (h, w) pair"""
    N, C, H, W = x.shape
    K, _, kh, kw = w.shape
    (sh, sw), (ph, pw), (dh, dw) = pair(s), pair(p), pair(d)
    Ho, Wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    xp = np.zeros((N, C, H + 2 * ph, W + 2 * pw)); xp[:, :, ph:ph + H, pw:pw + W] = x
    out = np.zeros((N, K, Ho, Wo))
    for ky in range(kh):
        for kx in range(kw):
            out += np.einsum('kc,nchw->nkhw', w[:, :, ky, kx].astype(np.float64),
                             xp[:, :, ky * dh:ky * dh + sh * (Ho - 1) + 1:sh, kx * dw:kx * dw + sw * (Wo - 1) + 1:sw])
    return out


def deconv64(x, w):
    """float64 Deconvolution 4x4 / stride 2 / pad 1 (NCHW, weights (Cin, Cout, 4, 4)): the full 2h x 2w output; the skip tensor's
    Crop keeps its first rows and columns"""
    N, C, h, w_ = x.shape
    out = np.zeros((N, w.shape[1], 2 * h + 2, 2 * w_ + 2))
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky:ky + 2 * h:2, kx:kx + 2 * w_:2] += np.einsum('ck,nchw->nkhw', w[:, :, ky, kx].astype(np.float64), x)
    return out[:, :, 1:1 + 2 * h, 1:1 + 2 * w_]


def bn_params(rng, name, C, tc, negative=False):
    """BatchNorm constants of mixed sign (scale and shift), small shifts; channel tc's scale is +-1 (negative: -1)"""
    g = rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)
    g[tc] = -1.0 if negative else 1.0
    return {name + "_gamma": g.astype(np.float32), name + "_beta": (rng.standard_normal(C) * 2.0 ** -24).astype(np.float32),
            name + "_moving_mean": (rng.standard_normal(C) * 2.0 ** -24).astype(np.float32),
            name + "_moving_var": np.full(C, 1.0 - 1e-5, np.float32)}
