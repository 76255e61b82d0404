"""Hand-written plans for the operator tests: NHWC views of the arena, a builder of plan text (import_nchw -> convolutions -> export_nchw
with every launch geometry forced) and a float64 convolution.  No tests in here."""
import numpy as np

al = lambda b: (b + 255) // 256 * 256
r4 = lambda c: (c + 3) // 4 * 4
bits = lambda v: int(np.float32(v).view(np.uint32)) & 0x7FFFFFFF


class V(object):
    """an NHWC view of the arena: offset, channels, channel stride, H, W, images"""

    def __init__(self, off, C, Cs, H, W, N, space="A"):
        self.off, self.C, self.Cs, self.H, self.W, self.N, self.space = off, C, Cs, H, W, N, space

    def ref(self):
        return "%s:%d:%d:%d:%d:%d:%d" % (self.space, self.off, self.C, self.Cs, self.H, self.W, self.N)

    def sub(self, c0, C):
        return V(self.off + 4 * c0, C, self.Cs, self.H, self.W, self.N, self.space)


class Builder(object):
    def __init__(self, N):
        self.N, self.arena, self.head, self.lines, self.params = N, 0, [], [], {}
        self.inputs, self.outputs, self.readers = {}, {}, []

    def buf(self, C, H, W, Cs=None):
        v = V(self.arena, C, Cs or r4(C), H, W, self.N)
        self.arena += al(self.N * H * W * v.Cs * 4)
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
        return "\n".join(["option tune=0", "arena bytes=%d" % max(self.arena, 256)] + self.head + self.lines) + "\n"


def conv64(x, w, s=1, p=0, d=1):
    """float64 NCHW convolution, zero padding"""
    N, C, H, W = x.shape
    K, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * p - d * (kh - 1) - 1) // s + 1, (W + 2 * p - d * (kw - 1) - 1) // s + 1
    xp = np.zeros((N, C, H + 2 * p, W + 2 * p)); xp[:, :, p:p + H, p:p + W] = x
    out = np.zeros((N, K, Ho, Wo))
    for ky in range(kh):
        for kx in range(kw):
            out += np.einsum('kc,nchw->nkhw', w[:, :, ky, kx].astype(np.float64),
                             xp[:, :, ky * d:ky * d + s * (Ho - 1) + 1:s, kx * d:kx * d + s * (Wo - 1) + 1:s])
    return out
