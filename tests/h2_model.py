"""The arithmetic of the fp16x2 form (kernels.h ConvParams::wh2r; csrc/range.h) restated in numpy.  No tests in here:
tests/test_h2_model_cpu.py holds the form's claims against this model, tests/test_h2_octaves_gpu.py holds the kernels against it.

Everything is float64 on values that are exact halves, so a product of two terms (22 significant bits) and a sum of a few thousand of
them are exact here: what separates a kernel from this model is its fp32 accumulation alone.

  pixels   s = range_scale(bits of the largest |pixel| of the tensor)            range.h
           hi = half(v * s), lo = half(fma(v, s, -hi))                          conv_b3r.hip store_a, conv_halo.hip, conv_stem_b3.hip
  weights  q[row] = 15 - frexp_exponent(largest |w| of the output channel)      accel_hip.cpp pack_h2r (all parity classes of a
           hi = half(w * 2^q), lo = half(w * 2^q - hi)                          deconvolution together), conv_stem_b3_pack_h2
  product  hi * hi + hi * lo + lo * hi, summed, times 2^-q / s                  conv_b3r.hip mma; the epilogue's scale_h2 * xinv

flush_subnormals=True zeroes every half term below 2^-14: what a conversion or a matrix unit that flushed half subnormals would leave.
The Winograd kernels split V = B^T d B at s / 4 and U = G g G^T per output channel: they have no exact model here; a direct evaluation
at s / 4 is their yardstick."""
import numpy as np

TOP_EXP = 14            # range.h RANGE_TOP_EXP: the largest pixel lands in [2^13, 2^14)
W_TOP_EXP = 15          # pack_h2r: the largest weight of an output channel lands in [2^14, 2^15)
HALF_MIN_NORMAL = 2.0 ** -14


def half(x, flush_subnormals=False):
    """x (float64) rounded to the nearest half, returned as float64"""
    h = np.asarray(x, np.float64).astype(np.float16).astype(np.float64)
    if flush_subnormals:
        h = np.where(np.abs(h) < HALF_MIN_NORMAL, 0.0, h)
    return h


def float_bits(v):
    return int(np.float32(abs(float(v))).view(np.uint32))


def range_scale(bits):
    """range.h range_scale: the power of two s with s * largest in [2^13, 2^14), its exponent clamped to +-100; an all-zero tensor: 1"""
    e = (126 + TOP_EXP) - ((int(bits) >> 23) & 0xFF)
    e = min(max(e, -100), 100)
    if not bits:
        e = 0
    return 2.0 ** e


def split_pixels(x, s, flush_subnormals=False):
    """(hi, lo) of x * s.  v * s is exact in fp32 (s is a power of two, nothing near the ends of the fp32 range) and so is the
    residual: one rounding to half each"""
    v = np.asarray(x, np.float32).astype(np.float64) * float(s)
    hi = half(v, flush_subnormals)
    return hi, half(v - hi, flush_subnormals)


def weight_exponents(w, cout_axis=0):
    """q per output channel: 15 - frexp_exponent(largest |w| of the channel); 0 for an all-zero channel"""
    w = np.asarray(w, np.float32)
    amax = np.abs(np.moveaxis(w, cout_axis, 0).reshape(w.shape[cout_axis], -1)).max(axis=1)
    q = W_TOP_EXP - np.frexp(amax)[1]
    return np.where(amax > 0, q, 0).astype(np.int64)


def split_weights(w, q=None, cout_axis=0, flush_subnormals=False):
    """(hi, lo, q) of w * 2^q[output channel]"""
    w = np.asarray(w, np.float32)
    if q is None:
        q = weight_exponents(w, cout_axis)
    shape = [1] * w.ndim
    shape[cout_axis] = -1
    v = w.astype(np.float64) * 2.0 ** np.asarray(q, np.float64).reshape(shape)
    hi = half(v, flush_subnormals)
    return hi, half(v - hi, flush_subnormals), q


def kept_products(xh, xl, wh, wl, mul=np.multiply):
    """the three products the kernels keep (lo * lo is dropped); `mul`: any bilinear map of a pixel and a weight array"""
    return mul(xh, wh) + mul(xh, wl) + mul(xl, wh)


def conv(x, w, s, conv64, cout_axis=0, flush_subnormals=False):
    """The fp16x2 form of conv64(x, w) at pixel scale s, in float64.  conv64(x, w) -> (N, Cout, Ho, Wo): any float64 convolution,
    linear in both arguments (it must not round its arguments: pass float64 arrays through)."""
    xh, xl = split_pixels(x, s, flush_subnormals)
    wh, wl, q = split_weights(w, None, cout_axis, flush_subnormals)
    acc = kept_products(xh, xl, wh, wl, conv64)
    return acc * (2.0 ** -q.astype(np.float64))[None, :, None, None] / float(s)


def split_error_bound(m, top_exp=TOP_EXP, flush_subnormals=False):
    """Bound of |hi + lo - v| / |v| for a scaled value v in [2^(top_exp - 1 - m), 2^(top_exp - m)): m octaves below the window
    the tensor's largest value is put into.
    hi keeps 11 bits, the residual is at most half a unit of hi's last place, 2^(top_exp - 12 - m); lo keeps 11 bits of it (its error
    is at most 2^(top_exp - 24 - m): 2^-23 of v) unless its unit falls below the half subnormals' 2^-24 (error at most 2^-25).
    Flushed: a residual below 2^-14 is lost whole."""
    lo_max = 2.0 ** (top_exp - 12 - m)
    v_min = 2.0 ** (top_exp - 1 - m)
    if flush_subnormals:
        if v_min < HALF_MIN_NORMAL:
            return 1.0
        return max(2.0 ** -23, min(lo_max, HALF_MIN_NORMAL) / v_min)
    if v_min < 2.0 ** -24:
        return 1.0
    return max(2.0 ** -23, 2.0 ** -25 / v_min)
