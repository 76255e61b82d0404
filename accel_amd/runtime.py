"""ctypes binding of libaccel_hip.so (include/accel_hip.h).

The library is the only compute path of accel_amd: there is no CPU fallback.
If it is missing or no MI355X is visible, every call raises AccelError.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACCEL_LIB_PATH") or os.path.join(_HERE, "libaccel_hip.so")      # (override: A/B of two builds)
_lib = None


class AccelError(RuntimeError):
    pass


def build(force=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    stale = force or not os.path.exists(LIB_PATH)
    if not stale:
        t = os.path.getmtime(LIB_PATH)
        for f in os.listdir(src):
            if f.endswith((".hip", ".cpp", ".h")) and os.path.getmtime(os.path.join(src, f)) > t:
                stale = True
        hdr = os.path.join(_HERE, "..", "include", "accel_hip.h")
        if os.path.exists(hdr) and os.path.getmtime(hdr) > t:
            stale = True
    if stale:
        subprocess.check_call(["make", "-C", src, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


class YUVLayout(ctypes.Structure):
    """accel_yuv_layout (include/accel_hip.h): how I420 (0), P010 (1) or YUY2 (2) frames lie in memory, and their colour mode"""
    _fields_ = [("format", ctypes.c_int), ("colour", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int), ("pitch", ctypes.c_size_t),
                ("pitch_c", ctypes.c_size_t), ("u_offset", ctypes.c_size_t), ("v_offset", ctypes.c_size_t), ("frame_bytes", ctypes.c_size_t)]


def _declare(lib):
    c = ctypes
    vp, i, f, sz = c.c_void_p, c.c_int, c.c_float, c.c_size_t
    lib.accel_last_error.restype = c.c_char_p
    lib.accel_version.restype = c.c_char_p
    lib.accel_ctx_stream.restype = vp
    lib.accel_ctx_stream.argtypes = [vp]
    sigs = {
        "accel_ctx_create": [i, c.POINTER(vp)],
        "accel_ctx_destroy": [vp],
        "accel_sync": [vp],
        "accel_model_create": [vp, c.POINTER(vp)],
        "accel_model_destroy": [vp],
        "accel_model_set_param": [vp, c.c_char_p, vp, i, c.POINTER(c.c_int64)],
        "accel_model_has_param": [vp, c.c_char_p],
        "accel_model_add_plan": [vp, c.c_char_p, c.c_char_p, c.POINTER(vp)],
        "accel_plan_op_launch": [vp, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)],
        "accel_plan_op_mode": [vp, c.c_int, c.POINTER(c.c_int)],
        "accel_plan_op_range": [vp, c.c_int, c.POINTER(c.c_float), c.POINTER(c.c_int)],
        "accel_plan_op_range_words": [vp, c.c_int, vp, c.c_int],
        "accel_tune_stats": [c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)],
        "accel_plan_finalize": [vp],
        "accel_plan_run": [vp],
        "accel_plan_num_ops": [vp],
        "accel_plan_op_info": [vp, i, c.c_char_p, c.c_char_p, c.POINTER(c.c_double), c.POINTER(c.c_double)],
        "accel_plan_profile": [vp, i, vp, i],
        "accel_plan_run_serial": [vp],
        "accel_plan_arena_read": [vp, sz, vp, sz, c.POINTER(sz)],
        "accel_model_write": [vp, c.c_char_p, vp, sz, i],
        "accel_model_bind_device": [vp, c.c_char_p, vp, sz],
        "accel_model_read": [vp, c.c_char_p, vp, sz, i],
        "accel_model_buffer": [vp, c.c_char_p, c.POINTER(vp), c.POINTER(sz)],
        "accel_model_buffer_generation": [vp, c.c_char_p, c.POINTER(c.c_uint64)],
        "accel_host_alloc": [sz, c.POINTER(vp)],
        "accel_host_free": [vp],
        "accel_model_prefetch": [vp, c.c_char_p, vp, sz],
        "accel_model_commit": [vp, c.c_char_p],
        "accel_model_read_async": [vp, c.c_char_p, vp, sz],
        "accel_frame_u8": [vp, vp, i, i, i, sz, vp, i, i, c.c_double, i, i, vp],
        "accel_model_write_u8": [vp, c.c_char_p, vp, i, i, i, sz, vp, i, i, c.c_double, i, i, i],
        "accel_model_prefetch_u8": [vp, c.c_char_p, vp, sz],
        "accel_model_commit_u8": [vp, c.c_char_p, i, i, i, sz, vp, i, i, c.c_double, i, i],
        "accel_nv12_coefficients": [i, c.POINTER(c.c_int32)],
        "accel_frame_nv12": [vp, vp, i, i, i, sz, sz, sz, i, vp, i, i, c.c_double, i, i, vp],
        "accel_nv12_to_bgr": [vp, vp, i, i, i, sz, sz, sz, i, vp, sz, i],
        "accel_model_write_nv12": [vp, c.c_char_p, vp, i, i, i, sz, sz, sz, i, vp, i, i, c.c_double, i, i, i],
        "accel_model_commit_nv12": [vp, c.c_char_p, i, i, i, sz, sz, sz, i, vp, i, i, c.c_double, i, i],
        "accel_yuv10_coefficients": [i, c.POINTER(c.c_int32)],
        "accel_frame_yuv": [vp, vp, i, c.POINTER(YUVLayout), vp, i, i, c.c_double, i, i, vp],
        "accel_yuv_to_bgr": [vp, vp, i, c.POINTER(YUVLayout), vp, sz, i],
        "accel_model_write_yuv": [vp, c.c_char_p, vp, i, c.POINTER(YUVLayout), vp, i, i, c.c_double, i, i, i],
        "accel_model_commit_yuv": [vp, c.c_char_p, i, c.POINTER(YUVLayout), vp, i, i, c.c_double, i, i],
        "accel_frame_yuv_sited": [vp, vp, i, c.POINTER(YUVLayout), vp, i, i, c.c_double, i, i, vp, i],
        "accel_yuv_to_bgr_sited": [vp, vp, i, c.POINTER(YUVLayout), vp, sz, i, i],
        "accel_model_write_yuv_sited": [vp, c.c_char_p, vp, i, c.POINTER(YUVLayout), vp, i, i, c.c_double, i, i, i, i],
        "accel_model_commit_yuv_sited": [vp, c.c_char_p, i, c.POINTER(YUVLayout), vp, i, i, c.c_double, i, i, i],
        "accel_labels_to_source": [vp, vp, i, i, i, i, i, i, i, vp, sz],
        "accel_labels_hist": [vp, vp, i, i, i, i, i, vp, i, i, sz, i, vp],
        "accel_labels_colour": [vp, vp, i, i, i, i, i, i, i, vp, i, vp, sz, i, vp, sz],
        "accel_model_labels_to_source": [vp, i, i, i, i, i, vp, sz, i],
        "accel_model_hist_add": [vp, vp, i, i, i, sz, i, i, i, i],
        "accel_model_hist_read": [vp, vp, i, i],
        "accel_model_labels_colour": [vp, i, i, i, i, i, vp, i, vp, sz, i, i, vp, sz, i],
        "accel_scores_confidence": [vp, vp, i, i, i, i, i, i, i, i, i, vp, sz, vp, sz, vp, sz, vp],
        "accel_model_confidence": [vp, i, i, i, i, i, i, vp, sz, vp, sz, vp, sz, vp, i],
        "accel_scores_confidence_interp": [vp, vp, i, i, i, i, i, i, i, i, i, vp, sz, vp, sz, vp, sz, vp, sz, vp],
        "accel_model_confidence_interp": [vp, i, i, i, i, i, i, vp, sz, vp, sz, vp, sz, vp, sz, vp, i],
        "accel_scores_labels": [vp, vp, i, i, i, i, i, i, i, i, vp, sz],
        "accel_model_scores_labels": [vp, i, i, i, i, i, vp, sz, i],
        "accel_model_scores_hist_add": [vp, vp, i, i, i, sz, i, i, i, i],
        "accel_model_scores_colour": [vp, i, i, i, i, i, vp, i, vp, sz, i, i, vp, sz, i],
        "accel_frame_change": [vp, vp, vp, i, i, i, i, i, i, i, vp, vp, vp, vp, sz],
        "accel_model_frame_change": [vp, c.c_char_p, i, i, i, i, i, vp, vp, vp, sz, i, c.POINTER(c.c_int)],
        "accel_model_frame_keep": [vp],
        "accel_labels_summary": [vp, vp, i, i, i, i, i, i, i, i, vp, sz, vp, vp, vp, vp, sz],
        "accel_model_labels_summary": [vp, i, i, i, i, i, i, i, vp, vp, vp, i, c.POINTER(c.c_int)],
        "accel_model_scores_summary": [vp, i, i, i, i, i, i, i, vp, vp, vp, i, c.POINTER(c.c_int)],
        "accel_labels_components": [vp, vp, i, i, i, i, i, i, i, i, i, i, i, vp, vp, vp, vp, sz],
        "accel_model_labels_components": [vp, i, i, i, i, i, i, i, i, i, i, vp, vp, vp, vp, sz],
        "accel_model_scores_components": [vp, i, i, i, i, i, i, i, i, i, i, vp, vp, vp, vp, sz],
        "accel_model_labels_forget": [vp],
        "accel_boundary_distance": [vp, vp, i, i, i, sz, i, vp, sz],
        "accel_labels_band_hist": [vp, vp, i, i, i, i, i, vp, i, i, sz, i, c.POINTER(c.c_int), i, vp],
        "accel_model_band_hist_add": [vp, vp, i, i, i, sz, i, i, i, c.POINTER(c.c_int), i, i],
        "accel_model_scores_band_hist_add": [vp, vp, i, i, i, sz, i, i, i, c.POINTER(c.c_int), i, i],
        "accel_model_band_hist_read": [vp, vp, i, i, i],
        "accel_labels_overlay_yuv": [vp, vp, i, i, i, i, i, c.POINTER(YUVLayout), vp, i, vp, vp],
        "accel_model_labels_overlay_yuv": [vp, i, i, i, c.POINTER(YUVLayout), vp, i, vp, i, vp, i],
        "accel_model_scores_overlay_yuv": [vp, i, i, i, c.POINTER(YUVLayout), vp, i, vp, i, vp, i],
        "accel_comm_available": [],
        "accel_comm_unique_id": [vp],
        "accel_comm_create": [vp, i, i, vp, c.POINTER(vp)],
        "accel_comm_destroy": [vp],
        "accel_gather_logits": [vp, vp, vp, sz, i],
        "accel_gather_frames": [vp, vp, sz, vp, sz, i],
        "accel_expand_scores": [vp, vp, i, vp, vp, vp],
        "accel_gather_scores": [vp, vp, i, i, vp, vp, vp, i],
        "accel_comm_sync": [vp],
        "accel_key_forward": [vp, vp, i, vp, vp, vp, i],
        "accel_cur_forward": [vp, vp, vp, i, vp, vp, vp, i],
        "accel_conv2d": [vp, vp, i, i, i, i, vp, vp, i, i, i, i, i, i, i, i, i, vp, vp, vp, i, f, i, vp],
        "accel_deconv2d_4x4s2": [vp, vp, i, i, i, i, vp, vp, i, i, f, vp],
        "accel_deform_conv2d": [vp, vp, i, i, i, i, vp, vp, i, i, i, i, i, i, i, i, i, i, vp],
        "accel_pool2d": [vp, vp, i, i, i, i, i, i, i, i, i, i, i, i, vp, vp, i, vp],
        "accel_flow_warp": [vp, vp, i, i, i, vp, vp],
        "accel_score_fuse": [vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, vp],
        "accel_argmax_c": [vp, vp, i, i, i, vp],
        "accel_flow_input": [vp, vp, vp, i, i, vp],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = i
    return sigs


EXPORTS = None


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (same soname as the system's).  Whichever copy a process loads
    first serves both users; when the SYSTEM copy came first, torch's later CUDA initialisation failed on this image
    ("No HIP GPUs are available": torch 2.10+rocm7.0 against the ROCm 7.2 runtime), while libaccel_hip runs fine on
    torch's copy.  So if torch is installed but not imported yet, its runtime is loaded before libaccel_hip.so --
    located through the import machinery, torch itself is NOT imported -- and any order of use works
    (tests/test_configs_gpu.py::test_torch_initialises_after_the_library).  ACCEL_SYSTEM_HIP=1 skips this."""
    import sys
    if "torch" in sys.modules or os.environ.get("ACCEL_SYSTEM_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    global _lib, EXPORTS
    if _lib is None:
        _share_torch_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise AccelError("libaccel_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                             "accel_amd has no CPU fallback")
        _lib = ctypes.CDLL(LIB_PATH)
        EXPORTS = _declare(_lib)
    return _lib


def tune_stats():
    """(decisions replayed from a table, decisions taken by timing, entries of the shipped table) of this process"""
    a, b, c_ = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib().accel_tune_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c_))
    return a.value, b.value, c_.value


def check(rc):
    if rc != 0:
        raise AccelError("libaccel_hip: %s (code %d)" % (lib().accel_last_error().decode(), rc))


def _fp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u8_frames(frames, width=None):
    """uint8 frames as the C ABI takes them: (contiguous array, n, h, w, pitch).  `frames` is n x h x w x 3 (or one h x w x 3
    frame), or -- with `width` -- n x h x pitch bytes: rows of `width` BGR pixels followed by padding bytes."""
    a = np.ascontiguousarray(frames, dtype=np.uint8)
    if width is not None:
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("pitched frames must be n x h x pitch bytes, got shape %s" % (a.shape,))
        return a, a.shape[0], a.shape[1], int(width), a.shape[2]
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[3] != 3:
        raise ValueError("frames must be n x h x w x 3 uint8 (BGR), got shape %s" % (a.shape,))
    return a, a.shape[0], a.shape[1], a.shape[2], 3 * a.shape[2]


def _nv12_frames(buf, h, w, pitch=None, uv_offset=None, frame_bytes=None, colour=0):
    """NV12 bytes as the C ABI takes them: (contiguous n x frame_bytes array, (n, h, w, pitch, uv_offset, frame_bytes, colour))"""
    from .utils import image
    lay = image.nv12_layout(h, w, pitch, uv_offset, frame_bytes)
    a = np.ascontiguousarray(image.nv12_bytes(buf, lay))
    return a, (a.shape[0], lay["h"], lay["w"], lay["pitch"], lay["uv_offset"], lay["frame_bytes"], image.nv12_colour(colour))


def nv12_coefficients(colour):
    """accel_nv12_coefficients: the six integers (yoff, ky, krv, kgu, kgv, kbu) of colour mode 0 .. 3 as the library holds them (no GPU)"""
    out = (ctypes.c_int32 * 6)()
    check(lib().accel_nv12_coefficients(int(colour), out))
    return tuple(int(v) for v in out)


def yuv_struct(layout, colour=None):
    """the YUVLayout of a utils.image.yuv_layout dict (`colour`, a name or a number, unless the dict holds one)"""
    from .utils import image
    colour = layout.get("colour", 0) if colour is None else colour
    return YUVLayout(int(layout["format"]), image.nv12_colour(colour), int(layout["h"]), int(layout["w"]), int(layout["pitch"]),
                     int(layout["pitch_c"]), int(layout["u_offset"]), int(layout["v_offset"]), int(layout["frame_bytes"]))


def _yuv_frames(buf, fmt, h, w, colour=0, **layout):
    """I420 / P010 / YUY2 bytes as the C ABI takes them: (contiguous flat uint8 array, n, YUVLayout); the keywords are those of
    utils.image.yuv_layout"""
    from .utils import image
    lay = image.yuv_layout(fmt, h, w, **layout)
    a, n = image.yuv_bytes(buf, lay)
    return a, n, yuv_struct(lay, colour)


def _siting(siting):
    """the number 0 .. 3 of a chroma siting (utils.image.chroma_siting)"""
    from .utils import image
    return image.chroma_siting(siting)


def nv12_struct(n, h, w, pitch, uv_offset, frame_bytes, colour):
    """NV12's flat layout as the YUVLayout of format 3 the _sited entry points take (`n` is dropped: the arguments are the tuple of
    _nv12_frames)"""
    return YUVLayout(3, int(colour), int(h), int(w), int(pitch), 0, int(uv_offset), 0, int(frame_bytes))


def yuv10_coefficients(colour):
    """accel_yuv10_coefficients: the six integers (yoff, ky, krv, kgu, kgv, kbu) of colour mode 0 .. 3 for P010's 10-bit samples (no GPU)"""
    out = (ctypes.c_int32 * 6)()
    check(lib().accel_yuv10_coefficients(int(colour), out))
    return tuple(int(v) for v in out)


def _means3(means_bgr):
    m = [float(v) for v in np.asarray(means_bgr, np.float64).reshape(-1)]
    if len(m) != 3:
        raise ValueError("means_bgr must hold three values (B, G, R)")
    return (ctypes.c_double * 3)(*m)


def _u8_maps(maps, width=None, what="labels"):
    """uint8 maps as the C ABI takes them: (contiguous array, n, h, w, pitch).  `maps` is n x h x w (or one h x w map), or --
    with `width` -- n x h x pitch bytes: rows of `width` pixels followed by padding bytes."""
    a = np.ascontiguousarray(maps, dtype=np.uint8)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("%s must be n x h x w uint8, got shape %s" % (what, a.shape))
    return a, a.shape[0], a.shape[1], a.shape[2] if width is None else int(width), a.shape[2]


def _widths(widths):
    """the widths of a trimap as the C ABI takes them: an array of ints (the library checks their values)"""
    ws = [int(v) for v in widths]
    return (ctypes.c_int * len(ws))(*ws)


def _palette(palette):
    p = np.ascontiguousarray(np.asarray(palette, dtype=np.uint8).reshape(-1))
    if p.size != 768:
        raise ValueError("the palette must hold 256 x 3 bytes (R, G, B), got %d" % p.size)
    return p


def _overlay_frames(buf, fmt, h, w, **layout):
    """frames an overlay is written over, as the C ABI takes them: (contiguous flat uint8 array, n, YUVLayout, shape of the result); `fmt` and the
    keywords are those of utils.image.overlay_layout (formats 0 .. 2 and "nv12" / 3)"""
    from .utils import image
    lay = image.overlay_layout(fmt, h, w, **layout)
    src = np.asarray(buf)
    if lay["format"] == 3:
        a = np.ascontiguousarray(image.nv12_bytes(src, lay)).reshape(-1)
        n = a.size // lay["frame_bytes"]
    else:
        a, n = image.yuv_bytes(src, lay)
    return a, n, yuv_struct(lay, 0), (src.shape if src.dtype == np.uint8 else a.shape)


def _table_ycc(table, fmt_number):
    t = np.ascontiguousarray(np.asarray(table).reshape(-1))
    top = 1023 if fmt_number == 1 else 255
    if t.size != 768 or not np.issubdtype(t.dtype, np.integer) or t.min() < 0 or t.max() > 65535:
        raise ValueError("the table must hold 256 x 3 integers (Y, Cb, Cr) in 0 .. %d (utils.image.palette_ycbcr)" % top)
    return np.ascontiguousarray(t.astype(np.uint16))


def _result_rows(out, n, h, w, channels):
    """the destination of a finishing call and its row pitch: a fresh n x h x w [x 3] array, or the caller's n x h x pitch bytes
    (only the first w * channels bytes of every row are written)"""
    if out is None:
        out = np.empty((n, h, w) if channels == 1 else (n, h, w, channels), np.uint8)
        return out, w * channels
    if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable or out.ndim != 3 or out.shape[:2] != (n, h):
        raise ValueError("out must be a writeable C-contiguous uint8 array of n x h x pitch = %d x %d x pitch bytes" % (n, h))
    return out, out.shape[2]


def _components_outputs(n, h, w, max_components, comp, sums, ids, width=None):
    """the destinations of a components call: (count, comp, sums, ids, ids pitch in bytes); comp / sums True or False, ids True, False or the
    caller's int32 array of n x h x pitch words (only the first w words of every row are written)"""
    cells = min(max(int(max_components), 0), 65536)
    count = np.zeros(n, np.int32)
    c = np.zeros((n, cells, 8), np.int32) if comp else None
    s = np.zeros((n, cells, 2), np.uint64) if sums else None
    if ids is None or ids is False:
        return count, c, s, None, 0
    if ids is True:
        return count, c, s, np.empty((n, h, w), np.int32), 4 * w
    if width is not None and int(width) != w:
        raise ValueError("width = %d, the rows of ids receive w = %d words" % (int(width), w))
    if ids.dtype != np.int32 or not ids.flags.c_contiguous or not ids.flags.writeable or ids.ndim != 3 or ids.shape[:2] != (n, h):
        raise ValueError("ids must be a writeable C-contiguous int32 array of n x h x pitch = %d x %d x pitch words" % (n, h))
    return count, c, s, ids, 4 * ids.shape[2]


def _confidence_outputs(n, h, w, conf, margin, second, hist, labels=None):
    """the destinations of a confidence call: for conf, margin and second True (a fresh tight array), False / None (left out) or the
    caller's array of n x h x pitch elements (uint8, for margin float32: pitch * 4 bytes per row), of which only the first w of every
    row are written; `hist` True or False.  Returns ([conf, margin, second, hist], [(pointer, pitch in bytes)] of the first three,
    hist pointer), with None / (None, 0) for what is left out.  labels (the interpolated forms; not None): the same rule as conf, and
    it comes first in both lists."""
    outs, ptrs = [], []
    first = () if labels is None else ((labels, np.uint8, "labels"),)
    for want, dtype, what in first + ((conf, np.uint8, "conf"), (margin, np.float32, "margin"), (second, np.uint8, "second")):
        if want is None or want is False:
            outs.append(None)
            ptrs.append((None, 0))
            continue
        if want is True:
            a = np.empty((n, h, w), dtype)
        else:
            a = want
            if a.dtype != dtype or not a.flags.c_contiguous or not a.flags.writeable or a.ndim != 3 or a.shape[:2] != (n, h):
                raise ValueError("%s must be a writeable C-contiguous %s array of n x h x pitch = %d x %d x pitch elements"
                                 % (what, np.dtype(dtype).name, n, h))
        outs.append(a)
        ptrs.append((_fp(a), a.shape[2] * a.itemsize))
    hs = np.zeros((n, 256), np.uint64) if hist else None
    outs.append(hs)
    return outs, ptrs, None if hs is None else _fp(hs)


class Context(object):
    def __init__(self, device_id=0):
        self.handle = ctypes.c_void_p()
        check(lib().accel_ctx_create(int(device_id), ctypes.byref(self.handle)))
        self.device_id = int(device_id)

    def sync(self):
        check(lib().accel_sync(self.handle))

    @property
    def stream(self):
        return lib().accel_ctx_stream(self.handle)

    def close(self):
        if self.handle:
            lib().accel_ctx_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    # ---- operator level (host NCHW fp32 in/out) --------------------------------
    def conv2d(self, x, w, bias=None, stride=1, pad=0, dilate=1, scale=None, shift=None,
               residual=None, act=0, slope=0.1, tile=-1):
        x, w = _f32(x), _f32(w)
        N, C, H, W = x.shape
        K, _, kh, kw = w.shape
        p2 = lambda v: (v, v) if np.isscalar(v) else tuple(v)
        (sh, sw), (ph, pw), (dh, dw) = p2(stride), p2(pad), p2(dilate)
        Ho = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
        Wo = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
        y = np.empty((N, K, Ho, Wo), np.float32)
        keep = [None if a is None else _f32(a) for a in (bias, scale, shift, residual)]
        ptr = [None if a is None else _fp(a) for a in keep]
        check(lib().accel_conv2d(self.handle, _fp(x), N, C, H, W, _fp(w), ptr[0], K, kh, kw, sh, sw, ph, pw,
                                 dh, dw, ptr[1], ptr[2], ptr[3], int(act), float(slope), int(tile), _fp(y)))
        return y

    def deconv2d_4x4s2(self, x, w, bias=None, act=0, slope=0.1):
        x, w = _f32(x), _f32(w)
        N, C, H, W = x.shape
        K = w.shape[1]
        y = np.empty((N, K, 2 * H, 2 * W), np.float32)
        b = None if bias is None else _f32(bias)
        check(lib().accel_deconv2d_4x4s2(self.handle, _fp(x), N, C, H, W, _fp(w), None if b is None else _fp(b),
                                         K, int(act), float(slope), _fp(y)))
        return y

    def deform_conv2d(self, x, offset, w, stride=1, pad=0, dilate=1, dg=1):
        x, offset, w = _f32(x), _f32(offset), _f32(w)
        N, C, H, W = x.shape
        K, _, kh, kw = w.shape
        Ho = (H + 2 * pad - dilate * (kh - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dilate * (kw - 1) - 1) // stride + 1
        y = np.empty((N, K, Ho, Wo), np.float32)
        check(lib().accel_deform_conv2d(self.handle, _fp(x), N, C, H, W, _fp(offset), _fp(w), K, kh, kw,
                                        stride, stride, pad, pad, dilate, dilate, dg, _fp(y)))
        return y

    def pool2d(self, x, kind, kernel, stride, pad=0, convention="valid", scale=None, shift=None, relu=False):
        x = _f32(x)
        N, C, H, W = x.shape
        full = convention == "full"
        po = lambda n: (1 + -(-(n + 2 * pad - kernel) // stride)) if full else (1 + (n + 2 * pad - kernel) // stride)
        y = np.empty((N, C, po(H), po(W)), np.float32)
        s = None if scale is None else _f32(scale)
        b = None if shift is None else _f32(shift)
        check(lib().accel_pool2d(self.handle, _fp(x), N, C, H, W, int(kind == "max"), int(full), kernel, kernel,
                                 stride, stride, pad, pad, None if s is None else _fp(s),
                                 None if b is None else _fp(b), int(relu), _fp(y)))
        return y

    def flow_warp(self, feat, flow):
        feat, flow = _f32(feat), _f32(flow)
        _, C, H, W = feat.shape
        out = np.empty_like(feat)
        check(lib().accel_flow_warp(self.handle, _fp(feat), C, H, W, _fp(flow), _fp(out)))
        return out

    def score_fuse(self, left, wl, right=None, wr=None, cw=None, cb=None):
        left, wl = _f32(left), _f32(wl)
        _, ncls, Hs, Ws = left.shape
        logits = np.empty((1, ncls, 16 * Hs, 16 * Ws), np.float32)
        labels = np.empty((1, 16 * Hs, 16 * Ws), np.uint8)
        opt = [None if a is None else _f32(a) for a in (right, wr, cw, cb)]
        ptr = [None if a is None else _fp(a) for a in opt]
        check(lib().accel_score_fuse(self.handle, _fp(left), ptr[0], ncls, Hs, Ws, _fp(wl), ptr[1], ptr[2], ptr[3],
                                     _fp(logits), _fp(labels)))
        return logits, labels

    def argmax_c(self, logits):
        logits = _f32(logits)
        _, C, H, W = logits.shape
        labels = np.empty((1, H, W), np.uint8)
        check(lib().accel_argmax_c(self.handle, _fp(logits), C, H, W, _fp(labels)))
        return labels

    def frame_u8(self, frames, means_bgr, out_h, out_w, step, H, W, width=None):
        """accel_frame_u8: uint8 BGR frames (see _u8_frames) -> the n x 3 x H x W fp32 tensor transform(resize(..)) gives on the
        host; out_h, out_w, step, H, W from utils.image.resize_geometry / resample_step"""
        a, n, h, w, pitch = _u8_frames(frames, width)
        out = np.empty((n, 3, int(H), int(W)), np.float32)
        check(lib().accel_frame_u8(self.handle, _fp(a), n, h, w, pitch, _means3(means_bgr), int(out_h), int(out_w), float(step),
                                   int(H), int(W), _fp(out)))
        return out

    def frame_nv12(self, buf, h, w, means_bgr, out_h, out_w, step, H, W, pitch=None, uv_offset=None, frame_bytes=None, colour=0, siting=0):
        """accel_frame_nv12: NV12 bytes (uint8, flat or n x frame_bytes; see utils.image.nv12_layout) -> the n x 3 x H x W fp32 tensor
        transform(resize(nv12_to_bgr_host(..))) gives on the host.  `siting` (utils.image.chroma_siting) other than replicate:
        accel_frame_yuv_sited with NV12 as format 3"""
        a, lay = _nv12_frames(buf, h, w, pitch, uv_offset, frame_bytes, colour)
        out = np.empty((lay[0], 3, int(H), int(W)), np.float32)
        if _siting(siting):
            check(lib().accel_frame_yuv_sited(self.handle, _fp(a), lay[0], ctypes.byref(nv12_struct(*lay)), _means3(means_bgr), int(out_h), int(out_w),
                                              float(step), int(H), int(W), _fp(out), _siting(siting)))
            return out
        check(lib().accel_frame_nv12(self.handle, _fp(a), *lay, _means3(means_bgr), int(out_h), int(out_w), float(step), int(H), int(W), _fp(out)))
        return out

    def nv12_to_bgr(self, buf, h, w, pitch=None, uv_offset=None, frame_bytes=None, colour=0, out=None, siting=0):
        """accel_nv12_to_bgr: NV12 bytes -> n x h x w x 3 uint8 BGR (utils.image.nv12_to_bgr_host, on the GPU); `out`: n x h x pitch
        bytes to write the rows into instead.  `siting` other than replicate: accel_yuv_to_bgr_sited with NV12 as format 3"""
        a, lay = _nv12_frames(buf, h, w, pitch, uv_offset, frame_bytes, colour)
        out, out_pitch = _result_rows(out, lay[0], lay[1], lay[2], 3)
        if _siting(siting):
            check(lib().accel_yuv_to_bgr_sited(self.handle, _fp(a), lay[0], ctypes.byref(nv12_struct(*lay)), _fp(out), out_pitch, _siting(siting), 0))
            return out
        check(lib().accel_nv12_to_bgr(self.handle, _fp(a), *lay, _fp(out), out_pitch, 0))
        return out

    def nv12_to_bgr_device(self, src_ptr, dst_ptr, n, h, w, pitch, uv_offset, frame_bytes, colour, out_pitch, siting=0):
        """the same from HBM into HBM (a decoder's output for a viewer, or for the blend of a colour image): only enqueued on the
        context's stream; the caller keeps the source unchanged until the kernel has run"""
        if _siting(siting):
            lay = nv12_struct(n, h, w, pitch, uv_offset, frame_bytes, colour)
            check(lib().accel_yuv_to_bgr_sited(self.handle, ctypes.c_void_p(src_ptr), int(n), ctypes.byref(lay), ctypes.c_void_p(dst_ptr),
                                               int(out_pitch), _siting(siting), 1))
            return
        check(lib().accel_nv12_to_bgr(self.handle, ctypes.c_void_p(src_ptr), int(n), int(h), int(w), int(pitch), int(uv_offset), int(frame_bytes),
                                      int(colour), ctypes.c_void_p(dst_ptr), int(out_pitch), 1))

    def frame_yuv(self, buf, fmt, h, w, means_bgr, out_h, out_w, step, H, W, colour=0, siting=0, **layout):
        """accel_frame_yuv: I420 / P010 / YUY2 bytes (see utils.image.yuv_layout for the layout keywords, yuv_bytes for the buffer) -> the
        n x 3 x H x W fp32 tensor transform(resize(yuv_to_bgr_host(..))) gives on the host.  `siting` (utils.image.chroma_siting) other
        than replicate: accel_frame_yuv_sited"""
        a, n, lay = _yuv_frames(buf, fmt, h, w, colour, **layout)
        out = np.empty((n, 3, int(H), int(W)), np.float32)
        if _siting(siting):
            check(lib().accel_frame_yuv_sited(self.handle, _fp(a), n, ctypes.byref(lay), _means3(means_bgr), int(out_h), int(out_w), float(step),
                                              int(H), int(W), _fp(out), _siting(siting)))
            return out
        check(lib().accel_frame_yuv(self.handle, _fp(a), n, ctypes.byref(lay), _means3(means_bgr), int(out_h), int(out_w), float(step), int(H), int(W),
                                    _fp(out)))
        return out

    def yuv_to_bgr(self, buf, fmt, h, w, colour=0, out=None, siting=0, **layout):
        """accel_yuv_to_bgr: I420 / P010 / YUY2 bytes -> n x h x w x 3 uint8 BGR (utils.image.yuv_to_bgr_host, on the GPU); `out`: n x h x pitch
        bytes to write the rows into instead.  `siting` other than replicate: accel_yuv_to_bgr_sited"""
        a, n, lay = _yuv_frames(buf, fmt, h, w, colour, **layout)
        out, out_pitch = _result_rows(out, n, lay.h, lay.w, 3)
        if _siting(siting):
            check(lib().accel_yuv_to_bgr_sited(self.handle, _fp(a), n, ctypes.byref(lay), _fp(out), out_pitch, _siting(siting), 0))
            return out
        check(lib().accel_yuv_to_bgr(self.handle, _fp(a), n, ctypes.byref(lay), _fp(out), out_pitch, 0))
        return out

    def yuv_to_bgr_device(self, src_ptr, dst_ptr, n, layout, out_pitch, colour=None, siting=0):
        """the same from HBM into HBM (`layout`: a utils.image.yuv_layout dict or a YUVLayout): only enqueued on the context's stream; the caller
        keeps the source unchanged until the kernel has run"""
        lay = layout if isinstance(layout, YUVLayout) else yuv_struct(layout, colour)
        if _siting(siting):
            check(lib().accel_yuv_to_bgr_sited(self.handle, ctypes.c_void_p(src_ptr), int(n), ctypes.byref(lay), ctypes.c_void_p(dst_ptr),
                                               int(out_pitch), _siting(siting), 1))
            return
        check(lib().accel_yuv_to_bgr(self.handle, ctypes.c_void_p(src_ptr), int(n), ctypes.byref(lay), ctypes.c_void_p(dst_ptr), int(out_pitch), 1))

    def labels_to_source(self, labels, out_h, out_w, h, w, out=None):
        """accel_labels_to_source: n x H x W label maps whose valid region is out_h x out_w -> n x h x w labels at the source size
        (utils.image.labels_to_source_host); `out`: n x h x pitch bytes to write the rows into instead"""
        a, n, H, W, _ = _u8_maps(labels)
        out, pitch = _result_rows(out, n, int(h), int(w), 1)
        check(lib().accel_labels_to_source(self.handle, _fp(a), n, H, W, int(out_h), int(out_w), int(h), int(w), _fp(out), pitch))
        return out

    def labels_hist(self, labels, out_h, out_w, gt, ncls, width=None, hist=None):
        """accel_labels_hist: the confusion matrix (rows gt, columns prediction, uint64 ncls x ncls) of the label maps taken to the
        size of `gt` (n x h x w, or n x h x pitch bytes with `width`), added to `hist` when one is given"""
        a, n, H, W, _ = _u8_maps(labels)
        g, gn, h, w, pitch = _u8_maps(gt, width, "gt")
        if gn != n:
            raise ValueError("%d label maps but %d ground-truth maps" % (n, gn))
        hist = np.zeros((int(ncls), int(ncls)), np.uint64) if hist is None else np.ascontiguousarray(hist, dtype=np.uint64).copy()
        check(lib().accel_labels_hist(self.handle, _fp(a), n, H, W, int(out_h), int(out_w), _fp(g), h, w, pitch, int(ncls), _fp(hist)))
        return hist

    def boundary_distance(self, maps, cap, width=None, out=None):
        """accel_boundary_distance: n x h x w uint8 maps (or n x h x pitch bytes with `width`) -> n x h x w uint8, the Chebyshev distance of every
        pixel to the nearest pixel with a differing 4-neighbour, capped at `cap` in 1 .. 16 (utils.image.boundary_distance_host); `out`: n x h x pitch
        bytes to write the rows into instead"""
        g, n, h, w, pitch = _u8_maps(maps, width, "maps")
        out, out_pitch = _result_rows(out, n, h, w, 1)
        check(lib().accel_boundary_distance(self.handle, _fp(g), n, h, w, pitch, int(cap), _fp(out), out_pitch))
        return out

    def labels_band_hist(self, labels, out_h, out_w, gt, ncls, widths, width=None, hist=None):
        """accel_labels_band_hist: the confusion matrix of labels_hist split into buckets of the distance to the boundaries of `gt`: uint64
        (len(widths) + 1) x ncls x ncls (utils.image.band_hist_host), added to `hist` when one is given"""
        a, n, H, W, _ = _u8_maps(labels)
        g, gn, h, w, pitch = _u8_maps(gt, width, "gt")
        if gn != n:
            raise ValueError("%d label maps but %d ground-truth maps" % (n, gn))
        ws = _widths(widths)
        shape = (len(ws) + 1, int(ncls), int(ncls))
        hist = np.zeros(shape, np.uint64) if hist is None else np.ascontiguousarray(hist, dtype=np.uint64).reshape(shape).copy()
        check(lib().accel_labels_band_hist(self.handle, _fp(a), n, H, W, int(out_h), int(out_w), _fp(g), h, w, pitch, int(ncls), ws, len(ws), _fp(hist)))
        return hist

    def labels_colour(self, labels, out_h, out_w, h, w, palette, frames=None, alpha=256, rgb=True, width=None, out=None):
        """accel_labels_colour: n x h x w x 3 colours palette[label] at the source size (utils.image.colour_host), blended with
        `frames` (uint8 BGR, see _u8_frames) when given; `out`: n x h x pitch bytes to write the rows into instead"""
        a, n, H, W, _ = _u8_maps(labels)
        f, fp = None, 0
        if frames is not None:
            f, fn, fh, fw, fp = _u8_frames(frames, width)
            if (fn, fh, fw) != (n, int(h), int(w)):
                raise ValueError("frames of %d x %d x %d for a result of %d x %d x %d" % (fn, fh, fw, n, h, w))
        out, pitch = _result_rows(out, n, int(h), int(w), 3)
        check(lib().accel_labels_colour(self.handle, _fp(a), n, H, W, int(out_h), int(out_w), int(h), int(w), _fp(_palette(palette)),
                                        int(bool(rgb)), None if f is None else _fp(f), fp, int(alpha), _fp(out), pitch))
        return out

    def labels_overlay_yuv(self, labels, out_h, out_w, buf, fmt, h, w, table, alpha=128, **layout):
        """accel_labels_overlay_yuv: n x H x W label maps whose valid region is out_h x out_w, blended over the frames in `buf` (I420 / P010 / YUY2
        / "nv12"; the layout keywords of utils.image.overlay_layout) with the colours `table` (256 x 3 Y, Cb, Cr: utils.image.palette_ycbcr) ->
        the bytes of the same frames in the same layout, uint8 in the shape of `buf` (utils.image.overlay_yuv_host of the labels at the source
        size, on the GPU)"""
        a, n, H, W, _ = _u8_maps(labels)
        f, fn, lay, shape = _overlay_frames(buf, fmt, h, w, **layout)
        if fn != n:
            raise ValueError("%d label maps but %d frames" % (n, fn))
        out = f.copy()      # the library fills n frames up to the last sample of the last one; what a buffer holds behind that is the input's too
        check(lib().accel_labels_overlay_yuv(self.handle, _fp(a), n, H, W, int(out_h), int(out_w), ctypes.byref(lay), _fp(_table_ycc(table, lay.format)),
                                             int(alpha), _fp(f), _fp(out)))
        return out.reshape(shape)

    def scores_confidence(self, scores, out_h, out_w, h, w, is_prob=False, conf=True, margin=True, second=True, hist=True):
        """accel_scores_confidence: n x ncls x H x W scores whose valid region is out_h x out_w -> (conf, margin, second, hist) at the
        source size h x w (utils.image.confidence_host); each of conf / margin / second is True, False (left out: None is returned
        in its place) or an array of n x h x pitch elements to write the rows into; hist True or False"""
        a = _f32(scores)
        if a.ndim != 4:
            raise ValueError("scores must be n x ncls x H x W fp32, got shape %s" % (a.shape,))
        n, ncls, H, W = a.shape
        outs, p, hp = _confidence_outputs(n, int(h), int(w), conf, margin, second, hist)
        check(lib().accel_scores_confidence(self.handle, _fp(a), n, ncls, H, W, int(out_h), int(out_w), int(h), int(w), int(bool(is_prob)),
                                            p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], hp))
        return tuple(outs)

    def scores_confidence_interp(self, scores, out_h, out_w, h, w, is_prob=False, labels=True, conf=True, margin=True, second=True, hist=True):
        """accel_scores_confidence_interp: n x ncls x H x W scores whose valid region is out_h x out_w -> (labels, conf, margin, second, hist)
        at the source size h x w, all five from the bilinearly interpolated scores (utils.image.confidence_interpolated_host); the
        arguments are those of scores_confidence, labels like conf"""
        a = _f32(scores)
        if a.ndim != 4:
            raise ValueError("scores must be n x ncls x H x W fp32, got shape %s" % (a.shape,))
        n, ncls, H, W = a.shape
        outs, p, hp = _confidence_outputs(n, int(h), int(w), conf, margin, second, hist, labels=False if labels is None else labels)
        check(lib().accel_scores_confidence_interp(self.handle, _fp(a), n, ncls, H, W, int(out_h), int(out_w), int(h), int(w), int(bool(is_prob)),
                                                   p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], p[3][0], p[3][1], hp))
        return tuple(outs)

    def scores_labels(self, scores, out_h, out_w, h, w, out=None):
        """accel_scores_labels: n x ncls x H x W scores whose valid region is out_h x out_w -> n x h x w labels at the source size, the
        argmax of the bilinearly interpolated scores (utils.image.labels_interpolated_host); `out`: n x h x pitch bytes to write the
        rows into instead"""
        a = _f32(scores)
        if a.ndim != 4:
            raise ValueError("scores must be n x ncls x H x W fp32, got shape %s" % (a.shape,))
        n, ncls, H, W = a.shape
        out, pitch = _result_rows(out, n, int(h), int(w), 1)
        check(lib().accel_scores_labels(self.handle, _fp(a), n, ncls, H, W, int(out_h), int(out_w), int(h), int(w), _fp(out), pitch))
        return out

    def frame_change(self, x, out_h, out_w, cell, level_q=0, sig_key=None, sig=True, changed=True, sad=True, mask=True):
        """accel_frame_change: the image input x (n x 3 x H x W fp32, valid region out_h x out_w) -> (sig, changed, sad, mask) -- its signature
        (n x gh x gw int32) and, against the signature `sig_key` of a key frame, the number of changed cells (n uint32), the sum of the
        differences (n uint64) and the mask (utils.image.frame_signature_host / frame_change_host).  sig / changed / sad are True or False
        (left out: None is returned in its place); mask True, False or an array of n x gh x pitch bytes to write the rows into.
        sig_key=None: the signature only -- (sig, None, None, None)"""
        a = _f32(x)
        if a.ndim != 4 or a.shape[1] != 3:
            raise ValueError("x must be n x 3 x H x W fp32, got shape %s" % (a.shape,))
        n, _, H, W = a.shape
        cell = int(cell)
        gh, gw = -(-int(out_h) // cell) if cell > 0 else 0, -(-int(out_w) // cell) if cell > 0 else 0
        key = None
        if sig_key is None:
            changed = sad = mask = False
        else:
            key = np.ascontiguousarray(sig_key, dtype=np.int32)
            if key.shape != (n, gh, gw):
                raise ValueError("sig_key of shape %s for %d frames of %d x %d cells" % (key.shape, n, gh, gw))
        s = np.empty((n, gh, gw), np.int32) if sig else None
        c = np.zeros(n, np.uint32) if changed else None
        d = np.zeros(n, np.uint64) if sad else None
        mk, pitch = (None, 0) if mask is None or mask is False else _result_rows(None if mask is True else mask, n, gh, gw, 1)
        opt = lambda v: None if v is None else _fp(v)
        check(lib().accel_frame_change(self.handle, _fp(a), opt(key), n, H, W, int(out_h), int(out_w), cell, int(level_q), opt(s), opt(c), opt(d),
                                       opt(mk), pitch))
        return s, c, d, mk

    def labels_summary(self, labels, out_h, out_w, h, w, ncls, prev=None, prev_width=None, stats=True, box=True, trans=None, kept=False):
        """accel_labels_summary: n x H x W label maps whose valid region is out_h x out_w -> (stats, box, trans, kept) at the source size h x w --
        per frame and class (area, sum_x, sum_y) as n x ncls x 3 uint64, the inclusive box (x0, y0, x1, y1) as n x ncls x 4 int32, against `prev`
        (the previous frame's labels at the source size: n x h x w, or n x h x pitch bytes with `prev_width` = w) the transitions as
        n x (ncls * ncls) uint64, and the current map at the source size, n x h x w uint8 (utils.image.labels_summary_host).  stats / box / trans
        are True or False (left out: None is returned in its place; trans defaults to whether there is a `prev`); kept True, False or an array of
        n x h x pitch bytes to write the rows into"""
        a, n, H, W, _ = _u8_maps(labels)
        h, w, ncls = int(h), int(w), int(ncls)
        p, pp = None, 0
        if prev is not None:
            p, pn, ph, pw, pp = _u8_maps(prev, prev_width, "prev")
            if (pn, ph, pw) != (n, h, w):
                raise ValueError("prev of %d x %d x %d for a result of %d x %d x %d" % (pn, ph, pw, n, h, w))
        if trans is None:
            trans = prev is not None
        cells = max(ncls, 0)
        s = np.zeros((n, cells, 3), np.uint64) if stats else None
        b = np.zeros((n, cells, 4), np.int32) if box else None
        t = np.zeros((n, cells * cells), np.uint64) if trans else None
        k, kp = (None, 0) if kept is None or kept is False else _result_rows(None if kept is True else kept, n, h, w, 1)
        opt = lambda v: None if v is None else _fp(v)
        check(lib().accel_labels_summary(self.handle, _fp(a), n, H, W, int(out_h), int(out_w), h, w, ncls, opt(p), pp, opt(s), opt(b), opt(t), opt(k), kp))
        return s, b, t, k

    def labels_components(self, labels, out_h, out_w, h, w, ncls, connectivity=8, min_area=1, max_components=1024, comp=True, sums=True, ids=False,
                          width=None):
        """accel_labels_components: n x H x W label maps whose valid region is out_h x out_w -> (count, comp, sums, ids) of the connected components
        of the map at the source size h x w (utils.image.labels_components_host): count n int32, comp n x max_components x 8 int32 = (class, area,
        x0, y0, x1, y1, ax, ay), sums n x max_components x 2 uint64 = (sum_x, sum_y), ids n x h x w int32.  comp / sums are True or False (left out:
        None in its place); ids True, False or an int32 array of n x h x pitch words to write the rows into (`width`: the words of a row that are
        written, w)"""
        a, n, H, W, _ = _u8_maps(labels)
        count, c, s, k, kp = _components_outputs(n, int(h), int(w), max_components, comp, sums, ids, width)
        opt = lambda v: None if v is None else _fp(v)
        check(lib().accel_labels_components(self.handle, _fp(a), n, H, W, int(out_h), int(out_w), int(h), int(w), int(ncls), int(connectivity),
                                            int(min_area), int(max_components), _fp(count), opt(c), opt(s), opt(k), kp))
        return count, c, s, k

    def flow_input(self, cur, prev):
        cur, prev = _f32(cur), _f32(prev)
        _, _, H, W = cur.shape
        out = np.empty((1, 6, H // 2, W // 2), np.float32)
        check(lib().accel_flow_input(self.handle, _fp(cur), _fp(prev), H, W, _fp(out)))
        return out


class PinnedBuffer(object):
    """Page-locked host memory (accel_host_alloc) seen as a numpy array: the source of accel_model_prefetch and the
    destination of accel_model_read_async.  Freed with the object."""

    def __init__(self, shape, dtype=np.float32):
        self.shape, self.dtype = tuple(int(v) for v in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self._ptr = ctypes.c_void_p()
        check(lib().accel_host_alloc(max(self.nbytes, 1), ctypes.byref(self._ptr)))
        raw = (ctypes.c_char * max(self.nbytes, 1)).from_address(self._ptr.value)
        self.array = np.frombuffer(raw, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)

    @property
    def ptr(self):
        return self._ptr

    def close(self):
        if self._ptr:
            self.array = None
            lib().accel_host_free(self._ptr)
            self._ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm(object):
    """RCCL communicator of the C ABI (accel_comm_*): one per process/GPU; `gather` is accel_gather_logits."""

    @staticmethod
    def available():
        """None if this process can resolve librccl and the entry points of the gather, else the reason (no communicator is made)"""
        rc = lib().accel_comm_available()
        return None if rc == 0 else lib().accel_last_error().decode()

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        check(lib().accel_comm_unique_id(buf))
        return buf.raw

    def __init__(self, ctx, rank, nranks, unique_id):
        self.ctx, self.rank, self.nranks = ctx, int(rank), int(nranks)
        self.handle = ctypes.c_void_p()
        idb = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(lib().accel_comm_create(ctx.handle, self.rank, self.nranks, idb, ctypes.byref(self.handle)))

    def gather(self, send_ptr, recv_ptr, nbytes, root=0, send_bytes=None):
        """send_bytes < nbytes: a root that contributes fewer clips than the slot size (accel_gather_frames)"""
        if send_bytes is None or int(send_bytes) == int(nbytes):
            check(lib().accel_gather_logits(self.handle, ctypes.c_void_p(send_ptr), ctypes.c_void_p(recv_ptr) if recv_ptr else None,
                                            int(nbytes), int(root)))
        else:
            check(lib().accel_gather_frames(self.handle, ctypes.c_void_p(send_ptr), int(send_bytes),
                                            ctypes.c_void_p(recv_ptr) if recv_ptr else None, int(nbytes), int(root)))

    def gather_scores(self, plan, own_images, slot_images, recv_scores=None, logits_out=None, labels_out=None, root=0):
        """accel_gather_scores: the score maps plan `plan` has just left in `scores`, from every rank to the root, expanded there into
        logits + labels (device pointers; None on peers)"""
        vp = lambda p: ctypes.c_void_p(p) if p else None
        check(lib().accel_gather_scores(self.handle, plan.handle, int(own_images), int(slot_images), vp(recv_scores), vp(logits_out), vp(labels_out), int(root)))

    def sync(self):
        check(lib().accel_comm_sync(self.handle))

    def close(self):
        if self.handle:
            lib().accel_comm_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class Plan(object):
    def __init__(self, model, handle, role):
        self.model, self.handle, self.role = model, handle, role

    def finalize(self):
        check(lib().accel_plan_finalize(self.handle))

    def run(self):
        check(lib().accel_plan_run(self.handle))

    def ops(self):
        n = lib().accel_plan_num_ops(self.handle)
        out = []
        kind = ctypes.create_string_buffer(32)
        name = ctypes.create_string_buffer(64)
        fl, by = ctypes.c_double(), ctypes.c_double()
        for i in range(n):
            check(lib().accel_plan_op_info(self.handle, i, kind, name, ctypes.byref(fl), ctypes.byref(by)))
            t, k, nw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            check(lib().accel_plan_op_launch(self.handle, i, ctypes.byref(t), ctypes.byref(k), ctypes.byref(nw)))
            md = ctypes.c_int()
            check(lib().accel_plan_op_mode(self.handle, i, ctypes.byref(md)))
            out.append({"kind": kind.value.decode(), "name": name.value.decode(), "flops": fl.value, "bytes": by.value,
                        "tile": t.value, "ksplit": k.value, "narrow": nw.value, "mode": md.value})
        return out

    def ranges(self):
        """fp16x2 form: {op name: (pixel scale of the last run, source)} of the convolutions that have one (accel_plan_op_range);
        source 0 = no run yet / all-zero input, 1 = raised by the writers' epilogues, 2 = measured by a pass over the input view"""
        out = {}
        kind = ctypes.create_string_buffer(32)
        name = ctypes.create_string_buffer(64)
        for i in range(lib().accel_plan_num_ops(self.handle)):
            s, src = ctypes.c_float(), ctypes.c_int()
            check(lib().accel_plan_op_range(self.handle, i, ctypes.byref(s), ctypes.byref(src)))
            if s.value:
                check(lib().accel_plan_op_info(self.handle, i, kind, name, None, None))
                out[name.value.decode()] = (s.value, int(src.value))
        return out

    def range_words(self, i):
        """diagnostics (accel_plan_op_range_words): the words of conv op i's input range slot after the last run, as uint32 --
        word 0 is what the convolution read, the partial words the writers raise follow (csrc/range.h)"""
        out = np.zeros(1088, np.uint32)
        check(lib().accel_plan_op_range_words(self.handle, int(i), _fp(out), out.size))
        return out

    def expand_scores(self, scores_ptr, n_images, logits_ptr, labels_ptr, comm=None):
        """accel_expand_scores: logits + labels of n_images score maps (device pointers) by this plan's own last launch"""
        check(lib().accel_expand_scores(self.handle, ctypes.c_void_p(scores_ptr), int(n_images), ctypes.c_void_p(logits_ptr), ctypes.c_void_p(labels_ptr),
                                        comm.handle if comm is not None else None))

    def run_serial(self):
        """diagnostics: every op in list order on the context stream (no graph replay), then a host wait"""
        check(lib().accel_plan_run_serial(self.handle))

    def arena(self):
        """diagnostics: host copy of the plan's activation arena (uint8)"""
        n = ctypes.c_size_t()
        check(lib().accel_plan_arena_read(self.handle, 0, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, np.uint8)
        check(lib().accel_plan_arena_read(self.handle, 0, _fp(out), out.nbytes, None))
        return out

    def profile(self, iters=3):
        n = lib().accel_plan_num_ops(self.handle)
        ms = np.zeros(n, np.float32)
        check(lib().accel_plan_profile(self.handle, int(iters), _fp(ms), n))
        return ms


class Model(object):
    def __init__(self, ctx):
        self.ctx = ctx
        self.handle = ctypes.c_void_p()
        check(lib().accel_model_create(ctx.handle, ctypes.byref(self.handle)))
        self.plans = {}

    def set_param(self, name, arr):
        a = _f32(arr)
        shape = (ctypes.c_int64 * a.ndim)(*a.shape)
        check(lib().accel_model_set_param(self.handle, name.encode(), _fp(a), a.ndim, shape))

    def set_params(self, *dicts):
        for d in dicts:
            for k, v in d.items():
                self.set_param(k, v.asnumpy() if hasattr(v, "asnumpy") else v)

    def add_plan(self, role, text):
        h = ctypes.c_void_p()
        check(lib().accel_model_add_plan(self.handle, role.encode(), text.encode(), ctypes.byref(h)))
        p = Plan(self, h, role)
        self.plans[role] = p
        return p

    def write(self, buf, arr):
        a = np.ascontiguousarray(arr)
        self.__dict__.get("_resident", {}).pop(buf, None)     # Predictor's record of which host array is in `buf`
        check(lib().accel_model_write(self.handle, buf.encode(), _fp(a), a.nbytes, 0))

    def write_device(self, buf, dev_ptr, nbytes):
        self.__dict__.get("_resident", {}).pop(buf, None)
        check(lib().accel_model_write(self.handle, buf.encode(), ctypes.c_void_p(dev_ptr), nbytes, 1))

    def bind_device(self, buf, dev_ptr, nbytes):
        """zero-copy input (accel_model_bind_device): the plans read the image input `buf` from the caller's HBM buffer until the
        next write / bind; the caller keeps that buffer alive and unchanged until the runs have completed"""
        self.__dict__.get("_resident", {}).pop(buf, None)
        check(lib().accel_model_bind_device(self.handle, buf.encode(), ctypes.c_void_p(dev_ptr), nbytes))

    def read(self, buf, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        check(lib().accel_model_read(self.handle, buf.encode(), _fp(out), out.nbytes, 0))
        return out

    def read_device(self, buf, dev_ptr, nbytes):
        """enqueue a D2D copy of a persistent buffer into caller-owned HBM (no host sync)"""
        check(lib().accel_model_read(self.handle, buf.encode(), ctypes.c_void_p(dev_ptr), nbytes, 1))

    def has_buffer(self, buf):
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        return lib().accel_model_buffer(self.handle, buf.encode(), ctypes.byref(ptr), ctypes.byref(n)) == 0

    def buffer(self, buf):
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        check(lib().accel_model_buffer(self.handle, buf.encode(), ctypes.byref(ptr), ctypes.byref(n)))
        return ptr.value, n.value

    def generation(self, buf):
        """write generation of a persistent buffer (accel_model_buffer_generation)"""
        g = ctypes.c_uint64()
        check(lib().accel_model_buffer_generation(self.handle, buf.encode(), ctypes.byref(g)))
        return int(g.value)

    def prefetch(self, buf, pinned):
        """enqueue the upload of a PinnedBuffer into the shadow of `buf` on the copy stream (overlaps the running plan)"""
        check(lib().accel_model_prefetch(self.handle, buf.encode(), pinned.ptr, pinned.nbytes))

    def commit(self, buf):
        self.__dict__.get("_resident", {}).pop(buf, None)
        check(lib().accel_model_commit(self.handle, buf.encode()))

    def write_u8(self, buf, frames, means_bgr, out_h, out_w, step, H, W, width=None):
        """accel_model_write_u8: host uint8 BGR frames (see _u8_frames) converted on the GPU into the image input `buf`"""
        a, n, h, w, pitch = _u8_frames(frames, width)
        self.__dict__.get("_resident", {}).pop(buf, None)
        check(lib().accel_model_write_u8(self.handle, buf.encode(), _fp(a), n, h, w, pitch, _means3(means_bgr), int(out_h), int(out_w),
                                         float(step), int(H), int(W), 0))

    def write_u8_device(self, buf, dev_ptr, n, h, w, pitch, means_bgr, out_h, out_w, step, H, W):
        """the same with the bytes already in HBM (a decoder's output, a torch uint8 tensor's data_ptr()): read in place; the
        caller keeps them unchanged until the kernel has run"""
        self.__dict__.get("_resident", {}).pop(buf, None)
        check(lib().accel_model_write_u8(self.handle, buf.encode(), ctypes.c_void_p(dev_ptr), int(n), int(h), int(w), int(pitch),
                                         _means3(means_bgr), int(out_h), int(out_w), float(step), int(H), int(W), 1))

    def prefetch_u8(self, buf, pinned):
        """enqueue the upload of a uint8 PinnedBuffer into the uint8 shadow of `buf` on the copy stream"""
        check(lib().accel_model_prefetch_u8(self.handle, buf.encode(), pinned.ptr, pinned.nbytes))

    def commit_u8(self, buf, n, h, w, pitch, means_bgr, out_h, out_w, step, H, W):
        """accel_model_commit_u8: the compute stream waits for prefetch_u8, then the kernel converts the shadow into `buf`"""
        self.__dict__.get("_resident", {}).pop(buf, None)
        check(lib().accel_model_commit_u8(self.handle, buf.encode(), int(n), int(h), int(w), int(pitch), _means3(means_bgr),
                                          int(out_h), int(out_w), float(step), int(H), int(W)))

    def write_nv12(self, buf, nv12, h, w, means_bgr, out_h, out_w, step, H, W, pitch=None, uv_offset=None, frame_bytes=None, colour=0, siting=0):
        """accel_model_write_nv12: host NV12 bytes (see Context.frame_nv12) converted on the GPU into the image input `buf`.  `siting` other
        than replicate: accel_model_write_yuv_sited with NV12 as format 3"""
        a, lay = _nv12_frames(nv12, h, w, pitch, uv_offset, frame_bytes, colour)
        self.__dict__.get("_resident", {}).pop(buf, None)
        if _siting(siting):
            check(lib().accel_model_write_yuv_sited(self.handle, buf.encode(), _fp(a), lay[0], ctypes.byref(nv12_struct(*lay)), _means3(means_bgr),
                                                    int(out_h), int(out_w), float(step), int(H), int(W), _siting(siting), 0))
            return
        check(lib().accel_model_write_nv12(self.handle, buf.encode(), _fp(a), *lay, _means3(means_bgr), int(out_h), int(out_w), float(step),
                                           int(H), int(W), 0))

    def write_nv12_device(self, buf, dev_ptr, n, h, w, pitch, uv_offset, frame_bytes, colour, means_bgr, out_h, out_w, step, H, W, siting=0):
        """the same with the bytes already in HBM (a decoder's output, a torch uint8 tensor's data_ptr()): read in place; the
        caller keeps them unchanged until the kernel has run"""
        self.__dict__.get("_resident", {}).pop(buf, None)
        if _siting(siting):
            lay = nv12_struct(n, h, w, pitch, uv_offset, frame_bytes, colour)
            check(lib().accel_model_write_yuv_sited(self.handle, buf.encode(), ctypes.c_void_p(dev_ptr), int(n), ctypes.byref(lay), _means3(means_bgr),
                                                    int(out_h), int(out_w), float(step), int(H), int(W), _siting(siting), 1))
            return
        check(lib().accel_model_write_nv12(self.handle, buf.encode(), ctypes.c_void_p(dev_ptr), int(n), int(h), int(w), int(pitch), int(uv_offset),
                                           int(frame_bytes), int(colour), _means3(means_bgr), int(out_h), int(out_w), float(step), int(H), int(W), 1))

    def commit_nv12(self, buf, n, h, w, pitch, uv_offset, frame_bytes, colour, means_bgr, out_h, out_w, step, H, W, siting=0):
        """accel_model_commit_nv12: the compute stream waits for prefetch_u8 (NV12 bytes go through the uint8 shadow), then the kernel
        converts the shadow into `buf`"""
        self.__dict__.get("_resident", {}).pop(buf, None)
        if _siting(siting):
            lay = nv12_struct(n, h, w, pitch, uv_offset, frame_bytes, colour)
            check(lib().accel_model_commit_yuv_sited(self.handle, buf.encode(), int(n), ctypes.byref(lay), _means3(means_bgr), int(out_h), int(out_w),
                                                     float(step), int(H), int(W), _siting(siting)))
            return
        check(lib().accel_model_commit_nv12(self.handle, buf.encode(), int(n), int(h), int(w), int(pitch), int(uv_offset), int(frame_bytes),
                                            int(colour), _means3(means_bgr), int(out_h), int(out_w), float(step), int(H), int(W)))

    def write_yuv(self, buf, yuv, fmt, h, w, means_bgr, out_h, out_w, step, H, W, colour=0, siting=0, **layout):
        """accel_model_write_yuv: host I420 / P010 / YUY2 bytes (see Context.frame_yuv) converted on the GPU into the image input `buf`.
        `siting` other than replicate: accel_model_write_yuv_sited"""
        a, n, lay = _yuv_frames(yuv, fmt, h, w, colour, **layout)
        self.__dict__.get("_resident", {}).pop(buf, None)
        if _siting(siting):
            check(lib().accel_model_write_yuv_sited(self.handle, buf.encode(), _fp(a), n, ctypes.byref(lay), _means3(means_bgr), int(out_h),
                                                    int(out_w), float(step), int(H), int(W), _siting(siting), 0))
            return
        check(lib().accel_model_write_yuv(self.handle, buf.encode(), _fp(a), n, ctypes.byref(lay), _means3(means_bgr), int(out_h), int(out_w),
                                          float(step), int(H), int(W), 0))

    def write_yuv_device(self, buf, dev_ptr, n, layout, means_bgr, out_h, out_w, step, H, W, colour=None, siting=0):
        """the same with the bytes already in HBM (`layout`: a utils.image.yuv_layout dict or a YUVLayout): read in place; the caller keeps
        them unchanged until the kernel has run"""
        lay = layout if isinstance(layout, YUVLayout) else yuv_struct(layout, colour)
        self.__dict__.get("_resident", {}).pop(buf, None)
        if _siting(siting):
            check(lib().accel_model_write_yuv_sited(self.handle, buf.encode(), ctypes.c_void_p(dev_ptr), int(n), ctypes.byref(lay), _means3(means_bgr),
                                                    int(out_h), int(out_w), float(step), int(H), int(W), _siting(siting), 1))
            return
        check(lib().accel_model_write_yuv(self.handle, buf.encode(), ctypes.c_void_p(dev_ptr), int(n), ctypes.byref(lay), _means3(means_bgr),
                                          int(out_h), int(out_w), float(step), int(H), int(W), 1))

    def commit_yuv(self, buf, n, layout, means_bgr, out_h, out_w, step, H, W, colour=None, siting=0):
        """accel_model_commit_yuv: the compute stream waits for prefetch_u8 (the bytes go through the uint8 shadow), then the kernel converts
        the shadow into `buf`"""
        lay = layout if isinstance(layout, YUVLayout) else yuv_struct(layout, colour)
        self.__dict__.get("_resident", {}).pop(buf, None)
        if _siting(siting):
            check(lib().accel_model_commit_yuv_sited(self.handle, buf.encode(), int(n), ctypes.byref(lay), _means3(means_bgr), int(out_h), int(out_w),
                                                     float(step), int(H), int(W), _siting(siting)))
            return
        check(lib().accel_model_commit_yuv(self.handle, buf.encode(), int(n), ctypes.byref(lay), _means3(means_bgr), int(out_h), int(out_w),
                                           float(step), int(H), int(W)))

    # ---- finished frames: they only READ `labels` (no generation changes) ------------------------------------------------------
    def labels_to_source(self, n, out_h, out_w, h, w, out=None):
        """accel_model_labels_to_source: the first n maps of `labels` at the source size h x w, as a numpy n x h x w uint8"""
        out, pitch = _result_rows(out, int(n), int(h), int(w), 1)
        check(lib().accel_model_labels_to_source(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), _fp(out), pitch, 0))
        return out

    def labels_to_source_device(self, dev_ptr, n, out_h, out_w, h, w, pitch):
        """the same into caller-owned HBM (enqueued, no host wait)"""
        check(lib().accel_model_labels_to_source(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), ctypes.c_void_p(dev_ptr), int(pitch), 1))

    def hist_add(self, gt, out_h, out_w, ncls, width=None):
        """accel_model_hist_add: add the confusion matrix of `labels` against host ground truth (n x h x w uint8, or n x h x pitch
        bytes with `width`) to the model's accumulator"""
        g, n, h, w, pitch = _u8_maps(gt, width, "gt")
        check(lib().accel_model_hist_add(self.handle, _fp(g), n, h, w, pitch, int(out_h), int(out_w), int(ncls), 0))

    def hist_add_device(self, dev_ptr, n, h, w, pitch, out_h, out_w, ncls):
        """the same with the ground truth already in HBM: read in place, nothing crosses PCIe; the caller keeps it unchanged until
        the kernel has run"""
        check(lib().accel_model_hist_add(self.handle, ctypes.c_void_p(dev_ptr), int(n), int(h), int(w), int(pitch), int(out_h), int(out_w), int(ncls), 1))

    def hist_read(self, ncls, clear=False):
        """accel_model_hist_read: the accumulator as uint64 ncls x ncls (rows gt, columns prediction); clear=True zeroes it"""
        out = np.zeros((int(ncls), int(ncls)), np.uint64)
        check(lib().accel_model_hist_read(self.handle, _fp(out), int(ncls), int(bool(clear))))
        return out

    # ---- trimap evaluation: an accumulator of its own, (len(widths) + 1) x ncls x ncls buckets ------------------------------------------
    def band_hist_add(self, gt, out_h, out_w, ncls, widths, width=None):
        """accel_model_band_hist_add: add the confusion matrix of `labels` against host ground truth (as hist_add takes it), split into buckets of
        the distance to the ground truth's boundaries, to the model's band accumulator (enqueued: no host wait beyond the upload of gt)"""
        g, n, h, w, pitch = _u8_maps(gt, width, "gt")
        ws = _widths(widths)
        check(lib().accel_model_band_hist_add(self.handle, _fp(g), n, h, w, pitch, int(out_h), int(out_w), int(ncls), ws, len(ws), 0))

    def band_hist_add_device(self, dev_ptr, n, h, w, pitch, out_h, out_w, ncls, widths):
        """the same against ground truth in caller-owned HBM: n x h rows, `pitch` bytes apart"""
        ws = _widths(widths)
        check(lib().accel_model_band_hist_add(self.handle, ctypes.c_void_p(dev_ptr), int(n), int(h), int(w), int(pitch), int(out_h), int(out_w), int(ncls),
                                              ws, len(ws), 1))

    def scores_band_hist_add(self, gt, out_h, out_w, ncls, widths, width=None):
        """accel_model_scores_band_hist_add: band_hist_add with the labels of the interpolated scores: the same accumulator, the same rule"""
        g, n, h, w, pitch = _u8_maps(gt, width, "gt")
        ws = _widths(widths)
        check(lib().accel_model_scores_band_hist_add(self.handle, _fp(g), n, h, w, pitch, int(out_h), int(out_w), int(ncls), ws, len(ws), 0))

    def band_hist_read(self, ncls, nwidths, clear=False):
        """accel_model_band_hist_read: the band accumulator as uint64 (nwidths + 1) x ncls x ncls buckets; clear=True zeroes it"""
        out = np.zeros((int(nwidths) + 1, int(ncls), int(ncls)), np.uint64)
        check(lib().accel_model_band_hist_read(self.handle, _fp(out), int(ncls), int(nwidths), int(bool(clear))))
        return out

    def _colour(self, fn, n, out_h, out_w, h, w, palette, frames, alpha, rgb, width, out):
        f, fp = None, 0
        if frames is not None:
            f, fn_, fh, fw, fp = _u8_frames(frames, width)
            if (fn_, fh, fw) != (int(n), int(h), int(w)):
                raise ValueError("frames of %d x %d x %d for a result of %d x %d x %d" % (fn_, fh, fw, n, h, w))
        out, pitch = _result_rows(out, int(n), int(h), int(w), 3)
        check(fn(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), _fp(_palette(palette)), int(bool(rgb)),
                 None if f is None else _fp(f), fp, int(alpha), 0, _fp(out), pitch, 0))
        return out

    def labels_colour(self, n, out_h, out_w, h, w, palette, frames=None, alpha=256, rgb=True, width=None, out=None):
        """accel_model_labels_colour: the first n maps of `labels` as n x h x w x 3 colours at the source size, blended with host
        `frames` (uint8 BGR, see _u8_frames) when given"""
        return self._colour(lib().accel_model_labels_colour, n, out_h, out_w, h, w, palette, frames, alpha, rgb, width, out)

    def labels_colour_device(self, dst_ptr, n, out_h, out_w, h, w, pitch, palette, frame_ptr=None, frame_pitch=0, alpha=256, rgb=True):
        """the same into caller-owned HBM, blended with frames that are in HBM already (enqueued, no host wait)"""
        check(lib().accel_model_labels_colour(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), _fp(_palette(palette)), int(bool(rgb)),
                                              ctypes.c_void_p(frame_ptr) if frame_ptr else None, int(frame_pitch), int(alpha), 1,
                                              ctypes.c_void_p(dst_ptr), int(pitch), 1))

    def confidence(self, n, out_h, out_w, h, w, is_prob=False, conf=True, margin=True, second=True, hist=True):
        """accel_model_confidence: (conf, margin, second, hist) of the first n frames of `logits` at the source size h x w, as numpy
        arrays (see Context.scores_confidence for the arguments); it only READS `logits`"""
        outs, p, hp = _confidence_outputs(int(n), int(h), int(w), conf, margin, second, hist)
        check(lib().accel_model_confidence(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), int(bool(is_prob)),
                                           p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], hp, 0))
        return tuple(outs)

    def confidence_device(self, n, out_h, out_w, h, w, is_prob=False, conf_ptr=None, conf_pitch=0, margin_ptr=None, margin_pitch=0,
                          second_ptr=None, second_pitch=0, hist_ptr=None):
        """the same into caller-owned HBM (enqueued, no host wait): device pointers, pitches in bytes; hist_ptr names n x 256 uint64"""
        vp = lambda v: ctypes.c_void_p(v) if v else None
        check(lib().accel_model_confidence(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), int(bool(is_prob)),
                                           vp(conf_ptr), int(conf_pitch), vp(margin_ptr), int(margin_pitch), vp(second_ptr), int(second_pitch),
                                           vp(hist_ptr), 1))

    def confidence_interp(self, n, out_h, out_w, h, w, is_prob=False, labels=True, conf=True, margin=True, second=True, hist=True):
        """accel_model_confidence_interp: (labels, conf, margin, second, hist) of the first n frames of `logits` interpolated to the source
        size h x w, as numpy arrays (see Context.scores_confidence_interp for the arguments); it only READS `logits`"""
        outs, p, hp = _confidence_outputs(int(n), int(h), int(w), conf, margin, second, hist, labels=False if labels is None else labels)
        check(lib().accel_model_confidence_interp(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), int(bool(is_prob)),
                                                  p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], p[3][0], p[3][1], hp, 0))
        return tuple(outs)

    def confidence_interp_device(self, n, out_h, out_w, h, w, is_prob=False, labels_ptr=None, labels_pitch=0, conf_ptr=None, conf_pitch=0,
                                 margin_ptr=None, margin_pitch=0, second_ptr=None, second_pitch=0, hist_ptr=None):
        """the same into caller-owned HBM (enqueued, no host wait): device pointers, pitches in bytes; hist_ptr names n x 256 uint64"""
        vp = lambda v: ctypes.c_void_p(v) if v else None
        check(lib().accel_model_confidence_interp(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), int(bool(is_prob)),
                                                  vp(labels_ptr), int(labels_pitch), vp(conf_ptr), int(conf_pitch), vp(margin_ptr), int(margin_pitch),
                                                  vp(second_ptr), int(second_pitch), vp(hist_ptr), 1))

    # ---- frame change: it only READS the image input ---------------------------------------------------------------------------
    def frame_change(self, buf, n, out_h, out_w, cell, level_q, mask=False):
        """accel_model_frame_change: the signature of the first n frames of the image input `buf` (what the plans would read: a bound frame
        included) becomes the model's CURRENT signature and is compared with the KEPT one (frame_keep) if that was made under the same
        (n, out_h, out_w, cell): -> (changed n uint32, sad n uint64[, mask n x gh x gw uint8]) as numpy arrays, or None where nothing was
        compared.  It only READS `buf`"""
        n, cell = int(n), int(cell)
        c, d = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        mk, pitch = (None, 0)
        if mask and cell > 0:
            mk = np.zeros((n, -(-int(out_h) // cell), -(-int(out_w) // cell)), np.uint8)
            pitch = mk.shape[2]
        compared = ctypes.c_int(0)
        check(lib().accel_model_frame_change(self.handle, buf.encode(), n, int(out_h), int(out_w), cell, int(level_q), _fp(c), _fp(d),
                                             None if mk is None else _fp(mk), pitch, 0, ctypes.byref(compared)))
        if not compared.value:
            return None
        return (c, d, mk) if mask else (c, d)

    def frame_change_device(self, buf, n, out_h, out_w, cell, level_q, changed_ptr=None, sad_ptr=None, mask_ptr=None, mask_pitch=0):
        """the same into caller-owned HBM (enqueued, no host wait): n uint32, n uint64 and n x gh rows of mask_pitch bytes; -> whether the kept
        signature was compared with (the destinations are written only then)"""
        vp = lambda v: ctypes.c_void_p(v) if v else None
        compared = ctypes.c_int(0)
        check(lib().accel_model_frame_change(self.handle, buf.encode(), int(n), int(out_h), int(out_w), int(cell), int(level_q), vp(changed_ptr),
                                             vp(sad_ptr), vp(mask_ptr), int(mask_pitch), 1, ctypes.byref(compared)))
        return bool(compared.value)

    def frame_keep(self):
        """accel_model_frame_keep: the current signature (the last frame_change) becomes the kept one, the one later frames are compared with"""
        check(lib().accel_model_frame_keep(self.handle))

    # ---- summary of finished frames: it only READS `labels` / `logits` ------------------------------------------------------------
    def _summary(self, fn, n, out_h, out_w, h, w, ncls, track, stats, box):
        n, ncls = int(n), int(ncls)
        cells = max(ncls, 0)
        s = np.zeros((n, cells, 3), np.uint64) if stats else None
        b = np.zeros((n, cells, 4), np.int32) if box else None
        t = np.zeros((n, cells * cells), np.uint64) if track else None
        compared = ctypes.c_int(0)
        opt = lambda v: None if v is None else _fp(v)
        check(fn(self.handle, n, int(out_h), int(out_w), int(h), int(w), ncls, int(bool(track)), opt(s), opt(b), opt(t), 0, ctypes.byref(compared)))
        return s, b, t if compared.value else None

    def _summary_device(self, fn, n, out_h, out_w, h, w, ncls, track, stats_ptr, box_ptr, trans_ptr):
        vp = lambda v: ctypes.c_void_p(v) if v else None
        compared = ctypes.c_int(0)
        check(fn(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), int(ncls), int(bool(track)), vp(stats_ptr), vp(box_ptr), vp(trans_ptr), 1,
                 ctypes.byref(compared)))
        return bool(compared.value)

    def labels_summary(self, n, out_h, out_w, h, w, ncls, track=False, stats=True, box=True):
        """accel_model_labels_summary: (stats, box, trans) of the first n maps of `labels` at the source size h x w, as numpy arrays (see
        Context.labels_summary).  track=True compares with the model's KEPT map -- trans is None where there was none made under the same
        (n, h, w, ncls) -- and the current map becomes the kept one; track=False neither reads nor writes it.  It only READS `labels`"""
        return self._summary(lib().accel_model_labels_summary, n, out_h, out_w, h, w, ncls, track, stats, box)

    def labels_summary_device(self, n, out_h, out_w, h, w, ncls, track=False, stats_ptr=None, box_ptr=None, trans_ptr=None):
        """the same into caller-owned HBM (enqueued, no host wait): n x ncls x 3 uint64, n x ncls x 4 int32, n x ncls x ncls uint64; -> whether
        the kept map was compared with (trans is written only then)"""
        return self._summary_device(lib().accel_model_labels_summary, n, out_h, out_w, h, w, ncls, track, stats_ptr, box_ptr, trans_ptr)

    def scores_summary(self, n, out_h, out_w, h, w, ncls, track=False, stats=True, box=True):
        """accel_model_scores_summary: labels_summary with the labels of the interpolated scores; the same kept map"""
        return self._summary(lib().accel_model_scores_summary, n, out_h, out_w, h, w, ncls, track, stats, box)

    def scores_summary_device(self, n, out_h, out_w, h, w, ncls, track=False, stats_ptr=None, box_ptr=None, trans_ptr=None):
        """the same into caller-owned HBM (enqueued, no host wait)"""
        return self._summary_device(lib().accel_model_scores_summary, n, out_h, out_w, h, w, ncls, track, stats_ptr, box_ptr, trans_ptr)

    # ---- connected components of finished frames: they only READ `labels` / `logits` ------------------------------------------------
    def _components(self, fn, n, out_h, out_w, h, w, ncls, connectivity, min_area, max_components, comp, sums, ids):
        n = int(n)
        count, c, s, k, kp = _components_outputs(n, int(h), int(w), max_components, comp, sums, ids)
        opt = lambda v: None if v is None else _fp(v)
        check(fn(self.handle, n, int(out_h), int(out_w), int(h), int(w), int(ncls), int(connectivity), int(min_area), int(max_components), 0,
                 _fp(count), opt(c), opt(s), opt(k), kp))
        return count, c, s, k

    def _components_device(self, fn, n, out_h, out_w, h, w, ncls, connectivity, min_area, max_components, count_ptr, comp_ptr, sums_ptr, ids_ptr,
                           ids_pitch):
        vp = lambda v: ctypes.c_void_p(v) if v else None
        check(fn(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), int(ncls), int(connectivity), int(min_area), int(max_components), 1,
                 vp(count_ptr), vp(comp_ptr), vp(sums_ptr), vp(ids_ptr), int(ids_pitch if ids_pitch is not None else 4 * int(w))))

    def labels_components(self, n, out_h, out_w, h, w, ncls, connectivity=8, min_area=1, max_components=1024, comp=True, sums=True, ids=False):
        """accel_model_labels_components: (count, comp, sums, ids) of the first n maps of `labels` at the source size h x w, as numpy arrays (see
        Context.labels_components).  It only READS `labels`"""
        return self._components(lib().accel_model_labels_components, n, out_h, out_w, h, w, ncls, connectivity, min_area, max_components, comp, sums, ids)

    def labels_components_device(self, n, out_h, out_w, h, w, ncls, connectivity=8, min_area=1, max_components=1024, count_ptr=None, comp_ptr=None,
                                 sums_ptr=None, ids_ptr=None, ids_pitch=None):
        """the same into caller-owned HBM (enqueued, no host wait): n int32, n x max_components x 8 int32, n x max_components x 2 uint64 and
        n x h rows of w int32 `ids_pitch` bytes apart (default 4 * w)"""
        self._components_device(lib().accel_model_labels_components, n, out_h, out_w, h, w, ncls, connectivity, min_area, max_components, count_ptr,
                                comp_ptr, sums_ptr, ids_ptr, ids_pitch)

    def scores_components(self, n, out_h, out_w, h, w, ncls, connectivity=8, min_area=1, max_components=1024, comp=True, sums=True, ids=False):
        """accel_model_scores_components: labels_components with the labels of the interpolated scores; ncls is the class count of `logits`"""
        return self._components(lib().accel_model_scores_components, n, out_h, out_w, h, w, ncls, connectivity, min_area, max_components, comp, sums, ids)

    def scores_components_device(self, n, out_h, out_w, h, w, ncls, connectivity=8, min_area=1, max_components=1024, count_ptr=None, comp_ptr=None,
                                 sums_ptr=None, ids_ptr=None, ids_pitch=None):
        """the same into caller-owned HBM (enqueued, no host wait)"""
        self._components_device(lib().accel_model_scores_components, n, out_h, out_w, h, w, ncls, connectivity, min_area, max_components, count_ptr,
                                comp_ptr, sums_ptr, ids_ptr, ids_pitch)

    def labels_forget(self):
        """accel_model_labels_forget: drop the kept map (a new clip, a cut): the next tracked summary compares with nothing"""
        check(lib().accel_model_labels_forget(self.handle))

    # ---- labels from interpolated scores: they only READ `logits` ------------------------------------------------------------
    def scores_labels(self, n, out_h, out_w, h, w, out=None):
        """accel_model_scores_labels: the argmax of the first n frames of `logits` interpolated to the source size h x w, as a numpy
        n x h x w uint8 (utils.image.labels_interpolated_host)"""
        out, pitch = _result_rows(out, int(n), int(h), int(w), 1)
        check(lib().accel_model_scores_labels(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), _fp(out), pitch, 0))
        return out

    def scores_labels_device(self, dev_ptr, n, out_h, out_w, h, w, pitch):
        """the same into caller-owned HBM (enqueued, no host wait)"""
        check(lib().accel_model_scores_labels(self.handle, int(n), int(out_h), int(out_w), int(h), int(w), ctypes.c_void_p(dev_ptr), int(pitch), 1))

    def scores_hist_add(self, gt, out_h, out_w, ncls, width=None):
        """accel_model_scores_hist_add: hist_add with the labels of the interpolated scores: the same accumulator, the same ncls rule"""
        g, n, h, w, pitch = _u8_maps(gt, width, "gt")
        check(lib().accel_model_scores_hist_add(self.handle, _fp(g), n, h, w, pitch, int(out_h), int(out_w), int(ncls), 0))

    def scores_colour(self, n, out_h, out_w, h, w, palette, frames=None, alpha=256, rgb=True, width=None, out=None):
        """accel_model_scores_colour: labels_colour with the labels of the interpolated scores"""
        return self._colour(lib().accel_model_scores_colour, n, out_h, out_w, h, w, palette, frames, alpha, rgb, width, out)

    # ---- the overlay in the frame's own format: they only READ `labels` / `logits` -------------------------------------------------
    def _overlay_yuv(self, fn, n, out_h, out_w, buf, fmt, h, w, table, alpha, layout):
        f, fn_, lay, shape = _overlay_frames(buf, fmt, h, w, **layout)
        if fn_ != int(n):
            raise ValueError("%d frames for a result of %d" % (fn_, n))
        out = f.copy()      # the library fills n frames up to the last sample of the last one; what a buffer holds behind that is the input's too
        check(fn(self.handle, int(n), int(out_h), int(out_w), ctypes.byref(lay), _fp(_table_ycc(table, lay.format)), int(alpha), _fp(f), 0, _fp(out), 0))
        return out.reshape(shape)

    def _overlay_yuv_device(self, fn, src_ptr, dst_ptr, n, out_h, out_w, layout, table, alpha):
        lay = layout if isinstance(layout, YUVLayout) else yuv_struct(layout, 0)
        check(fn(self.handle, int(n), int(out_h), int(out_w), ctypes.byref(lay), _fp(_table_ycc(table, lay.format)), int(alpha),
                 ctypes.c_void_p(src_ptr) if src_ptr else None, 1, ctypes.c_void_p(dst_ptr) if dst_ptr else None, 1))

    def labels_overlay_yuv(self, n, out_h, out_w, buf, fmt, h, w, table, alpha=128, **layout):
        """accel_model_labels_overlay_yuv: the first n maps of `labels` blended over the host frames in `buf` (see Context.labels_overlay_yuv)
        -> the bytes of the same frames in the same layout, uint8 in the shape of `buf`"""
        return self._overlay_yuv(lib().accel_model_labels_overlay_yuv, n, out_h, out_w, buf, fmt, h, w, table, alpha, layout)

    def labels_overlay_yuv_device(self, src_ptr, dst_ptr, n, out_h, out_w, layout, table, alpha=128):
        """the same from frames in HBM into caller-owned HBM of the same layout (`layout`: a utils.image.overlay_layout dict or a YUVLayout);
        dst_ptr == src_ptr blends in place, any other overlap is refused.  Enqueued, no host wait"""
        self._overlay_yuv_device(lib().accel_model_labels_overlay_yuv, src_ptr, dst_ptr, n, out_h, out_w, layout, table, alpha)

    def scores_overlay_yuv(self, n, out_h, out_w, buf, fmt, h, w, table, alpha=128, **layout):
        """accel_model_scores_overlay_yuv: labels_overlay_yuv with the labels of the interpolated scores"""
        return self._overlay_yuv(lib().accel_model_scores_overlay_yuv, n, out_h, out_w, buf, fmt, h, w, table, alpha, layout)

    def scores_overlay_yuv_device(self, src_ptr, dst_ptr, n, out_h, out_w, layout, table, alpha=128):
        """the same from frames in HBM into caller-owned HBM; dst_ptr == src_ptr blends in place"""
        self._overlay_yuv_device(lib().accel_model_scores_overlay_yuv, src_ptr, dst_ptr, n, out_h, out_w, layout, table, alpha)

    def read_async(self, buf, pinned):
        """enqueue the download of `buf` into a PinnedBuffer on the compute stream; valid after ctx.sync()"""
        check(lib().accel_model_read_async(self.handle, buf.encode(), pinned.ptr, pinned.nbytes))

    def _outs(self, want, H, W, ncls=19):
        feat = np.empty((1, 2048, H // 16, W // 16), np.float32) if "feat" in want else None
        logits = np.empty((1, ncls, H, W), np.float32) if "logits" in want else None
        labels = np.empty((1, H, W), np.uint8) if "labels" in want else None
        return feat, logits, labels

    def key_forward(self, img, want=("logits", "labels")):
        """accel_key_forward: host image in, requested host outputs back (dict)."""
        img = _f32(img)
        H, W = img.shape[-2:]
        f, lg, lb = self._outs(want, H, W)
        self.__dict__.get("_resident", {}).clear()
        check(lib().accel_key_forward(self.handle, _fp(img), 0, None if f is None else _fp(f), None if lg is None else _fp(lg),
                                      None if lb is None else _fp(lb), 0))
        return {k: v for k, v in (("feat", f), ("logits", lg), ("labels", lb)) if v is not None}

    def cur_forward(self, img_cur, img_prev, want=("logits", "labels")):
        a, b = _f32(img_cur), _f32(img_prev)
        H, W = a.shape[-2:]
        f, lg, lb = self._outs(want, H, W)
        self.__dict__.get("_resident", {}).clear()
        check(lib().accel_cur_forward(self.handle, _fp(a), _fp(b), 0, None if f is None else _fp(f),
                                      None if lg is None else _fp(lg), None if lb is None else _fp(lb), 0))
        return {k: v for k, v in (("feat", f), ("logits", lg), ("labels", lb)) if v is not None}

    def close(self):
        if self.handle:
            lib().accel_model_destroy(self.handle)
            self.handle = ctypes.c_void_p()
