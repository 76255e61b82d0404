"""Array handles exchanged between harness code and the Predictor.

A DeviceArray is either host data (numpy) or a reference to a buffer that
lives in HBM inside a plan/model of the HIP runtime; `.asnumpy()` is the only
synchronising call, like `mx.nd.NDArray.asnumpy()` in the reference's demo
loop (dff_deeplab/demo.py:238,245)."""
import itertools

import numpy as np

_UID = itertools.count(1)


class DeviceArray(object):
    """Immutable once built (like an NDArray the harness never writes into): `uid` identifies the CONTENT, which is what
    lets a Predictor recognise that the bytes of an input are already in HBM.  Host data is a private copy
    (mx.nd.array copies, as MXNet does) and is handed out read-only."""

    def __init__(self, host=None, shape=None, fetch=None, device_ref=None, labels_of=None, pinned=None):
        self.uid = next(_UID)
        self._host = host
        if self._host is not None and self._host.flags.writeable:
            self._host.setflags(write=False)
        self._shape = tuple(shape) if shape is not None else tuple(self._host.shape)
        self._fetch = fetch            # callable -> numpy (blocks)
        self.device_ref = device_ref   # (owner model, buffer name, write generation) when resident in HBM
        self.labels_of = labels_of     # callable -> DeviceArray of the fused argmax, if any
        self.pinned = pinned           # runtime.PinnedBuffer behind `_host` when built with ctx=mx.cpu_pinned()

    @property
    def shape(self):
        return self._shape

    @property
    def on_device(self):
        return self._host is None

    @property
    def has_host_copy(self):
        return self._host is not None

    def asnumpy(self):
        """Blocks until the data is on the host.  The array is read-only: copy it before editing (MXNet returns a
        fresh copy on every call; one shared read-only copy keeps 160 MB logit maps from being duplicated)."""
        if self._host is None:
            h = np.ascontiguousarray(self._fetch())
            h.setflags(write=False)
            self._host = h
        return self._host

    def __repr__(self):
        return "<DeviceArray %s %s>" % ("x".join(map(str, self._shape)),
                                        "hbm" if self._host is None else "host")


def array(src, ctx=None, dtype=np.float32):
    """mx.nd.array: always a COPY of `src` (later edits of `src` do not reach the array).  With
    ctx=mx.cpu_pinned() the copy lives in page-locked memory, the source of overlapped uploads."""
    if isinstance(src, DeviceArray):
        return src
    a = np.asarray(src)
    if ctx is not None and getattr(ctx, "device_type", "") == "cpu_pinned":
        from .. import runtime
        pb = runtime.PinnedBuffer(a.shape, dtype)
        pb.array[...] = a
        return DeviceArray(host=pb.array, pinned=pb)
    return DeviceArray(host=np.array(a, dtype=dtype, order="C", copy=True))


class RawFrames(DeviceArray):
    """Video frames as a camera, a decoder or a PNG gives them -- uint8 N x h x w x 3, BGR -- standing for the image tensor the
    graphs read: `.shape` is the (N, 3, H, W) of transform(resize(frame)) (lib/utils/image.py:194-235), and a Predictor
    uploads the BYTES (a quarter of the fp32 tensor) and has the GPU resize, remove the mean and pad
    (accel_model_write_u8 / _prefetch_u8 / _commit_u8).  `.asnumpy()` is that tensor computed on the host, lazily, so a
    consumer that knows nothing about raw frames still works.  All frames of one array have the same size."""

    def __init__(self, frames_bgr_u8, pixel_means, target_size, max_size, stride=0, ctx=None):
        from ..utils import image
        if isinstance(frames_bgr_u8, (list, tuple)):
            if len({np.shape(f) for f in frames_bgr_u8}) != 1:
                raise ValueError("all frames of one raw-frame array must have the same size")
            frames_bgr_u8 = np.stack([np.asarray(f) for f in frames_bgr_u8])
        a = np.asarray(frames_bgr_u8)
        if a.ndim == 3:
            a = a[None]
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
            raise ValueError("raw frames must be uint8 N x h x w x 3 (BGR), got %s %s" % (a.dtype, a.shape))
        n, h, w = a.shape[:3]
        pb = None
        if ctx is not None and getattr(ctx, "device_type", "") == "cpu_pinned":
            from .. import runtime
            pb = runtime.PinnedBuffer(a.shape, np.uint8)
            pb.array[...] = a
            frames = pb.array
        else:
            frames = np.array(a, order="C", copy=True)      # a copy, like mx.nd.array: later edits of the source do not reach it
        frames.setflags(write=False)
        scale, out_h, out_w, H, W = image.resize_geometry(h, w, target_size, max_size, stride)
        DeviceArray.__init__(self, shape=(n, 3, H, W), fetch=self._host_tensor, pinned=pb)
        self.frames = frames
        self.means = tuple(float(v) for v in np.asarray(pixel_means, np.float64).reshape(-1))
        self.resize_args = (target_size, max_size, stride)
        self.scale = scale
        # what the C ABI is told (include/accel_hip.h, uint8 video frames)
        self.geometry = dict(out_h=out_h, out_w=out_w, step=image.resample_step(h, w, scale, out_h, out_w), H=H, W=W)

    def _host_tensor(self):
        from ..utils import image
        t, m, s = self.resize_args
        return np.concatenate([image.transform(image.resize(f, t, m, stride=s)[0], self.means) for f in self.frames]).astype(np.float32)

    @property
    def on_device(self):
        return False

    @property
    def has_host_copy(self):
        return True

    def __repr__(self):
        return "<RawFrames %s uint8 for %s>" % ("x".join(map(str, self.frames.shape)), "x".join(map(str, self._shape)))


def raw_frames(frames_bgr_u8, cfg, ctx=None):
    """Raw uint8 BGR frames (one h x w x 3 frame, N x h x w x 3, or a list of frames of one size) for a Predictor, resized
    to cfg.SCALES[0], centred on cfg.network.PIXEL_MEANS and padded to cfg.network.IMAGE_STRIDE on the GPU.  Always a COPY
    of the bytes; with ctx=mx.cpu_pinned() in page-locked memory."""
    target_size, max_size = cfg.SCALES[0][0], cfg.SCALES[0][1]
    return RawFrames(frames_bgr_u8, cfg.network.PIXEL_MEANS, target_size, max_size, cfg.network.IMAGE_STRIDE, ctx=ctx)


class NV12Frames(RawFrames):
    """Video frames as a decoder hands them out -- NV12: a luma plane and a half-size plane of interleaved Cb, Cr -- standing for the same
    image tensor as the RawFrames of their BGR conversion (utils.image.nv12_to_bgr_host): a Predictor uploads the BYTES, 1.5 per pixel,
    and the GPU converts the colour, resizes, removes the mean and pads (accel_model_write_nv12 / _prefetch_u8 / _commit_nv12).
    `.nv12` holds the bytes (n x frame_bytes), `.layout` what the C ABI is told about them; `.frames` is the BGR conversion computed on the
    host on first use, for consumers that want the picture (core.results), and `.asnumpy()` the tensor computed from it."""

    def __init__(self, buf, h, w, pixel_means, target_size, max_size, stride=0, colour="bt601", pitch=None, uv_offset=None, frame_bytes=None, ctx=None,
                 siting="replicate"):
        from ..utils import image
        siting = image.chroma_siting(siting)
        if isinstance(buf, (list, tuple)):
            if len({np.shape(f) for f in buf}) != 1:
                raise ValueError("all frames of one NV12 array must have the same number of bytes")
            buf = np.stack([np.asarray(f).reshape(-1) for f in buf])
            frame_bytes = buf.shape[1] if frame_bytes is None else frame_bytes
        elif np.ndim(buf) == 2 and frame_bytes is None:
            frame_bytes = np.shape(buf)[1]
        lay = image.nv12_layout(h, w, pitch, uv_offset, frame_bytes)
        a = image.nv12_bytes(buf, lay)
        n = a.shape[0]
        pb = None
        if ctx is not None and getattr(ctx, "device_type", "") == "cpu_pinned":
            from .. import runtime
            pb = runtime.PinnedBuffer(a.shape, np.uint8)
            pb.array[...] = a
            nv12 = pb.array
        else:
            nv12 = np.array(a, order="C", copy=True)      # a copy, like mx.nd.array: later edits of the source do not reach it
        nv12.setflags(write=False)
        h, w = lay["h"], lay["w"]
        scale, out_h, out_w, H, W = image.resize_geometry(h, w, target_size, max_size, stride)
        DeviceArray.__init__(self, shape=(n, 3, H, W), fetch=self._host_tensor, pinned=pb)
        self.nv12 = nv12
        self.layout = dict(n=n, colour=image.nv12_colour(colour), **lay)
        self.siting = siting      # how chroma is brought to the luma pixels (utils.image.CHROMA_SITINGS), a number
        self._frames = None
        self.means = tuple(float(v) for v in np.asarray(pixel_means, np.float64).reshape(-1))
        self.resize_args = (target_size, max_size, stride)
        self.scale = scale
        self.geometry = dict(out_h=out_h, out_w=out_w, step=image.resample_step(h, w, scale, out_h, out_w), H=H, W=W)

    @property
    def frames(self):
        """the frames as uint8 n x h x w x 3 BGR, converted on the host on first use"""
        if self._frames is None:
            from ..utils import image
            lay = self.layout
            f = image.nv12_to_bgr_host(self.nv12, lay["h"], lay["w"], lay["pitch"], lay["uv_offset"], lay["frame_bytes"], lay["colour"],
                                       siting=self.siting)
            f.setflags(write=False)
            self._frames = f
        return self._frames

    def __repr__(self):
        return "<NV12Frames %dx%dx%d for %s>" % (self.layout["n"], self.layout["h"], self.layout["w"], "x".join(map(str, self._shape)))


def nv12_frames(buf, h, w, cfg, colour="bt601", pitch=None, uv_offset=None, ctx=None, siting="replicate"):
    """NV12 frames of h x w pixels (uint8 bytes: one flat frame, n x frame_bytes, a flat run of whole frames, or a list of frames) for a
    Predictor: converted with `colour` (utils.image.NV12_COLOURS), resized to cfg.SCALES[0], centred on cfg.network.PIXEL_MEANS and padded
    to cfg.network.IMAGE_STRIDE on the GPU.  pitch: bytes per row (default w); uv_offset: where the chroma plane starts (default
    h * pitch); the bytes from frame to frame are the row length of an n x frame_bytes buffer, else those of one tightly laid-out frame.
    siting: where the chroma samples lie (utils.image.CHROMA_SITINGS): replicate, or left / centre / topleft for interpolated chroma.
    Always a COPY of the bytes; with ctx=mx.cpu_pinned() in page-locked memory."""
    target_size, max_size = cfg.SCALES[0][0], cfg.SCALES[0][1]
    return NV12Frames(buf, h, w, cfg.network.PIXEL_MEANS, target_size, max_size, cfg.network.IMAGE_STRIDE, colour=colour, pitch=pitch,
                      uv_offset=uv_offset, ctx=ctx, siting=siting)


class YUVFrames(RawFrames):
    """Video frames as a software decoder (I420 / YV12), a 10-bit hardware decoder (P010) or a capture card (YUY2) hands them out, standing for
    the same image tensor as the RawFrames of their BGR conversion (utils.image.yuv_to_bgr_host): a Predictor uploads the BYTES -- 1.5, 3 or 2
    per pixel -- and the GPU converts the colour, resizes, removes the mean and pads (accel_model_write_yuv / _prefetch_u8 / _commit_yuv).
    `.yuv` holds the bytes (flat: n frames `frame_bytes` apart), `.layout` what the C ABI is told about them (utils.image.yuv_layout plus n and
    colour); `.frames` is the BGR conversion computed on the host on first use, for consumers that want the picture (core.results), and
    `.asnumpy()` the tensor computed from it."""

    def __init__(self, buf, fmt, h, w, pixel_means, target_size, max_size, stride=0, colour="bt709", ctx=None, siting="replicate", **layout):
        from ..utils import image
        siting = image.chroma_siting(siting)
        if isinstance(buf, (list, tuple)):
            if len({np.shape(f) for f in buf}) != 1 or len({np.asarray(f).dtype for f in buf}) != 1:
                raise ValueError("all frames of one YUV array must have the same number of bytes")
            buf = np.stack([np.asarray(f).reshape(-1) for f in buf])
        if np.ndim(buf) == 2 and layout.get("frame_bytes") is None:
            layout["frame_bytes"] = np.shape(buf)[1] * np.asarray(buf).dtype.itemsize
        lay = image.yuv_layout(fmt, h, w, **layout)
        a, n = image.yuv_bytes(buf, lay)
        pb = None
        if ctx is not None and getattr(ctx, "device_type", "") == "cpu_pinned":
            from .. import runtime
            pb = runtime.PinnedBuffer(a.shape, np.uint8)
            pb.array[...] = a
            yuv = pb.array
        else:
            yuv = np.array(a, order="C", copy=True)      # a copy, like mx.nd.array: later edits of the source do not reach it
        yuv.setflags(write=False)
        h, w = lay["h"], lay["w"]
        scale, out_h, out_w, H, W = image.resize_geometry(h, w, target_size, max_size, stride)
        DeviceArray.__init__(self, shape=(n, 3, H, W), fetch=self._host_tensor, pinned=pb)
        self.yuv = yuv
        self.layout = dict(n=n, colour=image.nv12_colour(colour), **lay)
        self.siting = siting      # how chroma is brought to the luma pixels (utils.image.CHROMA_SITINGS), a number
        self._frames = None
        self.means = tuple(float(v) for v in np.asarray(pixel_means, np.float64).reshape(-1))
        self.resize_args = (target_size, max_size, stride)
        self.scale = scale
        self.geometry = dict(out_h=out_h, out_w=out_w, step=image.resample_step(h, w, scale, out_h, out_w), H=H, W=W)

    @property
    def frames(self):
        """the frames as uint8 n x h x w x 3 BGR, converted on the host on first use"""
        if self._frames is None:
            from ..utils import image
            lay = {k: v for k, v in self.layout.items() if k not in ("n", "colour", "format", "h", "w")}
            f = image.yuv_to_bgr_host(self.yuv, self.layout["format"], self.layout["h"], self.layout["w"], colour=self.layout["colour"],
                                      siting=self.siting, **lay)
            f.setflags(write=False)
            self._frames = f
        return self._frames

    def __repr__(self):
        from ..utils import image
        name = sorted(image.YUV_FORMATS, key=image.YUV_FORMATS.get)[self.layout["format"]]
        return "<YUVFrames %s %dx%dx%d for %s>" % (name, self.layout["n"], self.layout["h"], self.layout["w"], "x".join(map(str, self._shape)))


def yuv_frames(buf, fmt, h, w, cfg, colour="bt709", pitch=None, pitch_c=None, u_offset=None, v_offset=None, frame_bytes=None, ctx=None,
               siting="replicate"):
    """I420, P010 or YUY2 frames (`fmt`: utils.image.YUV_FORMATS) of h x w pixels for a Predictor -- uint8 bytes (uint16 words too for P010): one
    flat frame, n x frame_bytes, a flat run of frames, or a list of frames -- converted with `colour` (utils.image.NV12_COLOURS), resized to
    cfg.SCALES[0], centred on cfg.network.PIXEL_MEANS and padded to cfg.network.IMAGE_STRIDE on the GPU.  The layout keywords are those of
    utils.image.yuv_layout (tightly packed where nothing is given; the bytes from frame to frame default to the row length of an
    n x frame_bytes buffer).  siting: where the chroma samples lie (utils.image.CHROMA_SITINGS): replicate, or left / centre / topleft for
    interpolated chroma.  Always a COPY of the bytes; with ctx=mx.cpu_pinned() in page-locked memory."""
    target_size, max_size = cfg.SCALES[0][0], cfg.SCALES[0][1]
    return YUVFrames(buf, fmt, h, w, cfg.network.PIXEL_MEANS, target_size, max_size, cfg.network.IMAGE_STRIDE, colour=colour, ctx=ctx, pitch=pitch,
                     pitch_c=pitch_c, u_offset=u_offset, v_offset=v_offset, frame_bytes=frame_bytes, siting=siting)


def zeros(shape, ctx=None, dtype=np.float32):
    return DeviceArray(host=np.zeros(shape, dtype))


def argmax(arr, axis=1):
    """mx.ndarray.argmax(out, axis=1): when `arr` is a logits buffer produced by
    the fused score kernel the label map already exists in HBM (the kernel
    writes logits and first-max labels together); otherwise reduce on the host."""
    if isinstance(arr, DeviceArray) and arr.labels_of is not None and axis == 1:
        return arr.labels_of()
    a = arr.asnumpy() if isinstance(arr, DeviceArray) else np.asarray(arr)
    return DeviceArray(host=np.argmax(a, axis=axis).astype(np.float32))


class DataBatch(object):
    """mx.io.DataBatch as built at demo.py:210-212,229-231."""

    def __init__(self, data, label=None, pad=0, index=None, provide_data=None, provide_label=None):
        self.data = data
        self.label = label
        self.pad = pad
        self.index = index
        self.provide_data = provide_data
        self.provide_label = provide_label
