"""Finishing a frame on the GPU: the label map `mx.nd.argmax(logits)` returns, taken back to the source frame's size there and handed
over as labels, as a colour image or as counts in a confusion matrix (csrc/results_u8.hip behind accel_model_labels_to_source /
_labels_colour / _hist_add / _hist_read) -- and the logits themselves finished as a per-pixel confidence (csrc/confidence.hip behind
accel_model_confidence), or as labels of their own: `interpolate=True` takes the LOGITS handle, interpolates the scores bilinearly to the
source size and takes the argmax there (csrc/scores_labels.hip behind accel_model_scores_labels / _scores_hist_add / _scores_colour), and
`confidence(..., interpolate=True)` takes the confidence from those interpolated scores too, with the labels if asked, in one pass
(the interpolated form of csrc/confidence.hip behind accel_model_confidence_interp).  `overlay` blends the labels over NV12 / I420 / P010 / YUY2 frames and
hands back the frames' own format (csrc/overlay_yuv.hip behind accel_model_labels_overlay_yuv / _scores_overlay_yuv).  `summary` says what
is in the frame, where, and whether it just changed: per-class areas, coordinate sums and boxes, and the class transitions against the
previous frame, which is kept in HBM (csrc/labels_summary.hip behind accel_model_labels_summary / _scores_summary / _labels_forget).
`components` says how many objects of every class there are and where each one is: the connected components of the label map with their
area, box, first pixel and coordinate sums, in raster order, and the object index per pixel if asked (csrc/labels_components.hip behind
accel_model_labels_components / _scores_components).
`TrimapEvaluator` counts the confusion matrix in bands around the ground truth's boundaries, where propagated features are damaged first, and
`boundary_distance` gives the distance map itself (csrc/labels_band.hip behind accel_model_band_hist_add / _scores_band_hist_add /
_band_hist_read and accel_boundary_distance).

The reference fetches the label map and does all of this in numpy (demo.py:245-266: `.asnumpy()`, fast_hist, the palette PNG); its
evaluator resizes a prediction to the ground truth with nearest neighbour (lib/dataset/cityscape.py:227).  Here the prediction is at the
padded, resized size H x W a network fed with raw frames is bound at (mx.nd.raw_frames), the ground truth and the viewer are at the
camera's h x w, and `RawFrames.geometry` says how to get back.

A label handle names a buffer, not a copy: its `device_ref` is (model, "labels", write generation).  Every function here checks that
generation first -- stale labels are never read."""
import collections

import numpy as np

from .. import runtime
from ..utils.image import summary_centroids, summary_churn  # noqa: F401  (re-exported: the host helpers of `summary`)
from ..utils.image import components_centroids, components_of  # noqa: F401  (re-exported: the host helpers of `components`)


def _geometry(handle, like, hw=None, scores=False):
    """(n, out_h, out_w, h, w) of a finishing call.  `like`: a RawFrames array (its frames' size and the resize it stands for), a
    dict with out_h, out_w and h, w (other keys, such as those of RawFrames.geometry, are ignored; h, w default to `hw`), or None:
    the whole H x W map is valid and is resized to `hw`.  scores: the handle is a logits handle, n x ncls x H x W."""
    shape = tuple(handle.shape)
    if scores:
        if len(shape) != 4:
            raise ValueError("a logits handle is n x ncls x H x W, got shape %s" % (shape,))
        shape = (shape[0],) + shape[2:]
    elif len(shape) != 3:
        raise ValueError("a label handle is n x H x W, got shape %s" % (shape,))
    n, H, W = shape
    if like is None:
        out_h, out_w, src = H, W, hw or (H, W)
    elif isinstance(like, dict):
        out_h, out_w = like["out_h"], like["out_w"]
        src = (like["h"], like["w"]) if "h" in like and "w" in like else hw
        if src is None:
            raise ValueError("the geometry dict has no source size: add h and w")
    else:
        out_h, out_w = like.geometry["out_h"], like.geometry["out_w"]
        src = tuple(like.frames.shape[1:3])
    if hw is not None and tuple(hw) != tuple(src):
        raise ValueError("the ground truth is %d x %d, the source frames are %d x %d" % (hw[0], hw[1], src[0], src[1]))
    return n, int(out_h), int(out_w), int(src[0]), int(src[1])


def _model(handle, buffer="labels"):
    """the model whose `buffer` (`labels`, or `logits`) the handle stands for -- still holding what the handle was made for, or AccelError"""
    ref = getattr(handle, "device_ref", None)
    if not ref or ref[1] != buffer:
        if buffer == "labels":
            raise runtime.AccelError("not a label handle of the GPU path (mx.nd.argmax of a Predictor's logits): nothing to finish on the GPU")
        raise runtime.AccelError("not a %s handle of the GPU path (an output of Predictor.predict): nothing to finish on the GPU" % buffer)
    m, buf, gen = ref
    if m.generation(buf) != gen:
        what = "label" if buffer == "labels" else buffer
        raise runtime.AccelError("this %s handle is stale: its buffer has been written since (fetch it with .asnumpy(), or finish "
                                 "the frame, before the next forward that writes %s)" % (what, buffer))
    return m


def labels_at_source(handle, like, interpolate=False):
    """The labels of `handle` at the source frames' size: numpy n x h x w uint8 (utils.image.labels_to_source_host, on the GPU).
    interpolate=True: `handle` is the LOGITS handle of the frame; its scores are interpolated bilinearly to the source size and the
    argmax is taken there (utils.image.labels_interpolated_host, on the GPU)."""
    if interpolate:
        m = _model(handle, "logits")
        n, out_h, out_w, h, w = _geometry(handle, like, scores=True)
        return m.scores_labels(n, out_h, out_w, h, w)
    m = _model(handle)
    n, out_h, out_w, h, w = _geometry(handle, like)
    return m.labels_to_source(n, out_h, out_w, h, w)


def colour(handle, like, palette, frames=None, alpha=256, rgb=True, interpolate=False):
    """The labels of `handle` as a colour image at the source frames' size: numpy n x h x w x 3 uint8, palette[label] (256 x 3 R, G, B)
    in R, G, B order (rgb=True) or B, G, R; blended over `frames` (uint8 n x h x w x 3 BGR; frames=True takes those of a RawFrames
    `like`) with weight alpha / 256 (utils.image.colour_host, on the GPU).  interpolate=True: `handle` is the LOGITS handle and the
    labels are those of labels_at_source(handle, like, interpolate=True)."""
    m = _model(handle, "logits" if interpolate else "labels")
    n, out_h, out_w, h, w = _geometry(handle, like, scores=bool(interpolate))
    if frames is True:
        frames = like.frames
    if interpolate:
        return m.scores_colour(n, out_h, out_w, h, w, palette, frames=frames, alpha=alpha, rgb=rgb)
    return m.labels_colour(n, out_h, out_w, h, w, palette, frames=frames, alpha=alpha, rgb=rgb)


def overlay(handle, like, palette, alpha=128, interpolate=False):
    """The labels of `handle` blended over the frames of `like` IN THEIR OWN FORMAT: `like` is the NV12Frames or YUVFrames array the network was
    fed with, and the result is its bytes -- the shape and dtype of `like.nv12` / `like.yuv`, the same layout, gaps included -- with every sample
    blended with weight alpha / 256 towards palette[label] (256 x 3 R, G, B, taken to Y, Cb, Cr once with `like`'s colour mode:
    utils.image.palette_ycbcr; the per-sample rule is utils.image.overlay_yuv_host, on the GPU: csrc/overlay_yuv.hip).  What an encoder or a
    compositor takes; no BGR picture is made on the way.  The overlay's chroma is the mean of the palette colours over the pixels a chroma
    sample covers, whatever `like.siting` is: the frame's own samples are blended where they are and are not resited.
    interpolate=True: `handle` is the LOGITS handle and the labels are those of labels_at_source(handle, like, interpolate=True)."""
    from ..mx.ndarray import NV12Frames, YUVFrames
    from ..utils import image
    if not isinstance(like, (NV12Frames, YUVFrames)):
        raise ValueError("overlay writes NV12, I420, P010 or YUY2 frames in their own format: `like` must be an NV12Frames or a YUVFrames array, "
                         "got %s (for a BGR / RGB picture use results.colour)" % type(like).__name__)
    m = _model(handle, "logits" if interpolate else "labels")
    lay = like.layout
    # (the source size from the layout: `like.frames` would convert the frames to BGR on the host, for nothing)
    n, out_h, out_w, h, w = _geometry(handle, dict(like.geometry, h=lay["h"], w=lay["w"]), scores=bool(interpolate))
    if isinstance(like, NV12Frames):
        buf, fmt = like.nv12, 3
        keys = dict(pitch=lay["pitch"], u_offset=lay["uv_offset"], frame_bytes=lay["frame_bytes"])
    else:
        buf, fmt = like.yuv, lay["format"]
        keys = {k: lay[k] for k in ("pitch", "pitch_c", "u_offset", "v_offset", "frame_bytes")}
    table = image.palette_ycbcr(palette, lay["colour"], bits=10 if fmt == 1 else 8)
    run = m.scores_overlay_yuv if interpolate else m.labels_overlay_yuv
    return run(n, out_h, out_w, buf, fmt, h, w, table, alpha=alpha, **keys)


def confidence(handle, like, margin=False, second=False, hist=False, probabilities=None, interpolate=False, labels=False):
    """How sure the network was, per source pixel, from the LOGITS handle a Predictor returned (not the label handle): conf, numpy
    n x h x w uint8 = min(255, floor(256 * largest softmax probability)) -- or the tuple (conf[, margin][, second][, hist]) with what
    was asked for: margin n x h x w float32 = top score - runner-up score, second n x h x w uint8 = the runner-up class, hist
    n x 256 uint64 = pixels per conf level of each frame (utils.image.confidence_host, on the GPU: the scores of the nearest map pixel,
    pixel for pixel with labels_at_source under the nearest rule).  probabilities: the stored scores are probabilities already (a tail
    lowered with softmax=1); None takes the answer from the handle.
    interpolate=True: everything is taken from the scores interpolated bilinearly to the source pixel, pixel for pixel with
    labels_at_source(handle, like, interpolate=True) (utils.image.confidence_interpolated_host, on the GPU, one pass over the logits).
    labels=True (needs interpolate=True; under the nearest rule the label handle already exists) prepends that label map, n x h x w uint8:
    (labels, conf[, margin][, second][, hist])."""
    if labels and not interpolate:
        raise ValueError("labels=True needs interpolate=True: under the nearest rule the labels are those of the label handle (labels_at_source)")
    m = _model(handle, "logits")
    n, out_h, out_w, h, w = _geometry(handle, like, scores=True)
    if probabilities is None:
        probabilities = bool(getattr(handle, "probabilities", False))
    want = dict(is_prob=probabilities, conf=True, margin=bool(margin), second=bool(second), hist=bool(hist))
    if interpolate:
        out = m.confidence_interp(n, out_h, out_w, h, w, labels=bool(labels), **want)
    else:
        out = m.confidence(n, out_h, out_w, h, w, **want)
    out = tuple(a for a in out if a is not None)
    return out[0] if len(out) == 1 else out


Summary = collections.namedtuple("Summary", "stats box trans")


def summary(handle, like, ncls=19, track=False, interpolate=False, box=True):
    """What is in the frame, where, and did it just change, from the labels of `handle` at the source frames' size without fetching them:
    Summary(stats, box, trans) -- stats n x ncls x 3 uint64 = (area, sum_x, sum_y) per frame and class (summary_centroids gives the
    centroids, area / (h * w) the share of the frame), box n x ncls x 4 int32 = the inclusive (x0, y0, x1, y1) of every class, (w, h, -1, -1)
    for an absent one (None with box=False), ids >= ncls ignored (utils.image.labels_summary_host, on the GPU: csrc/labels_summary.hip).
    track=True also compares with the previous tracked frame of the same model, kept at the source size in HBM: trans is n x (ncls * ncls)
    uint64, rows the previous frame's class, columns this frame's (summary_churn gives the churn, per_class_iu of the square matrix the
    temporal IoU) -- or None where there was nothing to compare with: the first tracked frame, after forget(), or after a change of frame
    size, batch or ncls.  interpolate=True: `handle` is the LOGITS handle and the labels are those of
    labels_at_source(handle, like, interpolate=True)."""
    m = _model(handle, "logits" if interpolate else "labels")
    n, out_h, out_w, h, w = _geometry(handle, like, scores=bool(interpolate))
    run = m.scores_summary if interpolate else m.labels_summary
    return Summary(*run(n, out_h, out_w, h, w, int(ncls), track=bool(track), stats=True, box=bool(box)))


Components = collections.namedtuple("Components", "count comp sums ids")


def components(handle, like, ncls=19, connectivity=8, min_area=1, max_components=1024, ids=False, interpolate=False):
    """The objects of every class, from the labels of `handle` at the source frames' size without fetching them: Components(count, comp, sums,
    ids) of the connected components of equal labels < ncls (4- or 8-connected; ids >= ncls are background and separate components) with at
    least min_area pixels, in raster order of their first pixel -- count n int32 = their number per frame (the full number, also above
    max_components), comp n x max_components x 8 int32 = (class, area, x0, y0, x1, y1, ax, ay) with the inclusive box and the first pixel, -1 in
    the unused records, sums n x max_components x 2 uint64 = (sum_x, sum_y) (components_centroids gives the centroids, components_of the
    trimmed records of one frame), ids n x h x w int32 = the record index per source pixel or -1 (None with ids=False)
    (utils.image.labels_components_host, on the GPU: csrc/labels_components.hip).  interpolate=True: `handle` is the LOGITS handle, the labels
    are those of labels_at_source(handle, like, interpolate=True) and ncls must be the class count of the scores."""
    m = _model(handle, "logits" if interpolate else "labels")
    n, out_h, out_w, h, w = _geometry(handle, like, scores=bool(interpolate))
    run = m.scores_components if interpolate else m.labels_components
    return Components(*run(n, out_h, out_w, h, w, int(ncls), connectivity=int(connectivity), min_area=int(min_area),
                           max_components=int(max_components), comp=True, sums=True, ids=bool(ids)))


def forget(handle):
    """Drop the map that summary(..., track=True) keeps in the model of `handle` (a label or a logits handle, stale or not: nothing of it
    is read): call it at the start of a clip or after a cut, so that the first frame is not compared with the last one of another scene."""
    ref = getattr(handle, "device_ref", None)
    if not ref:
        raise runtime.AccelError("not a handle of the GPU path: there is no kept map to forget")
    ref[0].labels_forget()


def confidence_summary(hist, level=128):
    """(mean confidence as a probability: the centre of every level's interval weighted by its count; share of pixels below `level`)
    of one frame's 256 counts"""
    c = np.asarray(hist, np.float64).reshape(256)
    total = c.sum()
    if total <= 0:
        return float("nan"), float("nan")
    return float((c * (np.arange(256) + 0.5) / 256.0).sum() / total), float(c[:int(level)].sum() / total)


def per_class_iu(hist):
    """demo.py:55-56"""
    hist = np.asarray(hist, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))


class Evaluator(object):
    """mIoU bookkeeping of the demo loop (fast_hist per frame, summed) with the counting on the GPU: `add` enqueues one kernel that
    takes the prediction to the ground truth's size and adds to a confusion matrix that lives in the model; nothing but the ground
    truth crosses PCIe until `hist()`.  One accumulator per model: the evaluator adopts the model of the first handle it is given
    and reports what was added since then (the accumulator's content at that moment is its zero)."""

    def __init__(self, num_classes):
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= 32:
            raise ValueError("num_classes = %d, must be in 1 .. 32" % self.num_classes)
        self._m = None
        self._base = np.zeros((self.num_classes, self.num_classes), np.int64)

    def add(self, handle, gt, like=None, interpolate=False):
        """count `handle`'s labels against ground truth `gt` ([n x] h x w uint8; ids >= num_classes, such as 255, are ignored).
        interpolate=True: `handle` is the LOGITS handle and the labels are those of labels_at_source(handle, like, interpolate=True)"""
        m = _model(handle, "logits" if interpolate else "labels")
        if self._m is None:
            self._base = m.hist_read(self.num_classes).astype(np.int64)
            self._m = m
        elif m is not self._m:
            raise runtime.AccelError("this evaluator accumulates in another model: one Evaluator per model")
        g = np.asarray(gt)
        if g.ndim == 2:
            g = g[None]
        if g.dtype != np.uint8:
            g = np.where((g >= 0) & (g < 256), g, 255).astype(np.uint8)      # anything outside a byte is ignored either way
        n, out_h, out_w, h, w = _geometry(handle, like, hw=g.shape[1:3], scores=bool(interpolate))
        if g.shape[0] != n:
            raise ValueError("%d label maps but %d ground-truth maps" % (n, g.shape[0]))
        if interpolate:
            m.scores_hist_add(g, out_h, out_w, self.num_classes)
        else:
            m.hist_add(g, out_h, out_w, self.num_classes)

    def hist(self, clear=False):
        """the confusion matrix so far: int64 num_classes x num_classes, rows ground truth, columns prediction (waits for the GPU)"""
        if self._m is None:
            return np.zeros((self.num_classes, self.num_classes), np.int64)
        out = self._m.hist_read(self.num_classes, clear=clear).astype(np.int64) - self._base
        if clear:
            self._base[...] = 0
        return out

    def per_class_iu(self):
        return per_class_iu(self.hist())


def boundary_distance(maps, cap, ctx=None):
    """The distance of every pixel of label maps ([n x] h x w uint8: ground truth, or fetched predictions) to the nearest boundary: numpy n x h x w
    uint8 = min(cap, Chebyshev distance to the nearest pixel with a differing 4-neighbour), cap in 1 .. 16 (utils.image.boundary_distance_host, on
    the GPU: csrc/labels_band.hip behind accel_boundary_distance).  d == 0 is the outline a viewer draws, d < k the band a trimap of width k counts
    in.  ctx: the runtime.Context to run on; None opens one on device 0 for the call."""
    if ctx is not None:
        return ctx.boundary_distance(maps, cap)
    own = runtime.Context(0)
    try:
        return own.boundary_distance(maps, cap)
    finally:
        own.close()


class TrimapEvaluator(object):
    """mIoU restricted to bands around the ground truth's boundaries, against the band width (the trimap of the DeepLab papers), counted on the GPU:
    `add` enqueues one kernel that takes the prediction to the ground truth's size, measures every pixel's distance to the nearest ground-truth
    boundary and adds to one confusion matrix per distance bucket in the model (csrc/labels_band.hip behind accel_model_band_hist_add /
    _scores_band_hist_add / _band_hist_read; utils.image.band_hist_host).  widths: 1 to 4 strictly ascending band widths in pixels, 1 .. 16.  The
    accumulator is the model's band accumulator, separate from the one `Evaluator` uses: both may run on one model.  The evaluator adopts the model
    of the first handle it is given and reports what was added since then."""

    def __init__(self, num_classes, widths=(1, 2, 4, 8)):
        from ..utils.image import band_widths
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= 32:
            raise ValueError("num_classes = %d, must be in 1 .. 32" % self.num_classes)
        self.widths = band_widths(widths)
        self._m = None
        self._base = np.zeros((len(self.widths) + 1, self.num_classes, self.num_classes), np.int64)

    def add(self, handle, gt, like=None, interpolate=False):
        """count `handle`'s labels against ground truth `gt` ([n x] h x w uint8; ids >= num_classes, such as 255, are ignored as classes and
        still make boundaries).  interpolate=True: `handle` is the LOGITS handle and the labels are those of
        labels_at_source(handle, like, interpolate=True)"""
        m = _model(handle, "logits" if interpolate else "labels")
        if self._m is None:
            self._base = m.band_hist_read(self.num_classes, len(self.widths)).astype(np.int64)
            self._m = m
        elif m is not self._m:
            raise runtime.AccelError("this evaluator accumulates in another model: one TrimapEvaluator per model")
        g = np.asarray(gt)
        if g.ndim == 2:
            g = g[None]
        if g.dtype != np.uint8:
            g = np.where((g >= 0) & (g < 256), g, 255).astype(np.uint8)      # anything outside a byte is ignored either way
        n, out_h, out_w, h, w = _geometry(handle, like, hw=g.shape[1:3], scores=bool(interpolate))
        if g.shape[0] != n:
            raise ValueError("%d label maps but %d ground-truth maps" % (n, g.shape[0]))
        if interpolate:
            m.scores_band_hist_add(g, out_h, out_w, self.num_classes, self.widths)
        else:
            m.band_hist_add(g, out_h, out_w, self.num_classes, self.widths)

    def buckets(self, clear=False):
        """the counts per distance bucket so far: int64 (K + 1) x num_classes x num_classes (waits for the GPU)"""
        if self._m is None:
            return np.zeros_like(self._base)
        out = self._m.band_hist_read(self.num_classes, len(self.widths), clear=clear).astype(np.int64) - self._base
        if clear:
            self._base[...] = 0
        return out

    def hist(self, clear=False):
        """int64 (K + 1) x num_classes x num_classes, rows ground truth, columns prediction: [k] is the BAND of width widths[k] (cumulative),
        [K] the whole frame"""
        return self.cumulative(self.buckets(clear=clear))

    @staticmethod
    def cumulative(buckets):
        from ..utils.image import band_cumulative
        return band_cumulative(buckets)

    @staticmethod
    def iu_of(hist):
        """per_class_iu of every matrix of a (K + 1) x ncls x ncls array: (K + 1) x ncls"""
        return np.stack([per_class_iu(h) for h in np.asarray(hist)])

    @staticmethod
    def miou_of(hist):
        """the mean IoU over the classes present in every matrix of a (K + 1) x ncls x ncls array: K + 1 floats, nan where a matrix is empty"""
        iu = TrimapEvaluator.iu_of(hist)
        out = np.full(iu.shape[0], np.nan)
        some = ~np.isnan(iu).all(axis=1)
        out[some] = np.nanmean(iu[some], axis=1)
        return out

    def per_class_iu(self):
        return self.iu_of(self.hist())

    def miou(self):
        """K + 1 floats: the mIoU inside the band of every width, then of the whole frame; nan where a band holds no counted pixel"""
        return self.miou_of(self.hist())
