"""Accel inference + mIoU + timing harness: the counterpart of
dff_deeplab/demo.py (the only working segmentation harness of the reference,
SURVEY.md F2), on the HIP runtime.

    python -m accel_amd.demo --version 18 --interval 5 --num_ex 10 [--avg]
                             [--data DIR --labels DIR | --synthetic HxW]
                             [--params accel-18-0000.params flownet-0000.params]

Reproduced behaviour (demo.py:107-284): frame selection (`lb_pos = 19`,
`offset = interval-1` or `i % interval` with --avg), key/non-key schedule
(`idx % interval == 0`), `data_key` = PREVIOUS frame, feature feedback,
`correction_output` vs `croped_score_output` (Accel-101), 2 warm-up frames,
tic/toc around forward + argmax + label-map fetch, fast_hist/per_class_iu mIoU.
Without Cityscapes on disk the clip source is synthetic (`--synthetic`).
"""
import argparse
import glob
import os

import numpy as np

from . import mx
from .config.config import config, update_config
from .core.tester import Predictor, im_segment
from .utils.image import CHROMA_SITINGS, NV12_COLOURS, YUV_FORMATS, bgr_to_nv12_host, bgr_to_yuv_host, resize, transform
from .utils.tictoc import tic, toc


def fast_hist(pred, label, n):
    """demo.py:50-53"""
    k = (label >= 0) & (label < n)
    return np.bincount(n * label[k].astype(int) + pred[k], minlength=n ** 2).reshape(n, n)


def per_class_iu(hist):
    """demo.py:55-56"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))


def select_frames(image_names, num_ex, interv, avg_acc, snip_len=30, lb_pos=19):
    """demo.py:152-163: per 30-frame snippet keep `interv` frames positioned so
    that the labelled frame (index 19) is `offset` frames after the key frame."""
    out = []
    for i in range(num_ex):
        snip_pos = i * snip_len
        offset = i % interv if avg_acc else interv - 1
        start_pos = lb_pos - offset
        out.extend(image_names[snip_pos + start_pos: snip_pos + start_pos + interv])
    return out


def label_key(path):
    """(city, sequence, frame) of a Cityscapes file name `<city>_<seq>_<frame>_<suffix>.png` -- the city is part of the
    key: lindau_0000NN_000019 and munster_0000NN_000019 both exist in val for NN = 0..58 (the reference walks the label
    list in order with lb_idx instead, demo.py:140-150,262-266)."""
    c = os.path.basename(path).split('_')
    return tuple(c[:3]) if len(c) > 3 else None


def get_symbols(version, cfg):
    from . import symbols
    name = "accel_" + str(version)
    inst = getattr(getattr(symbols, name), name)()
    return inst, inst.get_key_test_symbol(cfg), inst.get_cur_test_symbol(cfg)


def build_batches(frames_bgr, cfg, pinned=False, raw=False, nv12=None, yuv=None, yuv_colour='bt709', siting='replicate'):
    """demo.py:165-190: list of [data, data_key, feat_key] arrays per frame.

    One array per frame serves as this frame's `data` and as the next frame's `data_key` (the reference builds two
    NDArrays from the same image, demo.py:176-181): arrays are immutable, so the Predictor recognises the object it
    uploaded one call earlier and copies the image inside HBM instead of sending it over PCIe twice.
    pinned=True places the images in page-locked memory (mx.cpu_pinned()), the source of overlapped uploads.
    raw=True keeps every frame as its uint8 BGR bytes (mx.nd.raw_frames): no fp32 image is built on the host, a quarter of
    the bytes cross PCIe and the GPU resizes, removes the mean and pads (accel_model_write_u8).
    nv12=<colour mode> (utils.image.NV12_COLOURS) feeds every frame as NV12 bytes (mx.nd.nv12_frames), as a video decoder would hand it
    out -- bgr_to_nv12_host stands in for the decoder; an eighth of the bytes cross PCIe and the GPU converts the colour as well.
    yuv=<format> (utils.image.YUV_FORMATS) feeds every frame as I420, P010 or YUY2 bytes (mx.nd.yuv_frames) converted with `yuv_colour`, the
    same way -- bgr_to_yuv_host stands in for the decoder or the capture card.
    siting=<name> (utils.image.CHROMA_SITINGS), with nv12 or yuv: the stand-in decoder sites its chroma samples that way and the GPU interpolates
    them back accordingly; replicate: samples made as block means (centre) and replicated, as ever."""
    if siting not in CHROMA_SITINGS:
        raise ValueError("siting = %r, must be one of %s" % (siting, ", ".join(sorted(CHROMA_SITINGS))))
    made = 'centre' if siting == 'replicate' else siting      # how the stand-in decoder sites its samples
    data, prev = [], None
    ctx = mx.cpu_pinned() if pinned else None
    zero_feat = mx.nd.array(np.zeros((1, cfg.network.DFF_FEAT_DIM, 1, 1)))
    for im in frames_bgr:
        if nv12 is not None:
            h, w = im.shape[:2]
            if h % 2 or w % 2:
                raise ValueError("--nv12: NV12 frames have an even height and width, this frame is %d x %d (odd-sized)" % (h, w))
            cur = mx.nd.nv12_frames(bgr_to_nv12_host(im, nv12, siting=made), h, w, cfg, colour=nv12, ctx=ctx, siting=siting)
        elif yuv is not None:
            h, w = im.shape[:2]
            if h % 2 or w % 2:
                raise ValueError("--yuv: the %s frames made here have an even height and width, this frame is %d x %d (odd-sized)" % (yuv, h, w))
            cur = mx.nd.yuv_frames(bgr_to_yuv_host(im, yuv, yuv_colour, siting=made), yuv, h, w, cfg, colour=yuv_colour, ctx=ctx, siting=siting)
        elif raw:
            cur = mx.nd.raw_frames(im, cfg, ctx=ctx)
        else:
            target_size, max_size = cfg.SCALES[0][0], cfg.SCALES[0][1]
            im, _ = resize(im, target_size, max_size, stride=cfg.network.IMAGE_STRIDE)
            cur = mx.nd.array(transform(im, cfg.network.PIXEL_MEANS), ctx=ctx)
        if prev is None:
            prev = cur
        data.append([cur, prev, zero_feat])
        prev = cur
    return data


class ClipRunner(object):
    """The demo.py hot loop as an object: a key and a cur Predictor sharing one device."""

    data_names = ['data', 'data_key', 'feat_key']

    _tags = 0

    def __init__(self, version, cfg, arg_params, aux_params, frame_hw, context=None, model=None, batch=1, share_models=False):
        """`model`: bind both predictors on this runtime.Model (the bench does).  Otherwise the runner's two predictors
        share models with each other only -- two runners interleaving clips of the same size do not see each other's
        propagated feature -- unless share_models=True (one model per device, size and parameter content, as for
        predictors built directly)."""
        self.version = str(version)
        ClipRunner._tags += 1
        self.owner = None if (share_models or model is not None) else "cliprunner-%d" % ClipRunner._tags
        self.cfg = cfg
        H, W = frame_hw
        _, key_sym, cur_sym = get_symbols(version, cfg)
        ctx = context or [mx.gpu(0)]
        B = int(batch)      # frames per call: one frame of each of B independent clips (throughput mode)
        max_shape = [[('data', (B, 3, H, W)), ('data_key', (B, 3, H, W))]]
        provide = [[('data', (B, 3, H, W)), ('data_key', (B, 3, H, W)), ('feat_key', (B, 2048, 1, 1))]]
        self.key_predictor = Predictor(key_sym, self.data_names, [], context=ctx, max_data_shapes=max_shape,
                                       provide_data=provide, provide_label=[None],
                                       arg_params=arg_params, aux_params=aux_params, model=model, owner=self.owner)
        self.cur_predictor = Predictor(cur_sym, self.data_names, [], context=ctx, max_data_shapes=max_shape,
                                       provide_data=provide, provide_label=[None],
                                       arg_params=arg_params, aux_params=aux_params, model=model, owner=self.owner)
        self.feat = None
        self.last_key, self.last_change = None, None      # what the last step did (see step)
        self.output_key = 'croped_score_output' if self.version in ('101', 'dff') else 'correction_output'

    def close(self):
        """release the models this runner owns (no-op for shared / explicit models)"""
        if self.owner is not None:
            from .core import tester
            tester.release_models(self.owner)

    def prefetch(self, arrays):
        """start the upload of the NEXT frame's image (page-locked arrays only) beside the running forward"""
        return self.key_predictor.prefetch(arrays[0])

    def _decide(self, idx, arrays, batch, schedule):
        """With a schedule: the images are staged into HBM (Predictor.stage: what predict() would do, so the predictor chosen afterwards moves
        nothing), `data` is measured against the frame kept at the last key frame (accel_model_frame_change) when the schedule looks at frames,
        the schedule decides, and on a key frame the frame's signature becomes the kept one."""
        self.last_change = None
        if not schedule.needs_change:
            return schedule.decide(idx)
        for name, a in zip(self.data_names[:2], arrays[:2]):
            if getattr(a, "uid", None) is None:
                raise ValueError("the adaptive schedule stages the frame before it chooses a predictor, and `%s` is an array without identity "
                                 "(plain numpy): it could not be recognised as staged and would be uploaded twice; wrap it with mx.nd.array / "
                                 "mx.nd.raw_frames" % name)
        data = arrays[0]
        m = self.cur_predictor.stage(batch)
        n, H, W = data.shape[0], data.shape[2], data.shape[3]
        g = getattr(data, "geometry", None)      # raw frames: the valid region inside the padded size
        out_h, out_w = (g["out_h"], g["out_w"]) if g else (H, W)
        got = m.frame_change("data", n, out_h, out_w, schedule.cell, schedule.level_q)
        if got is not None:
            cells = (-(-out_h // schedule.cell)) * (-(-out_w // schedule.cell))
            self.last_change = [(int(c), cells, int(s)) for c, s in zip(got[0], got[1])]
        key = schedule.decide(idx, self.last_change)
        if key:
            m.frame_keep()
        return key

    def step(self, idx, arrays, interval, schedule=None):
        """One frame (demo.py:235-245).  Returns (logits handle, label-map handle).  schedule=None: a key frame at idx % interval == 0, the
        reference's loop; a core.schedule.KeySchedule decides otherwise (`interval` is then not looked at) and `last_key` / `last_change`
        (per frame (changed cells, cells, sad), or None where nothing was compared) say what happened."""
        batch = mx.io.DataBatch(data=[list(arrays)], label=[], pad=0, index=idx,
                                provide_data=[[(k, v.shape) for k, v in zip(self.data_names, arrays)]],
                                provide_label=[None])
        if schedule is not None:
            self.last_key = self._decide(idx, arrays, batch, schedule)
        else:
            self.last_key = idx % interval == 0
        if self.last_key:
            output_all, self.feat = im_segment(self.key_predictor, batch)
            logits = output_all[0]['croped_score_output']
        else:
            batch.data[0][-1] = self.feat
            batch.provide_data[0][-1] = ('feat_key', self.feat.shape)
            output_all, self.feat = im_segment(self.cur_predictor, batch)
            logits = output_all[0][self.output_key]
        return logits, mx.nd.argmax(logits, axis=1)


def run_clip(version, cfg, arg_params, aux_params, frames_bgr, interval, want_logits=True):
    """Runs the demo schedule over `frames_bgr`; returns per-frame (logits, labels) numpy."""
    data = build_batches(frames_bgr, cfg)
    H, W = data[0][0].shape[2:]
    runner = ClipRunner(version, cfg, arg_params, aux_params, (H, W))
    outs = []
    for idx, arrays in enumerate(data):
        logits, labels = runner.step(idx, arrays, interval)
        lab = np.uint8(np.squeeze(labels.asnumpy()))
        outs.append((logits.asnumpy() if want_logits else None, lab))
    return outs


def _trimap_widths(text):
    """--trimap: '1,2,4,8' -> (1, 2, 4, 8)"""
    from .utils.image import band_widths
    try:
        return band_widths(int(v) for v in text.split(','))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def main(argv=None):
    ap = argparse.ArgumentParser(description='Accel demo (MI355X)')
    ap.add_argument('--version', default='18')
    ap.add_argument('--interval', type=int, default=5)
    ap.add_argument('--num_ex', type=int, default=10)
    ap.add_argument('--avg', dest='avg_acc', action='store_true')
    ap.add_argument('--cfg', default=None, help='experiments/dff_deeplab/cfgs/dff_deeplab_vid_demo.yaml')
    ap.add_argument('--data', default='', help='Cityscapes root (leftImg8bit_sequence/, gtFine/)')
    ap.add_argument('--synthetic', default='1024x2048')
    ap.add_argument('--params', nargs='*', default=[], help='MXNet .params checkpoints, merged in order')
    ap.add_argument('--out', default='', help='directory for palette PNGs seg_<frame>.png (demo.py:252-257)')
    ap.add_argument('--pageable', action='store_true',
                    help='frames in pageable host memory, uploaded synchronously inside each forward (the reference\'s '
                         'loop one to one); default: page-locked frames, the next frame\'s upload overlaps the current forward')
    ap.add_argument('--raw-frames', dest='raw_frames', action='store_true',
                    help='upload the frames as uint8 BGR bytes and resize / mean-subtract / pad them on the GPU: no fp32 image '
                         'is built on the host')
    ap.add_argument('--nv12', nargs='?', const='bt601', default=None, choices=sorted(NV12_COLOURS),
                    help='feed the frames as NV12 bytes, the format video decoders hand out (implies --raw-frames): the frames, of even '
                         'height and width, are turned into NV12 on the host (standing in for a decoder) and the GPU converts the colour '
                         'with the named matrix, resizes, mean-subtracts and pads')
    ap.add_argument('--yuv', default=None, choices=sorted(YUV_FORMATS),
                    help='feed the frames as I420 (software decoders), P010 (10-bit hardware decoders) or YUY2 (capture cards) bytes (implies '
                         '--raw-frames, excludes --nv12): the frames, of even height and width, are turned into that format on the host and '
                         'the GPU converts the colour with the matrix of --yuv-colour, resizes, mean-subtracts and pads')
    ap.add_argument('--yuv-colour', dest='yuv_colour', default='bt709', choices=sorted(NV12_COLOURS), help='the colour mode of --yuv')
    ap.add_argument('--chroma-siting', dest='chroma_siting', default='replicate', choices=sorted(CHROMA_SITINGS, key=CHROMA_SITINGS.get),
                    help='with --nv12 or --yuv: where the chroma samples of the frames lie -- left (H.264 / HEVC), centre (JPEG) or topleft '
                         '(BT.2020) -- the stand-in decoder sites them so and the GPU interpolates Cb and Cr to every luma pixel; replicate '
                         '(default): every pixel takes the sample of its 2 x 2 block')
    ap.add_argument('--finish-on-gpu', dest='finish_on_gpu', action='store_true',
                    help='finish every frame on the GPU: the timed loop fetches the labels at the SOURCE frame\'s size (padding and '
                         'resize undone there), the confusion matrix of the mIoU accumulates in HBM and --out writes those labels; '
                         'with --raw-frames this evaluates frames of any size against ground truth of their own size')
    ap.add_argument('--confidence', action='store_true',
                    help='with --finish-on-gpu: per frame, the mean confidence (largest softmax probability) and the share of pixels '
                         'below level 128 of 256, from a histogram made on the GPU where the logits are; --out also writes '
                         'conf_<frame>.png in greyscale.  With --interpolate the confidence is that of the interpolated scores, the '
                         'ones the labels are the argmax of, and both come from one pass over the logits inside the timed loop')
    ap.add_argument('--interpolate', action='store_true',
                    help='with --finish-on-gpu: the labels at the source size are the argmax of the bilinearly INTERPOLATED scores '
                         '(made on the GPU where the logits are) instead of the nearest label of the finished map; the mIoU counts them')
    ap.add_argument('--overlay-yuv', dest='overlay_yuv', action='store_true',
                    help='with --finish-on-gpu and --nv12 or --yuv: the labels blended over the frame IN ITS OWN FORMAT on the GPU (what an '
                         'encoder or a compositor takes; honours --interpolate); --out writes overlay_<frame>.png, the GPU\'s BGR '
                         'conversion of those bytes')
    ap.add_argument('--summary', action='store_true',
                    help='with --finish-on-gpu: per frame, the three largest classes with their share of the frame and their box, and from the '
                         'second frame of a clip on the label churn against the previous frame -- counted on the GPU at the source size, a few '
                         'hundred bytes per frame instead of the label map.  With --interpolate the labels are those of the interpolated scores')
    ap.add_argument('--components', type=int, nargs='?', const=64, default=None, metavar='MIN_AREA',
                    help='with --finish-on-gpu: per frame, the number of objects of every class that has any -- the connected components of the '
                         'labels at the source size with at least MIN_AREA pixels (default 64), found on the GPU -- and the class, box and area '
                         'of the largest one; "(truncated)" when there are more objects than records.  With --interpolate the labels are those '
                         'of the interpolated scores')
    ap.add_argument('--trimap', type=_trimap_widths, default=None, metavar='W1,W2,..',
                    help='with --finish-on-gpu: 1 to 4 ascending band widths in pixels (1 .. 16), such as 1,2,4,8: at the end of the run, one line '
                         'per width with the mIoU restricted to the pixels closer than that to a ground-truth boundary -- where feature '
                         'propagation costs accuracy first -- counted on the GPU with the mIoU itself (honours --interpolate)')
    ap.add_argument('--adaptive-key', dest='adaptive_key', type=float, default=None, metavar='SHARE',
                    help='content-adaptive key frames: a frame becomes a key frame when more than SHARE (0 .. 1) of its cells changed against '
                         'the last key frame, measured on the GPU where the frame is; --interval is then the LONGEST distance between key '
                         'frames.  The per-frame line gains " key" / " share 0.xxx"')
    ap.add_argument('--key-level', dest='key_level', type=float, default=16.0,
                    help='with --adaptive-key: the mean absolute change of a cell, in grey levels, above which it counts as changed')
    ap.add_argument('--key-cell', dest='key_cell', type=int, default=32, choices=[8, 16, 32, 64], help='with --adaptive-key: the cell size in pixels')
    ap.add_argument('--scales', default='', help='TARGETxMAX: resize target for the short side and limit for the long side '
                                                 '(overrides SCALES of the configuration, also the one --synthetic sets)')
    args = ap.parse_args(argv)
    if args.trimap and not args.finish_on_gpu:
        ap.error("--trimap needs --finish-on-gpu: the bands are counted on the GPU")
    version, interv, num_ex = str(args.version), args.interval, args.num_ex
    if version not in ['18', '34', '50', '101', 'dff']:
        raise ValueError("Invalid Accel version '%s' - must be one of Accel-{18,34,50,101} (or 'dff')" % version)
    if interv < 1:
        raise ValueError("Invalid interval %d - must be >=1" % interv)
    if num_ex < 1:
        raise ValueError("Invalid num_ex %d - must be >=1" % num_ex)
    if args.confidence and not args.finish_on_gpu:
        raise ValueError("--confidence needs --finish-on-gpu")
    if args.interpolate and not args.finish_on_gpu:
        raise ValueError("--interpolate needs --finish-on-gpu")
    if args.summary and not args.finish_on_gpu:
        raise ValueError("--summary needs --finish-on-gpu")
    if args.components is not None and not args.finish_on_gpu:
        raise ValueError("--components needs --finish-on-gpu")
    if args.nv12 and args.yuv:
        raise ValueError("--nv12 and --yuv are mutually exclusive: the frames are fed in one format")
    if args.overlay_yuv and not (args.finish_on_gpu and (args.nv12 or args.yuv)):
        raise ValueError("--overlay-yuv needs --finish-on-gpu and one of --nv12 / --yuv: the overlay is written in the frame's own format")
    if args.chroma_siting != 'replicate' and not (args.nv12 or args.yuv):
        raise ValueError("--chroma-siting needs --nv12 or --yuv: only subsampled frames have a chroma siting")
    if args.nv12 or args.yuv:
        args.raw_frames = True
    if args.cfg:
        update_config(args.cfg)
    num_classes = config.dataset.NUM_CLASSES

    labels = {}
    if args.data:
        from PIL import Image
        names, label_files = [], []
        for city in ('frankfurt', 'lindau', 'munster'):
            names += sorted(glob.glob(os.path.join(args.data, 'leftImg8bit_sequence/val', city, '*.png')))
            label_files += sorted(glob.glob(os.path.join(args.data, 'gtFine/val', city, '*trainIds.png')))
        names = select_frames(names[:30 * num_ex], num_ex, interv, args.avg_acc)
        frames = [np.asarray(Image.open(n).convert('RGB'))[:, :, ::-1] for n in names]
        for lf in label_files:
            labels[label_key(lf)] = lf
    else:
        from .utils import synth
        H, W = [int(v) for v in args.synthetic.split('x')]
        config.SCALES[0] = (H, W)
        frames, names = [], []
        for i in range(num_ex):
            clip = synth.make_clip(H, W, interv, seed=20260929 + i)
            frames += clip
            names += ['synthetic_%06d_%06d_leftImg8bit.png' % (i, t) for t in range(interv)]

    if args.scales:
        config.SCALES[0] = tuple(int(v) for v in args.scales.split('x'))
    from .utils import load_model, synth
    H, W = frames[0].shape[:2]
    if args.nv12 and (H % 2 or W % 2):
        raise ValueError("--nv12: NV12 frames have an even height and width, these frames are %d x %d (odd-sized)" % (H, W))
    if args.yuv and (H % 2 or W % 2):
        raise ValueError("--yuv: the %s frames made here have an even height and width, these frames are %d x %d (odd-sized)" % (args.yuv, H, W))
    if args.finish_on_gpu:    # how a label map goes back to a frame: the valid region of the bound size and the frame's own size
        from .core import results
        from .utils.image import resize_geometry
        g = resize_geometry(H, W, config.SCALES[0][0], config.SCALES[0][1], config.network.IMAGE_STRIDE)
        source = dict(out_h=g[1], out_w=g[2], h=H, w=W)
        evaluator, hist_before = results.Evaluator(num_classes), np.zeros((num_classes, num_classes), np.int64)
        trimap = results.TrimapEvaluator(num_classes, args.trimap) if args.trimap else None
    if args.raw_frames:       # the size the graphs are bound at: the frame after resize + padding
        from .utils.image import resize_geometry
        H, W = resize_geometry(H, W, config.SCALES[0][0], config.SCALES[0][1], config.network.IMAGE_STRIDE)[3:]
    if args.params:
        arg_params, aux_params = {}, {}
        for prefix in args.params:
            a, x = load_model.load_param_file(prefix, process=True)
            arg_params.update(a)
            aux_params.update(x)
    else:
        print('no --params given: seeded random weights (throughput is valid, mIoU is meaningless)')
        arg_params, aux_params = synth.model_params(version, H, W, config)

    data = build_batches(frames, config, pinned=not args.pageable, raw=args.raw_frames, nv12=args.nv12, yuv=args.yuv,
                         yuv_colour=args.yuv_colour, siting=args.chroma_siting)
    runner = ClipRunner(version, config, arg_params, aux_params, (H, W))
    for j in range(min(2, len(data))):       # warm up (demo.py:207-220)
        runner.step(j, data[j], interv)[1].asnumpy()
    print("warmup done")
    schedule = None
    if args.adaptive_key is not None:
        from .core.schedule import KeySchedule
        schedule = KeySchedule.adaptive(args.adaptive_key, level=args.key_level, cell=args.key_cell, max_interval=interv)
    time_sum, count = 0.0, 0
    hist = np.zeros((num_classes, num_classes))
    for idx, arrays in enumerate(data):
        tic()
        lg, lab = runner.step(idx, arrays, interv, schedule=schedule)
        if idx + 1 < len(data) and not args.pageable:
            runner.prefetch(data[idx + 1])        # next frame starts crossing PCIe while this one computes
        fused = args.finish_on_gpu and args.interpolate and args.confidence       # labels, conf and hist from ONE pass over the logits
        if fused:
            pred, conf, conf_hist = results.confidence(lg, source, interpolate=True, labels=True, hist=True)
            pred = pred[0]
        elif args.finish_on_gpu:
            pred = (results.labels_at_source(lg, source, interpolate=True) if args.interpolate else results.labels_at_source(lab, source))[0]
        else:
            pred = np.uint8(np.squeeze(lab.asnumpy()))
        elapsed = toc()
        time_sum += elapsed
        count += 1
        note = ''
        if schedule is not None:
            note = ' key' if runner.last_key else ''
            if runner.last_change:
                note += ' share {:.3f}'.format(max(c / float(cells) for c, cells, _ in runner.last_change))
        print('testing {} {:.4f}s [{:.4f}s]{}'.format(names[idx], elapsed, time_sum / count, note))
        if args.confidence:       # after the clock: the histogram is 2 KB, the map a byte per source pixel
            if not fused:
                conf, conf_hist = results.confidence(lg, source, hist=True)
            mean, low = results.confidence_summary(conf_hist[0])
            print('confidence mean {:.4f} below-128 {:.4f}'.format(mean, low))
            if args.out:
                from PIL import Image
                os.makedirs(args.out, exist_ok=True)
                Image.fromarray(conf[0]).save(os.path.join(args.out, 'conf_' + os.path.basename(names[idx])))
        if args.summary:          # after the clock: what is in the frame, where, and did it just change -- no label map crosses PCIe for it
            handle = lg if args.interpolate else lab
            if idx % interv == 0:
                results.forget(handle)        # a new clip: its first frame is not compared with the last one of another scene
            s = results.summary(handle, source, ncls=num_classes, track=True, interpolate=args.interpolate)
            area = s.stats[0, :, 0].astype(np.int64)
            top = [k for k in np.argsort(-area, kind='stable')[:3] if area[k] > 0]
            line = ' '.join('{}:{:.3f}[{},{},{},{}]'.format(k, area[k] / float(source['h'] * source['w']), *s.box[0, k]) for k in top)
            if s.trans is not None:
                line += ' churn {:.3f}'.format(float(results.summary_churn(s.trans)[0]))
            print('summary ' + line)
        if args.components is not None:       # after the clock: how many objects of every class, and the largest one -- a few KB per frame
            c = results.components(lg if args.interpolate else lab, source, ncls=num_classes, min_area=args.components,
                                   interpolate=args.interpolate)
            rec, _ = results.components_of(c, 0)
            per_class = np.bincount(rec[:, 0], minlength=num_classes)
            line = ' '.join('{}:{}'.format(k, per_class[k]) for k in range(num_classes) if per_class[k])
            if len(rec):
                big = rec[int(np.argmax(rec[:, 1]))]
                line += ' largest {}[{},{},{},{}]={}'.format(big[0], big[2], big[3], big[4], big[5], big[1])
            if int(c.count[0]) > c.comp.shape[1]:
                line += ' (truncated)'
            print('components ' + line)
        if args.out:
            from PIL import Image
            from .dataset.cityscape import getpallete
            os.makedirs(args.out, exist_ok=True)
            seg = Image.fromarray(pred)
            seg.putpalette(getpallete(256))
            seg.save(os.path.join(args.out, 'seg_' + os.path.basename(names[idx])))
        if args.overlay_yuv:      # after the clock: the frame's own bytes with the labels blended in, shown through the GPU's own conversion
            from .dataset.cityscape import getpallete
            like = arrays[0]
            over = results.overlay(lg if args.interpolate else lab, like, getpallete(256), interpolate=args.interpolate)
            if args.out:
                from PIL import Image
                ctx, lay = lab.device_ref[0].ctx, like.layout
                if args.nv12:
                    bgr = ctx.nv12_to_bgr(over, lay['h'], lay['w'], lay['pitch'], lay['uv_offset'], lay['frame_bytes'], lay['colour'], siting=like.siting)
                else:
                    keys = {k: lay[k] for k in ('pitch', 'pitch_c', 'u_offset', 'v_offset', 'frame_bytes')}
                    bgr = ctx.yuv_to_bgr(over, lay['format'], lay['h'], lay['w'], colour=lay['colour'], siting=like.siting, **keys)
                os.makedirs(args.out, exist_ok=True)
                Image.fromarray(np.ascontiguousarray(bgr[0][:, :, ::-1])).save(os.path.join(args.out, 'overlay_' + os.path.basename(names[idx])))
        lf = labels.get(label_key(names[idx]))
        if lf is not None:
            from PIL import Image
            label = np.asarray(Image.open(lf))
            if args.finish_on_gpu:      # counted on the GPU against `lab` itself; this frame's matrix is the difference of two reads
                if args.interpolate:
                    evaluator.add(lg, label, like=source, interpolate=True)
                else:
                    evaluator.add(lab, label, like=source)
                hist = evaluator.hist()
                curr_hist, hist_before = hist - hist_before, hist
                if trimap is not None:
                    trimap.add(lg if args.interpolate else lab, label, like=source, interpolate=args.interpolate)
            else:
                curr_hist = fast_hist(pred.flatten(), label.flatten(), num_classes)
                hist += curr_hist
            print('mIoU {mIoU:.3f}'.format(mIoU=round(np.nanmean(per_class_iu(curr_hist)) * 100, 2)))
            print('(cum) mIoU {mIoU:.3f}'.format(mIoU=round(np.nanmean(per_class_iu(hist)) * 100, 2)))
    if hist.sum() > 0:
        ious = per_class_iu(hist) * 100
        print(' '.join('{:.03f}'.format(i) for i in ious))
        print('===> final mIoU {mIoU:.3f}'.format(mIoU=round(np.nanmean(ious), 2)))
        if args.trimap:
            for width, miou in zip(trimap.widths, trimap.miou()):
                print('trimap {:2d} px: mIoU {:.2f}'.format(width, miou * 100))
    print('{:.2f} frames/s'.format(count / time_sum))
    print('done')


if __name__ == '__main__':
    main()
