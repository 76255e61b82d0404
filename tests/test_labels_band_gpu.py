"""Trimap evaluation on the GPU (csrc/labels_band.hip behind accel_boundary_distance, accel_labels_band_hist and the accel_model_* forms): the distance to
the ground truth's boundaries and the confusion matrix per bucket of it are what utils.image.boundary_distance_host and band_hist_host give -- EXACTLY.
Everything is integer arithmetic, so every comparison is np.array_equal: no tolerance.  (Host side, and the wrong kernels the cases tell apart:
test_labels_band_cpu.py.)"""
import ctypes
import re

import numpy as np
import pytest

from accel_amd.utils import image, synth

import band_ref as ref
import interp_ref
from test_interp_labels_gpu import _logits_model
from test_results_gpu import STRIDE, _check_rows, _labels_model, _pitched

pytestmark = pytest.mark.gpu

MAPS = [(s, v) for s in ref.ALL_SHAPES for v in ref.maps_of(s)]


def _map_id(sv):
    return "%s-%s" % ("x".join(str(v) for v in sv[0][:8]), sv[1])


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(got, want), (what, int(np.count_nonzero(got != want)), np.argwhere(got != want)[:4].tolist())


# ---- operator level ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sv", MAPS, ids=_map_id)
def test_the_distance_equals_the_specification(ctx, sv):
    s, values = sv
    g, want = ref.ground_truth(s, values), ref.distance(s, values)
    cap = s.widths[-1]
    _equal(ctx.boundary_distance(g, cap), want, "tight rows")
    _equal(ctx.boundary_distance(ref.ground_truth_pitched(s, values), cap, width=s.w), want, "a pitched source")
    # a pitched destination keeps the bytes between its rows
    for pitch in (s.w + 3, (s.w + 15) // 16 * 16 + 16):
        out = _pitched(np.zeros((s.n, s.h, s.w), np.uint8), pitch, pitch)
        before = out.copy()
        assert ctx.boundary_distance(g, cap, out=out) is out
        _check_rows(out, before, want, "dst pitch %d" % pitch)
    # the smaller caps are the same map cut lower: one of them per map
    low = max(1, cap // 2)
    _equal(ctx.boundary_distance(g, low), image.boundary_distance_host(g, low), "cap %d" % low)


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_the_buckets_equal_the_specification(ctx, case):
    s = case.shape
    labels, g, want = ref.labels(case), ref.ground_truth(s, case.values), ref.expected(case)
    got = ctx.labels_band_hist(labels, s.out_h, s.out_w, g, s.ncls, s.widths)
    _equal(got, want, "tight rows")
    _equal(ctx.labels_band_hist(labels, s.out_h, s.out_w, ref.ground_truth_pitched(s, case.values), s.ncls, s.widths, width=s.w), want, "pitched rows")
    # adding to a non-zero hist adds
    start = np.arange(want.size, dtype=np.uint64).reshape(want.shape) * np.uint64(1 << 33)
    _equal(ctx.labels_band_hist(labels, s.out_h, s.out_w, g, s.ncls, s.widths, hist=start), want + start, "added to counts")
    # the sum over the buckets is the matrix the whole-frame kernel gives for the same arrays
    whole = ctx.labels_hist(labels, s.out_h, s.out_w, g, s.ncls)
    _equal(got.sum(axis=0, dtype=np.uint64), whole, "the sum of the buckets against accel_labels_hist")


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_model_accumulates_per_widths_and_leaves_the_other_accumulator_alone(ctx):
    import torch
    from accel_amd import runtime
    s = ref.SHAPES[2]                                   # the crop, three frames
    a, b = ref.Case(s, "blocks+ignored", "independent"), ref.Case(s, "blocks", "ignored")
    ga, gb = ref.ground_truth(s, a.values), ref.ground_truth(s, b.values)
    K = len(s.widths)
    m, other = _labels_model(ctx, s.n, s.H, s.W), _labels_model(ctx, s.n, s.H, s.W)
    try:
        assert not m.band_hist_read(s.ncls, K).any() and not m.band_hist_read(7, 2).any()         # nothing added: any shape may be asked for
        m.write("labels", ref.labels(a))
        gen = m.generation("labels")
        m.hist_add(ga, s.out_h, s.out_w, s.ncls)
        whole = m.hist_read(s.ncls)
        m.band_hist_add(ga, s.out_h, s.out_w, s.ncls, s.widths)
        _equal(m.band_hist_read(s.ncls, K), ref.expected(a), "one add")
        m.band_hist_add(ref.ground_truth_pitched(s, a.values), s.out_h, s.out_w, s.ncls, s.widths, width=s.w)
        _equal(m.band_hist_read(s.ncls, K), ref.expected(a) * np.uint64(2), "two adds accumulate; pitched ground truth")
        assert not other.band_hist_read(s.ncls, K).any()                                          # per model
        # ground truth resident in HBM, at a pitch
        m.write("labels", ref.labels(b))
        dev = torch.from_numpy(ref.ground_truth_pitched(s, b.values).copy()).cuda()
        torch.cuda.synchronize()                         # torch's stream and the library's compute stream are not ordered by themselves
        m.band_hist_add_device(dev.data_ptr(), s.n, s.h, s.w, s.w + ref.GAP, s.out_h, s.out_w, s.ncls, s.widths)
        _equal(m.band_hist_read(s.ncls, K), ref.expected(a) * np.uint64(2) + ref.expected(b), "a device ground truth")
        ctx.sync()
        del dev
        # other widths or another ncls are refused until the accumulator has been cleared
        for ncls, widths in ((s.ncls, (1, 2, 4)), (s.ncls, (1, 2, 4, 9)), (21, s.widths)):
            with pytest.raises(runtime.AccelError, match="accumulator"):
                m.band_hist_add(gb, s.out_h, s.out_w, ncls, widths)
        for ncls, k in ((21, K), (s.ncls, K - 1)):
            with pytest.raises(runtime.AccelError, match="accumulator"):
                m.band_hist_read(ncls, k)
        total = ref.expected(a) * np.uint64(2) + ref.expected(b)
        _equal(m.band_hist_read(s.ncls, K, clear=True), total, "the refused calls added nothing")
        assert not m.band_hist_read(s.ncls, K).any()
        m.band_hist_add(gb, s.out_h, s.out_w, 21, (3, 16))
        _equal(m.band_hist_read(21, 2), image.band_hist_host(ref.labels(b), s.out_h, s.out_w, gb, 21, (3, 16)), "other values after a clear")
        # hist_add / hist_read of the same model saw none of it, and nothing was written
        _equal(m.hist_read(s.ncls), whole, "the whole-frame accumulator")
        m.hist_add(gb, s.out_h, s.out_w, s.ncls)
        _equal(m.hist_read(s.ncls, clear=True), whole + ref.expected(b).sum(axis=0, dtype=np.uint64), "and still adds")
        _equal(m.band_hist_read(21, 2), image.band_hist_host(ref.labels(b), s.out_h, s.out_w, gb, 21, (3, 16)), "untouched by hist_read(clear)")
        assert m.generation("labels") == gen + 1
        assert np.array_equal(m.read("labels", (s.n, s.H, s.W), np.uint8), ref.labels(b))
    finally:
        ctx.sync()
        m.close()
        other.close()


@pytest.mark.parametrize("case", interp_ref.pitched_cases()[:2] + [c for c in interp_ref.dyadic_cases() if c.kind == "ints" and c.ncls == 19][:2],
                         ids=interp_ref.ident)
def test_the_scores_form_counts_the_interpolated_labels(ctx, case):
    """the inputs of the interpolated-label tests, whose guard condition (test_interp_labels_cpu.py) makes equality of every label a fair demand"""
    labels = interp_ref.reference(case)                  # utils.image.labels_interpolated_host of the case's scores
    rng = np.random.default_rng(case.seed)
    gt = np.repeat(np.repeat(rng.integers(0, 19, (case.n, (case.h + 6) // 7, (case.w + 8) // 9), dtype=np.uint8), 7, axis=1), 9, axis=2)[:, :case.h, :case.w]
    gt = np.ascontiguousarray(gt)
    gt[:, case.h // 2, :] = 255
    widths = (1, 3, 6)
    want = image.band_hist_host(labels, case.h, case.w, gt, 19, widths)
    m = _logits_model(ctx, case.n, case.ncls, case.H, case.W)
    try:
        m.write("logits", interp_ref.scores(case))
        gen = m.generation("logits")
        m.scores_band_hist_add(gt, case.out_h, case.out_w, 19, widths)
        _equal(m.band_hist_read(19, 3), want, "one add")
        m.scores_band_hist_add(gt, case.out_h, case.out_w, 19, widths)
        _equal(m.band_hist_read(19, 3, clear=True), want * np.uint64(2), "two adds")
        assert m.generation("logits") == gen
    finally:
        ctx.sync()
        m.close()


# ---- argument errors --------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_err_arg(ctx):
    """every call the kernels could not honour is refused on the host, with a message that names the argument; nothing is launched, nothing is written and
    the accumulators are what they were"""
    from accel_amd import runtime
    lib = runtime.lib()
    n, H, W, out_h, out_w, h, w, ncls = 2, 32, 64, 31, 54, 29, 50, 19
    rng = np.random.default_rng(3)
    labels = rng.integers(0, ncls, (n, H, W), dtype=np.uint8)
    gt = np.repeat(rng.integers(0, ncls, (n, h, 5), dtype=np.uint8), 10, axis=2)
    hist = np.zeros((5, ncls, ncls), np.uint64)
    dist = np.zeros((n, h, w), np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    ints = lambda ws: None if ws is None else (ctypes.c_int * len(ws))(*ws)
    good = dict(labels=labels, n=n, H=H, W=W, out_h=out_h, out_w=out_w, gt=gt, h=h, w=w, gt_pitch=w, ncls=ncls, widths=(1, 2, 4, 8), nwidths=4, hist=hist,
                cap=8, dst=dist, dst_pitch=w)
    m, lm = _labels_model(ctx, n, H, W), _logits_model(ctx, n, 19, H, W)
    try:
        m.write("labels", labels)
        lm.write("logits", rng.standard_normal((n, 19, H, W)).astype(np.float32))
        m.band_hist_add(gt, out_h, out_w, ncls, (1, 2, 4, 8))
        lm.scores_band_hist_add(gt, out_h, out_w, ncls, (1, 2, 4, 8))
        m.hist_add(gt, out_h, out_w, ncls)
        state = m.band_hist_read(ncls, 4), lm.band_hist_read(ncls, 4), m.hist_read(ncls), m.generation("labels"), lm.generation("logits")
        calls = {
            "distance": lambda a: lib.accel_boundary_distance(ctx.handle, vp(a["gt"]), a["n"], a["h"], a["w"], a["gt_pitch"], a["cap"], vp(a["dst"]),
                                                              a["dst_pitch"]),
            "op": lambda a: lib.accel_labels_band_hist(ctx.handle, vp(a["labels"]), a["n"], a["H"], a["W"], a["out_h"], a["out_w"], vp(a["gt"]), a["h"], a["w"],
                                                       a["gt_pitch"], a["ncls"], ints(a["widths"]), a["nwidths"], vp(a["hist"])),
            "labels": lambda a: lib.accel_model_band_hist_add(m.handle, vp(a["gt"]), a["n"], a["h"], a["w"], a["gt_pitch"], a["out_h"], a["out_w"], a["ncls"],
                                                              ints(a["widths"]), a["nwidths"], 0),
            "scores": lambda a: lib.accel_model_scores_band_hist_add(lm.handle, vp(a["gt"]), a["n"], a["h"], a["w"], a["gt_pitch"], a["out_h"], a["out_w"],
                                                                     a["ncls"], ints(a["widths"]), a["nwidths"], 0),
        }
        every, hists, models = tuple(calls), ("op", "labels", "scores"), ("labels", "scores")
        cases = [(dict(n=0), "n =", every), (dict(n=-1), "n =", every), (dict(n=32769), "n =", every), (dict(h=0), "h =", every), (dict(w=0), "w =", every),
                 (dict(h=32769), "h =", every), (dict(w=32769), "w =", every), (dict(gt=None), "NULL", every), (dict(gt_pitch=w - 1), "pitch", every),
                 (dict(out_h=H + 1), "out_h", hists), (dict(out_w=W + 1), "out_w", hists), (dict(out_h=0), "out_h", hists), (dict(out_w=0), "out_w", hists),
                 (dict(H=0), "H x W", ("op",)), (dict(W=32769), "H x W", ("op",)), (dict(labels=None), "labels", ("op",)), (dict(hist=None), "hist", ("op",)),
                 (dict(ncls=0), "ncls", hists), (dict(ncls=33), "ncls", hists), (dict(widths=None), "widths", hists),
                 (dict(nwidths=0), "nwidths", hists), (dict(nwidths=5, widths=(1, 2, 3, 4, 5)), "nwidths", hists),
                 (dict(widths=(0, 2, 4, 8)), "widths[0]", hists), (dict(widths=(1, 2, 4, 17)), "widths[3]", hists),
                 (dict(widths=(1, 2, 2, 8)), "ascending", hists), (dict(widths=(1, 4, 2, 8)), "ascending", hists),
                 (dict(cap=0), "cap", ("distance",)), (dict(cap=17), "cap", ("distance",)), (dict(dst=None), "dst", ("distance",)),
                 (dict(dst_pitch=w - 1), "dst_pitch", ("distance",)),
                 (dict(n=n + 1), "n =", models),                                                  # larger than the bound batch
                 (dict(ncls=21), "accumulator", models), (dict(widths=(1, 2, 4), nwidths=3), "accumulator", models),
                 (dict(widths=(1, 2, 4, 9)), "accumulator", models)]
        for change, word, names in cases:
            for name in names:
                rc = calls[name](dict(good, **change))
                msg = lib.accel_last_error().decode()
                assert rc == -1, (name, change, rc, msg)       # ACCEL_ERR_ARG
                assert word in msg, (name, change, msg)
        assert lib.accel_boundary_distance(None, vp(gt), n, h, w, w, 8, vp(dist), w) == -1
        assert lib.accel_labels_band_hist(None, vp(labels), n, H, W, out_h, out_w, vp(gt), h, w, w, ncls, ints((1,)), 1, vp(hist)) == -1
        assert lib.accel_model_band_hist_add(None, vp(gt), n, h, w, w, out_h, out_w, ncls, ints((1,)), 1, 0) == -1
        assert lib.accel_model_band_hist_add(lm.handle, vp(gt), n, h, w, w, out_h, out_w, ncls, ints((1, 2, 4, 8)), 4, 0) == -1
        assert "labels" in lib.accel_last_error().decode()       # a model without label maps
        assert lib.accel_model_scores_band_hist_add(m.handle, vp(gt), n, h, w, w, out_h, out_w, ncls, ints((1, 2, 4, 8)), 4, 0) == -1
        assert "logits" in lib.accel_last_error().decode()       # and one without scores
        out = np.zeros((5, 21, 21), np.uint64)
        for args, word in (((None, vp(out), ncls, 4, 0), "m is"), ((m.handle, None, ncls, 4, 0), "out"), ((m.handle, vp(out), 0, 4, 0), "ncls"),
                           ((m.handle, vp(out), 33, 4, 0), "ncls"), ((m.handle, vp(out), ncls, 0, 0), "nwidths"), ((m.handle, vp(out), ncls, 5, 0), "nwidths"),
                           ((m.handle, vp(out), 21, 4, 0), "accumulator"), ((m.handle, vp(out), ncls, 3, 0), "accumulator")):
            assert lib.accel_model_band_hist_read(*args) == -1 and word in lib.accel_last_error().decode(), (args[2:], lib.accel_last_error().decode())
        # none of the refused calls wrote anything or reached the models
        assert not hist.any() and not dist.any() and not out.any()
        now = m.band_hist_read(ncls, 4), lm.band_hist_read(ncls, 4), m.hist_read(ncls), m.generation("labels"), lm.generation("logits")
        assert all(np.array_equal(a, b) for a, b in zip(state, now))
        # and every call is accepted as it stands
        want = image.band_hist_host(labels, out_h, out_w, gt, ncls, (1, 2, 4, 8))
        for name in every:
            assert calls[name](good) == 0, (name, lib.accel_last_error().decode())
        _equal(dist, image.boundary_distance_host(gt, 8), "the distance call")
        _equal(hist, want, "the operator call")
        _equal(m.band_hist_read(ncls, 4), want * np.uint64(2), "the labels form")
        interpolated = lm.scores_labels(n, out_h, out_w, h, w)
        _equal(lm.band_hist_read(ncls, 4), image.band_hist_host(interpolated, h, w, gt, ncls, (1, 2, 4, 8)) * np.uint64(2), "the scores form")
    finally:
        ctx.sync()
        m.close()
        lm.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def _block_gt(rng, rows, cols, ncls):
    gt = np.repeat(np.repeat(rng.integers(0, ncls, ((rows + 23) // 24, (cols + 30) // 31), dtype=np.uint8), 24, axis=0), 31, axis=1)[:rows, :cols]
    gt = np.ascontiguousarray(gt)
    gt[rows // 3:rows // 3 + 9, cols // 2:cols // 2 + 20] = 255
    return gt


def test_trimap_evaluator_on_accel18(demo_cfg):
    """Accel-18 at 128 x 256 on the synthetic clip, raw frames of 90 x 180: a key frame and a non-key frame are counted in bands on the GPU, next to the
    whole-frame evaluator, on the labels and on the interpolated scores"""
    from accel_amd import demo, runtime
    from accel_amd.core import results, tester
    H, W, rows, cols = 128, 256, 90, 180
    widths = (1, 2, 4, 8)
    demo_cfg.SCALES[0] = (H, W)
    demo_cfg.network.IMAGE_STRIDE = STRIDE
    arg, aux = synth.model_params("18", H, W, demo_cfg)
    frames = synth.make_clip(rows, cols, 3)
    rng = np.random.default_rng(rows)
    try:
        r = demo.ClipRunner("18", demo_cfg, arg, aux, (H, W))
        raw = demo.build_batches(frames, demo_cfg, raw=True)
        tri, ev, tri_i = results.TrimapEvaluator(19, widths), results.Evaluator(19), None
        total = np.zeros((5, 19, 19), np.int64)
        total_i = np.zeros((5, 19, 19), np.int64)
        kept = None
        for i in (0, 1):
            lg, lab = r.step(i, raw[i], 3)
            m = lab.device_ref[0]
            gen = m.generation("labels"), m.generation("logits")
            gt = _block_gt(rng, rows, cols, 19)
            tri.add(lab, gt, like=raw[i][0])
            ev.add(lab, gt, like=raw[i][0])
            src = results.labels_at_source(lab, raw[i][0])
            total += image.band_hist_host(src, rows, cols, gt, 19, widths).astype(np.int64)
            hist = tri.hist()
            assert hist.dtype == np.int64 and hist.shape == (5, 19, 19)
            assert np.array_equal(hist[4], ev.hist()), "the last entry is the whole frame"
            assert np.array_equal(hist[:4], np.cumsum(total, axis=0)[:4]), "the bands against the specification on the fetched labels"
            assert np.array_equal(tri.buckets(), total)
            # the distance of the fetched prediction, through the same context
            d = results.boundary_distance(src, 8, ctx=m.ctx)
            assert np.array_equal(d, image.boundary_distance_host(src, 8))
            assert (m.generation("labels"), m.generation("logits")) == gen
            kept = lab
        miou = tri.miou()
        assert miou.shape == (5,) and np.allclose(miou, results.TrimapEvaluator.miou_of(np.cumsum(total, axis=0)), equal_nan=True)
        assert tri.per_class_iu().shape == (5, 19)
        assert miou[4] == pytest.approx(float(np.nanmean(results.per_class_iu(ev.hist()))))
        # the interpolated scores go into the same accumulator: a second evaluator reports what was added since it adopted the model
        tri_i = results.TrimapEvaluator(19, widths)
        gt = _block_gt(rng, rows, cols, 19)
        tri_i.add(lg, gt, like=raw[1][0], interpolate=True)
        total_i += image.band_hist_host(results.labels_at_source(lg, raw[1][0], interpolate=True), rows, cols, gt, 19, widths).astype(np.int64)
        assert np.array_equal(tri_i.buckets(), total_i) and np.array_equal(tri.buckets(), total + total_i)
        with pytest.raises(runtime.AccelError, match="accumulator"):
            results.TrimapEvaluator(19, (2, 4)).add(lab, gt, like=raw[1][0])
        # a label handle kept across the next step names a buffer that has been rewritten: never read
        r.step(2, raw[2], 3)
        with pytest.raises(runtime.AccelError, match="stale"):
            tri.add(kept, gt, like=raw[1][0])
        assert np.array_equal(tri.buckets(clear=True), total + total_i) and not tri.hist().any()
    finally:
        tester.release_models()


TIMES = re.compile(r"\d+\.\d+s|\d+\.\d+ frames/s")


def test_demo_prints_the_trimap(demo_cfg, capsys, tmp_path):
    """--trimap 1,2,4 adds one line per width after the mIoU lines -- the numbers the host specification gives for the labels the run wrote -- and changes
    no other line: without the flag the output is what it is without this feature"""
    from PIL import Image
    from accel_amd import demo
    from accel_amd.core import results, tester
    rows, cols, interval, num_ex = 90, 180, 3, 2
    rng = np.random.default_rng(11)
    gts = {}
    for ci, city in enumerate(["frankfurt", "lindau"]):
        seq = tmp_path / "data" / "leftImg8bit_sequence" / "val" / city
        gt_dir = tmp_path / "data" / "gtFine" / "val" / city
        seq.mkdir(parents=True)
        gt_dir.mkdir(parents=True)
        for t, f in enumerate(synth.make_clip(rows, cols, 30, seed=700 + ci)):
            Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(str(seq / ("%s_000000_%06d_leftImg8bit.png" % (city, t))))
        gts[city] = _block_gt(rng, rows, cols, 19)
        Image.fromarray(gts[city]).save(str(gt_dir / ("%s_000000_000019_gtFine_trainIds.png" % city)))
    argv = ["--version", "18", "--interval", str(interval), "--num_ex", str(num_ex), "--data", str(tmp_path / "data"), "--scales", "128x256", "--raw-frames",
            "--finish-on-gpu"]
    outs = []
    for extra in (["--out", str(tmp_path / "seg")], ["--trimap", "1,2,4"]):
        try:
            demo.main(argv + extra)
        finally:
            tester.release_models()
        outs.append(capsys.readouterr().out)
    plain, with_trimap = (TIMES.sub("T", o).splitlines() for o in outs)
    assert not any(line.startswith("trimap") for line in plain)
    lines = [line for line in with_trimap if line.startswith("trimap")]
    assert [line for line in with_trimap if not line.startswith("trimap")] == plain
    assert len(lines) == 3 and with_trimap[-5:-2] == lines and with_trimap[-6].startswith("===> final mIoU") and plain[-1] == "done"
    # the labels the first run wrote are the fetched source-size labels of the labelled frames
    buckets = np.zeros((4, 19, 19), np.int64)
    for city, gt in gts.items():
        seg = np.asarray(Image.open(str(tmp_path / "seg" / ("seg_%s_000000_000019_leftImg8bit.png" % city))))
        assert seg.shape == (rows, cols)
        buckets += image.band_hist_host(seg, rows, cols, gt, 19, (1, 2, 4)).astype(np.int64)
    want = results.TrimapEvaluator.miou_of(np.cumsum(buckets, axis=0))
    assert lines == ["trimap %2d px: mIoU %.2f" % (width, v * 100) for width, v in zip((1, 2, 4), want)]
    with pytest.raises(SystemExit):
        demo.main(["--trimap", "1,2,4"])
    assert "finish-on-gpu" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        demo.main(["--finish-on-gpu", "--trimap", "4,2"])
    assert "ascending" in capsys.readouterr().err
