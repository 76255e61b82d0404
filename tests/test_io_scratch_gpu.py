"""The scratch buffers one model shares between its entry-point families (csrc/accel_io.cpp: staged input, staged output, interpolated labels,
the uint8 shadow of a prefetch): frames, finished frames, interpolated labels and confidence are called on ONE model in turn while the source size
goes up and down, so that every buffer is grown by one family and reused by another.  Each result is what the families' own tests demand --
the host specifications of utils/image.py and demo.fast_hist, np.array_equal, no tolerance -- and the inputs come from the builders of those tests
(interp_ref.py, confidence_ref.py), whose guard conditions are asserted here for the cases this walk adds."""
import numpy as np
import pytest

from accel_amd.utils import image

import confidence_ref as cref
import interp_ref as iref
import test_frames_nv12_gpu as nv12
from test_confidence_gpu import _bits
from test_frames_nv12_cpu import _tight
from test_frames_u8_gpu import MEANS, _frames, _geometry, _host, _same
from test_interp_labels_cpu import _smallest_gap
from test_results_gpu import PALETTE, _fast_hist

pytestmark = pytest.mark.gpu

H, W, NCLS = 48, 96, 19
# the sizes of test_model_second_prefetch_of_another_size: the second grows every scratch buffer, the third reuses it
SIZES = ((44, 82), (60, 120), (36, 72))


def _model(ctx, n):
    """a model with the image input `data` of n H x W frames (the plan of test_frames_u8_gpu._input_model, never run here), a `labels` and a
    `logits` buffer of n maps and their meta lines (test_results_gpu._labels_model, test_interp_labels_gpu._logits_model)"""
    from accel_amd import runtime
    m = runtime.Model(ctx)
    ib, h2, w2 = n * 3 * H * W * 4, H // 2, W // 2
    arena = (n * h2 * w2 * 32 + 255) // 256 * 256
    m.add_plan("op", "option graph=0 tune=0\narena bytes=%d\npbuf name=data bytes=%d\npbuf name=data_key bytes=%d\npbuf name=y bytes=%d\n"
                     "pbuf name=labels bytes=%d\npbuf name=logits bytes=%d\n"
                     "meta labels_n=%d labels_h=%d labels_w=%d\nmeta logits_n=%d logits_ncls=%d logits_h=%d logits_w=%d\n"
                     "prep_flow cur=data:0:3:4:%d:%d:%d prev=data_key:0:3:4:%d:%d:%d dst=A:0:6:8:%d:%d:%d H=%d W=%d\n"
                     "export_nchw src=A:0:6:8:%d:%d:%d dst=y:0:6:8:%d:%d:%d\n"
               % (arena, ib, ib, n * 6 * h2 * w2 * 4, (n * H * W + 255) // 256 * 256, n * NCLS * H * W * 4, n, H, W, n, NCLS, H, W,
                  H, W, n, H, W, n, h2, w2, n, H, W, h2, w2, n, h2, w2, n))
    return m


@pytest.mark.parametrize("n", [1, 2])
def test_scratch_is_shared_across_families_growth_and_reuse(ctx, n):
    from accel_amd import runtime
    m = _model(ctx, n)
    pins = []
    total = np.zeros((NCLS, NCLS), np.int64)
    try:
        for rows, cols in SIZES:
            what = "n = %d, %d x %d: " % (n, rows, cols)
            g = _geometry(rows, cols, H, W)
            out_h, out_w = g["out_h"], g["out_w"]
            assert (g["H"], g["W"]) == (H, W)
            rng = np.random.default_rng(rows * 4096 + cols + n)
            # 1. - 3. frames into the image input: host BGR, host NV12, prefetched BGR
            f = _frames(n, rows, cols, 500 + rows + n)
            m.write_u8("data", f, MEANS, **g)
            _same(m.read("data", (n, 3, H, W)), _host(f, H, W), what + "write_u8")
            y = _tight(n, rows, cols, 600 + rows + n)
            m.write_nv12("data", y, rows, cols, MEANS, **g)
            _same(m.read("data", (n, 3, H, W)), nv12._host(y, rows, cols, H, W), what + "write_nv12")
            f2 = _frames(n, rows, cols, 700 + rows + n)
            pins.append(runtime.PinnedBuffer(f2.shape, np.uint8))
            pins[-1].array[...] = f2
            m.prefetch_u8("data", pins[-1])
            m.commit_u8("data", n, rows, cols, 3 * cols, MEANS, **g)
            _same(m.read("data", (n, 3, H, W)), _host(f2, H, W), what + "prefetch_u8 + commit_u8")
            # 4. - 5. finished frames of the `labels` buffer: host ground truth into the accumulator, host frames into a host colour image
            labels = rng.integers(0, NCLS, (n, H, W), dtype=np.uint8)
            gt = rng.integers(0, NCLS, (n, rows, cols), dtype=np.uint8)
            gt[rng.integers(0, 4, gt.shape) == 0] = 255
            src = image.labels_to_source_host(labels, out_h, out_w, rows, cols)
            m.write("labels", labels)
            m.hist_add(gt, out_h, out_w, NCLS)
            total += _fast_hist(src, gt, NCLS)
            assert np.array_equal(m.hist_read(NCLS).astype(np.int64), total), what + "hist_add"
            got = m.labels_colour(n, out_h, out_w, rows, cols, PALETTE, frames=f, alpha=128)
            assert np.array_equal(got, image.colour_host(src, PALETTE, frames=f, alpha=128)), what + "labels_colour"
            # 6. - 8. the same from the interpolated scores of the `logits` buffer
            case = iref.small_case(rows, cols, H, W, ncls=NCLS, n=n, scale=1.0)
            assert (case.H, case.W, case.out_h, case.out_w) == (H, W, out_h, out_w)
            gap, top = _smallest_gap(case)
            assert gap >= iref.GUARD * top, (what, gap, top)              # the condition of test_interp_labels_cpu.py, for this case
            want = iref.reference(case)
            m.write("logits", iref.scores(case))
            m.scores_hist_add(gt, out_h, out_w, NCLS)
            total += _fast_hist(want, gt, NCLS)
            assert np.array_equal(m.hist_read(NCLS).astype(np.int64), total), what + "scores_hist_add"
            got = m.scores_colour(n, out_h, out_w, rows, cols, PALETTE, frames=f2, alpha=128)
            assert np.array_equal(got, image.colour_host(want, PALETTE, frames=f2, alpha=128)), what + "scores_colour"
            got = m.scores_labels(n, out_h, out_w, rows, cols)
            assert got.dtype == np.uint8 and np.array_equal(got, want), what + "scores_labels"
            # 9. confidence of the `logits` buffer
            ccase = cref.small_case(rows, cols, H, W, ncls=NCLS, n=n, scale=1.0)
            v, exact = cref.scaled_float64(ccase)
            assert not ((np.abs(v - np.rint(v)) < cref.GUARD) & ~exact).any(), what       # the condition of test_confidence_cpu.py, for this case
            m.write("logits", cref.scores(ccase))
            conf, margin, second, hist = m.confidence(n, out_h, out_w, rows, cols)
            wc, wm, ws, wh = cref.reference(ccase)
            assert np.array_equal(conf, wc) and np.array_equal(second, ws) and np.array_equal(hist, wh), what + "confidence"
            assert np.array_equal(_bits(margin), _bits(wm)), what + "margin"
        # the accumulator holds the sum of both kinds of additions at all three sizes
        assert total.sum() > 0 and np.array_equal(m.hist_read(NCLS).astype(np.int64), total)
    finally:
        ctx.sync()
        for p in pins:
            p.close()
        m.close()
