"""The float64 references of the byte movers (movers_ref.py) against the oracle, on the exact inputs test_movers_gpu.py uses, and the
oracle alone against every bound and condition that suite sets for the device: a bound the fp32 oracle cannot meet is a wrong
derivation, a case without its edge taps tests nothing."""
import numpy as np
import pytest

import movers_ref as R
from movers_ref import U
from oracle import ops as O
from plan_helpers import pair

nchw = lambda a: np.ascontiguousarray(np.asarray(a).transpose(0, 3, 1, 2))
nhwc = lambda a: np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))


def oracle_warp(feat, flow):
    return nhwc(O.flow_warp(nchw(feat), nchw(flow)))


def oracle_cols(x, off, k, s, p, d, dg):
    """O.deform_im2col image by image, as (N, Ho, Wo, taps, C)"""
    N, H, W, C = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    Ho, Wo = R.conv_out(H, kh, sh, ph, dh), R.conv_out(W, kw, sw, pw, dw)
    xs, offs = nchw(x), nchw(off)
    out = [O.deform_im2col(xs[n], offs[n], k, s, p, d, dg).reshape(C, kh * kw, Ho, Wo).transpose(2, 3, 1, 0) for n in range(N)]
    return np.stack(out)


# ---- warp -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.WARP_EXACT_C)
@pytest.mark.parametrize("H,W", R.WARP_EXACT_SIZES)
def test_warp_dyadic_inputs_are_exact_and_reach_every_edge(H, W, C):
    feat, flow, bias = R.warp_exact_inputs(H, W, C)
    ref = R.warp64(feat, flow)
    assert np.array_equal(ref.astype(np.float32), ref)                      # representable: nothing is rounded
    np.testing.assert_array_equal(oracle_warp(feat, flow), ref)
    out2 = np.maximum(ref + bias, 0.0)
    assert np.array_equal(out2.astype(np.float32), out2)
    assert not np.array_equal(flow[0], flow[1]) and not np.array_equal(feat[1], feat[2])
    for what, n in R.warp_landings(flow).items():
        assert n >= 1, (what, n)


@pytest.mark.parametrize("H,W,mag", R.WARP_BOUNDED)
def test_warp_bound_holds_for_the_oracle_with_room(H, W, mag):
    feat, flow, bias = R.warp_bounded_inputs(H, W, mag)
    ref, bound = R.warp64(feat, flow), R.warp_bound(feat, flow)
    ratio = float((np.abs(oracle_warp(feat, flow) - ref) / bound).max())
    print("warp %dx%d flow scale %g: oracle at %.2f of the bound" % (H, W, mag, ratio))
    assert ratio < 0.5
    o2 = np.maximum(oracle_warp(feat, flow) + bias, np.float32(0))
    assert (np.abs(o2 - np.maximum(ref + bias, 0)) <= bound + U * np.abs(ref + bias)).all()


def test_warp64_is_the_identity_at_zero_flow_and_a_shift_at_whole_flows():
    feat = R.gauss(1, 2, 6, 7, 4)
    np.testing.assert_array_equal(R.warp64(feat, np.zeros((2, 6, 7, 2))), feat)
    flow = np.zeros((2, 6, 7, 2))
    flow[..., 0] = 1.0
    want = np.zeros_like(feat)
    want[:, :, :-1] = feat[:, :, 1:]
    np.testing.assert_array_equal(R.warp64(feat, flow), want)


# ---- dcn_cols ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DCN_CASES, ids=lambda c: "k%ds%dp%dd%ddg%d_c%d_%dx%d" % c[:8])
def test_dcn_cols_dyadic_inputs_are_exact_and_take_every_branch(case):
    k, s, p, d, dg = case[:5]
    x, off = R.dcn_inputs(case)
    ref, _, rec = R.dcn_cols64(x, off, k, s, p, d, dg)
    assert np.array_equal(ref.astype(np.float32), ref)
    np.testing.assert_array_equal(oracle_cols(x, off, k, s, p, d, dg), ref)
    for what, n in R.branch_counts(rec).items():
        assert n >= R.DCN_MIN_TAPS, (what, n)
    assert np.abs(off).max() <= 2 and np.array_equal(off * 8, np.round(off * 8))
    i = R.DCN_CASES.index(case)
    if k == 3:
        assert R.dcn_blocks(case) == R.DCN_BLOCKS[i]


PAIR_IDS = lambda c: "k%dx%ds%dx%dp%dx%dd%dx%ddg%d_c%d_%dx%d" % (pair(c[0]) + pair(c[1]) + pair(c[2]) + pair(c[3]) + tuple(c[4:8]))


@pytest.mark.parametrize("case", R.DCN_PAIR_CASES, ids=PAIR_IDS)
def test_dcn_cols_with_unequal_pairs_is_exact_takes_every_branch_and_is_grid_sample_inside(case):
    """the reference with (h, w) pairs: bit for bit the oracle on the dyadic inputs of the GPU test, every branch of the rule taken
    where the geometry has it (no padding above: no tap starts outside above without an offset, the offsets alone send them there),
    and -- with every sample pulled inside the map, where DCN v1 and zero-padded bilinear interpolation are the same function --
    torch.nn.functional.grid_sample in double"""
    import torch
    k, s, p, d, dg, C, H, W, _ = case
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    assert kh != kw and ph != pw and dh != dw and (kh, kw) != (3, 3)
    x, off = R.dcn_inputs(case)
    ref, _, rec = R.dcn_cols64(x, off, k, s, p, d, dg)
    assert np.array_equal(ref.astype(np.float32), ref)
    np.testing.assert_array_equal(oracle_cols(x, off, k, s, p, d, dg), ref)
    for what, n in R.branch_counts(rec).items():
        assert n >= R.DCN_MIN_TAPS, (what, n)
    N, Ho, Wo, taps = ref.shape[:4]
    assert (Ho, Wo) == (R.conv_out(H, kh, sh, ph, dh), R.conv_out(W, kw, sw, pw, dw)) and taps == kh * kw
    # interior: move every sample into [0, H - 1] x [0, W - 1]
    o = off.astype(np.float64).reshape(N, Ho, Wo, dg, taps, 2)
    i, j = np.arange(taps) // kw, np.arange(taps) % kw
    py = (np.arange(Ho) * sh - ph).reshape(1, Ho, 1, 1, 1) + i * dh + o[..., 0]
    px = (np.arange(Wo) * sw - pw).reshape(1, 1, Wo, 1, 1) + j * dw + o[..., 1]
    o[..., 0] += np.clip(py, 0.0, H - 1.0) - py
    o[..., 1] += np.clip(px, 0.0, W - 1.0) - px
    py, px = np.clip(py, 0.0, H - 1.0), np.clip(px, 0.0, W - 1.0)
    xg = R.gauss(77, N, H, W, C).astype(np.float64)
    got = R.dcn_cols64(xg, o.reshape(off.shape), k, s, p, d, dg)[0]
    xt, cpg = torch.from_numpy(nchw(xg)), C // dg
    for g in range(dg):
        for t in range(taps):
            grid = torch.from_numpy(np.stack([px[:, :, :, g, t] / ((W - 1) / 2.0) - 1.0, py[:, :, :, g, t] / ((H - 1) / 2.0) - 1.0], axis=-1))
            want = torch.nn.functional.grid_sample(xt[:, g * cpg:(g + 1) * cpg], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            assert np.abs(got[:, :, :, t, g * cpg:(g + 1) * cpg] - nhwc(want.numpy())).max() <= 1e-12 * np.abs(xg).max(), (g, t)


def test_dcn_cases_cover_the_block_counts_and_both_kernels():
    assert sorted(R.DCN_BLOCKS.values()) == [1, 2, 7, 8, 9, 13]
    assert {c[:5] for c in R.DCN_CASES} == {(3, 1, 1, 1, 1), (3, 1, 2, 2, 4), (3, 2, 1, 1, 1), (1, 1, 0, 1, 2), (5, 1, 2, 1, 1)}
    assert {c[5] for c in R.DCN_CASES} == {16, 32}


def test_dcn_cols_bound_holds_for_the_oracle():
    case = R.DCN_CASES[3]
    k, s, p, d, dg = case[:5]
    x, off = R.dcn_inputs(case, gaussian=True)
    ref, S, _ = R.dcn_cols64(x, off, k, s, p, d, dg)
    assert (np.abs(oracle_cols(x, off, k, s, p, d, dg) - ref) <= 4 * U * S).all()      # 4 exact weights: 4 products, 3 sums, one on another


def test_big_dcn_case_is_beyond_the_infinity_cache_and_its_channel_subset_is_one_oracle_problem():
    c = R.BIG_DCN
    assert c["H"] * c["W"] * 9 * c["C"] * 4 > 256 << 20
    ch = R.BIG_DCN_CHANNELS
    assert len(ch) == 32 and np.array_equal(ch // 16, np.arange(32))
    x, off = R.big_dcn_inputs()
    grp = ch // (c["C"] // c["dg"])
    ref, _, rec = R.dcn_cols64(x[..., ch], off, 3, 1, 1, 1, c["dg"], grp=grp)
    assert np.array_equal(grp, np.arange(32) // 2)          # two consecutive channels per group: the oracle's own grouping
    np.testing.assert_array_equal(oracle_cols(x[..., ch], off, 3, 1, 1, 1, c["dg"]), ref)
    assert all(n >= R.DCN_MIN_TAPS for n in R.branch_counts(rec).values())


# ---- pools, BatchNorm, image inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.POOL_C)
@pytest.mark.parametrize("kind,k,s,p,full", R.POOL_MAX_CASES + [("avg", 2, 2, 0, True)])
def test_pool64_matches_the_oracle(kind, k, s, p, full, C):
    x = R.pool_inputs(C)
    ref, S = R.pool64(x, kind, k, s, p, full)
    got = nhwc(O.pool2d(nchw(x), kind, k, s, p, "full" if full else "valid"))
    if kind == "max":
        np.testing.assert_array_equal(got, ref)
    else:
        assert (np.abs(got - ref) <= 5 * U * S).all()          # three sums and the division


@pytest.mark.parametrize("C", R.POOL_C)
@pytest.mark.parametrize("kind,k,s,p,full", R.POOL_PAIR_CASES)
def test_pool64_with_unequal_pairs_matches_torch_and_the_oracle(kind, k, s, p, full, C):
    """torch.nn.functional.max_pool2d / avg_pool2d (count_include_pad, as mx.symbol.Pooling counts) in double with the same pairs:
    `valid` is ceil_mode=False; `full` is ceil_mode=True where that keeps the same number of windows.  The fp32 oracle: a maximum is
    exact, a dyadic average is one correctly rounded division away."""
    import torch
    assert k[0] != k[1] and s[0] != s[1] and p[0] != p[1]
    x = R.pool_dyadic_inputs(C)
    ref, S = R.pool64(x, kind, k, s, p, full)
    f = torch.nn.functional.max_pool2d if kind == "max" else torch.nn.functional.avg_pool2d
    want = f(torch.from_numpy(nchw(x).astype(np.float64)), k, s, p, ceil_mode=full).numpy()
    assert want.shape == nchw(ref).shape, "the case is one where both conventions keep the same windows"
    assert np.abs(nchw(ref) - want).max() <= 1e-13 * np.abs(want).max()
    got = nhwc(O.pool2d(nchw(x), kind, k, s, p, "full" if full else "valid"))
    if kind == "max":
        np.testing.assert_array_equal(got, ref)
    else:
        assert (np.abs(got - ref) <= U * np.abs(ref)).all()
    assert R.pool64(x, kind, k, s, p, not full)[0].shape == ref.shape


@pytest.mark.parametrize("C", R.POOL_C)
@pytest.mark.parametrize("fixg", [0, 1])
def test_bn_bound_holds_for_the_oracle(C, fixg):
    x, bn = R.pool_inputs(C), R.bn_inputs(C)
    v, _ = R.pool64(x, "max", 3, 2, 1, False)
    ref, S = R.bn_apply64(v, bn["gamma"], bn["beta"], bn["mean"], bn["var"], 2e-5, fixg, True)
    pooled = O.pool2d(nchw(x), "max", 3, 2, 1, "valid")
    got = nhwc(O.relu(O.batchnorm(pooled, bn["gamma"], bn["beta"], bn["mean"], bn["var"], 2e-5, bool(fixg))))
    # scale: var + eps, sqrt, division; shift: g * mean, its division by the rounded sd, the subtraction; then v * scale + shift
    assert (np.abs(got - ref) <= 8 * U * S).all()


def test_prep_references_match_the_oracle():
    H, W = R.PREP_RGB_HW
    img, _ = R.image_inputs(H, W)
    ref, _ = R.prep_rgb64(img)
    np.testing.assert_array_equal(ref[..., :3], nhwc(img))
    assert not ref[..., 3].any() and (H * W) % 256
    bn = R.bn_inputs(3)
    for fixg in (0, 1):
        ref, S = R.prep_rgb64(img, (bn["gamma"], bn["beta"], bn["mean"], bn["var"], 2e-5, fixg))
        got = nhwc(O.batchnorm(img, bn["gamma"], bn["beta"], bn["mean"], bn["var"], 2e-5, bool(fixg)))
        assert (np.abs(got - ref[..., :3]) <= 8 * U * S[..., :3]).all()
    H, W = R.PREP_FLOW_HW
    cur, prev = R.image_inputs(H, W, seed=7)
    ref, S = R.prep_flow64(cur, prev)
    data = np.concatenate([cur / np.float32(255.0), prev / np.float32(255.0)], axis=1)
    got = nhwc(O.pool2d(data, "avg", 2, 2, 0, "full"))
    assert (np.abs(got - ref[..., :6]) <= 8 * U * S[..., :6]).all()        # four divisions by 255, three sums, the division by 4
    assert not ref[..., 6:].any()


# ---- score tail -------------------------------------------------------------------------------------------------------------------
def oracle_tail(d, ncls):
    left = nchw(d["left"])
    H, W = 16 * left.shape[2], 16 * left.shape[3]
    a = O.crop_like(O.deconv2d(left, d["wl"], None, 16, 0, groups=ncls), (H, W), (8, 8))
    if "right" not in d:
        return a
    b = O.crop_like(O.deconv2d(nchw(d["right"]), d["wr"], None, 16, 0, groups=ncls), (H, W), (8, 8))
    return O.conv2d(np.concatenate([a, b], axis=1), d["cw"], d["cb"])


def softmax32(x):
    e = np.exp(x - x.max(axis=1, keepdims=True), dtype=np.float32)
    return e / e.sum(axis=1, keepdims=True, dtype=np.float32)


@pytest.mark.parametrize("name", sorted(R.TAIL_CASES))
def test_tail_bounds_hold_for_the_oracle(name):
    ncls, N, (Hs, Ws), right, uniform, opts = R.TAIL_CASES[name]
    d = R.tail_inputs(name)
    ref, S = R.tail64(**d)
    bound = R.tail_bound(ncls, S)
    got = oracle_tail(d, ncls)
    assert got.shape == ref.shape == (N, ncls, 16 * Hs, 16 * Ws)
    assert (np.abs(got - ref) <= bound).all()
    if uniform:
        assert all(np.array_equal(d["wl"][0], d["wl"][c]) for c in range(ncls))
    labels = R.argmax_first(ref)
    for n in range(N):
        assert len(np.unique(labels[n])) >= 2, (name, n)
    assert not np.array_equal(d["left"][0], d["left"][1])
    srt = np.sort(ref, axis=1)
    sure = (srt[:, -1] - srt[:, -2]) > 2 * bound.max(axis=1)
    assert sure.mean() >= 0.9, sure.mean()
    np.testing.assert_array_equal(O.argmax_c(got)[sure], labels[sure])
    if "softmax" in opts:
        assert ref.max() > 89           # expf overflows there: the subtraction of the maximum is exercised
        p_ref, p = R.softmax64(ref), softmax32(got)
        B = bound.max(axis=1, keepdims=True)
        assert (np.abs(p - p_ref) <= p_ref * (2 * B + (ncls + 8) * U) + 2.0 ** -126).all()
        assert (np.abs(p.astype(np.float64).sum(axis=1) - 1) <= (ncls + 2) * U).all()


def test_tail_cases_cover_the_modes():
    c = R.TAIL_CASES
    assert {v[0] for v in c.values()} == {2, 19, 21}
    assert {v[3] for v in c.values()} >= {None, (3, 5), (4, 6), (4, 5), (3, 6)}
    assert all(v[1] == 3 and v[2] == (3, 5) for v in c.values())


@pytest.mark.parametrize("name", sorted(R.TIE_CASES))
def test_tie_cases_tie_at_the_maximum(name):
    d = R.tail_inputs(name)
    ncls = R.TIE_CASES[name][0]
    ref, S = R.tail64(**d)
    got = oracle_tail(d, ncls)
    a, c = R.TIE_CLASSES
    assert np.array_equal(got[:, a], got[:, c]) and np.array_equal(ref[:, a], ref[:, c])
    assert (np.abs(got - ref) <= R.tail_bound(ncls, S)).all()
    assert ((got.max(axis=1) == got[:, a]).sum(axis=(1, 2)) >= 100).all()
    lab = O.argmax_c(got)
    assert (lab == a).sum() >= 300 and not (lab == c).any()
    if "softmax" in R.TIE_CASES[name][5]:
        assert ref.max() > 89
