"""Audit of the range-slot ids the lowering emits (lower.Lowering.text; csrc/range.h; accel_hip.cpp resolve_range_flags).

The library learns that an op wrote a buffer only from that op's `yr=` / `y2r=`.  A writer without the id is invisible to it: the
fp16x2-form convolution that reads the buffer (`xr=`) neither measures the buffer nor counts that writer, and its pixel scale can
then come from the other writers alone.  So, for every lowered plan of the headline models: every View argument of every op is
classified as a read or a write by the explicit table below (an argument the table does not know fails the audit, so a new op
kind cannot slip past it), and every op that writes a buffer some convolution reads through `xr=` carries that buffer's id in
the emitted text, under `yr=` for its first output and `y2r=` for its second."""
import pytest

from accel_amd.lower import View

# (op kind, argument) -> "r" (read) / "w" (write, with the key of the range id the text must carry for it)
ACCESS = {
    ("conv", "in"): "r", ("conv", "res"): "r", ("conv", "out"): "yr", ("conv", "out2"): "y2r",
    ("pool", "in"): "r", ("pool", "out"): "yr",
    ("dcn_cols", "in"): "r", ("dcn_cols", "off"): "r", ("dcn_cols", "out"): "yr",
    ("warp", "feat"): "r", ("warp", "flow"): "r", ("warp", "out"): "yr", ("warp", "out2"): "y2r",
    ("copy", "src"): "r", ("copy", "dst"): "yr",
    ("prep_rgb", "src"): "r", ("prep_rgb", "dst"): "yr",
    ("prep_flow", "cur"): "r", ("prep_flow", "prev"): "r", ("prep_flow", "dst"): "yr",
    ("score_tail", "left"): "r", ("score_tail", "right"): "r",
    ("import_nchw", "src"): "r", ("import_nchw", "dst"): "yr",
    ("export_nchw", "src"): "r",
}


def _sym(version, key):
    from accel_amd import symbols
    from accel_amd.config.config import config
    inst = getattr(getattr(symbols, "accel_" + version), "accel_" + version)()
    return inst.get_key_test_symbol(config) if key else inst.get_cur_test_symbol(config)


def _op_lines(text):
    """the op lines of a plan text as (kind, {key: value}) in list order"""
    out = []
    for line in text.splitlines():
        toks = line.split()
        if not toks or toks[0].startswith("#") or toks[0] in ("option", "meta", "arena", "pbuf"):
            continue
        out.append((toks[0], dict(t.split("=", 1) for t in toks[1:])))
    return out


def _bkey(v):
    return ("A", v.buf.id) if v.buf.space == "A" else ("P", v.buf.space)


def audit(text, lw):
    """the checks of the module docstring on one lowered plan; returns the number of (writer, read buffer) pairs checked"""
    lines = _op_lines(text)
    assert [k for k, _ in lines] == [k for k, _ in lw.ops]
    xr_of = {}      # buffer -> the id its convolution readers name
    for (kind, args), (_, toks) in zip(lw.ops, lines):
        for key, v in args.items():
            if isinstance(v, View):
                assert (kind, key) in ACCESS, "op %s %s: View argument %r is in no read/write table" % (kind, args.get("name"), key)
        if kind == "conv":
            assert "xr" in toks, "conv %s names no input range id" % args.get("name")
            b = _bkey(args["in"])
            assert xr_of.setdefault(b, toks["xr"]) == toks["xr"], "conv %s: one buffer, two range ids" % args.get("name")
    assert len(set(xr_of.values())) == len(xr_of), "two buffers share a range id"
    checked = 0
    for (kind, args), (_, toks) in zip(lw.ops, lines):
        for key, v in args.items():
            acc = ACCESS.get((kind, key)) if isinstance(v, View) else None
            if acc in (None, "r") or _bkey(v) not in xr_of:
                continue
            assert toks.get(acc) == xr_of[_bkey(v)], "%s %s writes %s (read by a convolution as range id %s) with %s=%s" % (
                kind, args.get("name"), key, xr_of[_bkey(v)], acc, toks.get(acc))
            checked += 1
    return checked


def _lower(version, key, N, fold_linear, feat_slot, dtype):
    from accel_amd import lower
    sym = _sym(version, key)
    H, W = 128, 256
    shapes = {"data": (N, 3, H, W), "data_key": (N, 3, H, W), "feat_key": (N, 2048, 1, 1) if key else (N, 2048, H // 16, W // 16)}
    shapes = {k: v for k, v in shapes.items() if k in sym.list_arguments()}
    return lower.lower(sym, shapes, conv_dtype=dtype, fold_linear=fold_linear, feat_slot=feat_slot)


@pytest.mark.parametrize("version", ["18", "34", "50", "101"])
def test_every_writer_of_a_range_read_buffer_names_its_id(demo_cfg, version):
    """key and cur plans (the cur pair: feat_slot 0 / 1, and the copy-back form), fold_linear on and off, N = 1 and 3, fp32 and
    bf16x3 convolutions, 128x256"""
    kinds = set()
    for key in (True, False):
        for N in (1, 3):
            for fold in (True, False):
                for slot in ((None,) if key else (None, 0, 1)):
                    for dtype in ("f32", "bf16x3"):
                        text, lw = _lower(version, key, N, fold, slot, dtype)
                        assert audit(text, lw) > 0
                        kinds.update(k for k, _ in lw.ops)
    assert {"conv", "pool", "warp", "prep_rgb"} <= kinds


def test_the_audit_sees_a_writer_without_its_id(demo_cfg):
    """the audit itself: the same plan with one writer's `yr=` / `y2r=` dropped from the text (the first such writer of every kind),
    and with a View argument no table knows"""
    mutated = set()
    for version in ("18", "101"):
        text, lw = _lower(version, False, 1, True, 0, "f32")
        assert audit(text, lw) > 0
        lines = text.splitlines()
        xr = set(t for l in lines for t in l.split() if t.startswith("xr="))
        for j, l in enumerate(lines):
            kind = l.split()[0]
            hit = [t for t in l.split() if t.split("=")[0] in ("yr", "y2r") and "xr=" + t.split("=")[1] in xr]
            if not hit or (kind, hit[-1].split("=")[0]) in mutated:
                continue
            mutated.add((kind, hit[-1].split("=")[0]))
            bad = list(lines)
            bad[j] = " ".join(t for t in l.split() if t != hit[-1])
            with pytest.raises(AssertionError, match="writes"):
                audit("\n".join(bad) + "\n", lw)
    assert {"conv", "warp", "pool", "dcn_cols", "prep_rgb", "prep_flow"} <= set(k for k, _ in mutated), mutated
    kind, args = lw.ops[0]
    args["new_input"] = args[[k for k, v in args.items() if isinstance(v, View)][0]]
    try:
        with pytest.raises(AssertionError, match="no read/write table"):
            audit(text, lw)
    finally:
        del args["new_input"]
