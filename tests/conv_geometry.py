"""The launch-geometry grid of tests/golden/conv_geometry.json: what finalize answers for every (layer, plan mode, launch geometry id,
split setting) -- the (tile, ksplit, narrow) that Plan.ops() reports, or the error it refuses the plan with.  One-conv plans with
tune=0 graph=0 under ACCEL_AUTOTUNE=0: the plans are finalized and never run, so no convolution is launched.
scripts/record_conv_geometry.py writes the file, test_conv_geometry_gpu.py replays the grid against it.  No tests in here."""
import collections
import os

import numpy as np

from plan_helpers import Builder, pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_geometry.json")

IDS = [None] + list(range(100))      # None: no tile= at all (conv_pick_tile chooses; Cout <= 4 layers go to the narrow kernel)
SPLITS = collections.OrderedDict([("default", ""), ("target1024", "split_target=1024"), ("nosplit", "nosplit=1")])
# plan modes: fp32 layers with the bf16x3 forms, with the fp16x2 forms, f16-mode layers, f16-mode layers between half buffers
MODES = collections.OrderedDict([("b3", "split=b3"), ("h2", "split=h2"), ("f16", "dtype=f16"), ("f16-half", "dtype=f16")])

# Layers: the shapes of tests/conv_ref.py (Case defaults, WINO_GEOMETRY, stem, deconv2x, weight-stationary 1x1, halo) and layers whose
# K is deep and whose grid is small, so every split-K rule of conv_plan_split engages.  K steps are of 32 (16 / 64 for ids 15 / 13),
# Winograd steps of 8 (id 40) or 16 channels (41-43).
#   name            Cin  Cout  H    W   N  k  s  p  d  mode         what it is for
_L = [
    ("default",      32,  136, 13,  19, 3, 3, 1, 1, 1, "conv"),     # Case defaults: 9 K steps in 12 blocks -- an ODD step count, split in two
    ("narrow",       32,    2, 13,  19, 3, 3, 1, 1, 1, "conv"),     # Cout_store 4: the narrow kernel without tile=
    ("cin12",        12,    5,  9,  11, 2, (1, 3), 1, 1, 1, "conv"),   # GEOMETRY k1x3: Cin % 8 == 4 (f16 mode leaves it in fp32), K 36 in 64
    ("halo",         64,   18, 12,  18, 3, 3, 1, 2, 2, "conv"),     # the halo shapes: Cout 18, dilation 2
    ("igemm-split",  512,  64,  4,   6, 1, 3, 1, 1, 1, "conv"),     # 144 K steps, one or two blocks: the igemm rule at its cap (KT / 4)
    ("deep-odd",     288,  40,  6,   7, 1, 3, 1, 1, 1, "conv"),     # 81 K steps (odd) in one block; Winograd refuses the odd width
    ("wino-128",     128,  72,  8,   8, 1, 3, 1, 1, 1, "conv"),     # Cin 128 on an 8x8 map: 16 / 8 Winograd steps, both rules split
    ("wino-split54", 144,  72,  8,   8, 1, 3, 1, 1, 1, "conv"),     # WINO_GEOMETRY split54: 9 steps -> 5 + 4, id 40: 18 -> 6 + 6 + 6 (even slices)
    ("wino-ragged",  176,  72, 14,  32, 2, 3, 1, 1, 1, "conv"),     # WINO_GEOMETRY split_ragged: 11 / 22 steps, block counts of 42 and 43 differ
    ("wino-strip",    32,  40,  2,  66, 3, 3, 1, 1, 1, "conv"),     # WINO_GEOMETRY strip: TH 1
    ("stem",           3,  64, 26,  38, 3, 7, 2, 3, 1, "conv"),     # 7x7 / 2 on a 3-channel image
    ("deconv",        64,   18,  6,   9, 3, 4, 2, 1, 1, "deconv2x"),   # four parity classes, K 256
    ("ws-64",         64, 256, 13,  19, 3, 1, 1, 0, 1, "conv"),     # weight-stationary 1x1: 64 -> 256
    ("ws-128",       128, 128, 13,  19, 3, 1, 1, 0, 1, "conv"),     # ... and 128 -> 128
    # Layers where the split is NOT capped at KT / 4, so ceil(target / blocks) decides: the nominal bm x bn of an id, the default targets
    # (768, Winograd 512) and split_target=1024 all show in ksplit.  Blocks below are (pixel blocks) x (channel blocks).
    # 36 steps (cap 9), M 24444, Cout 192: 256x256 96 x 1 -> 8; 128x256 191 x 1 -> 5; 256x128 96 x 2 -> 4 (target 1024: 6);
    # 128x128 191 x 2 and below: no split, 3 or 2 with target 1024 -- the large tiles tell each other apart
    ("split-large",  128, 192, 126, 194, 1, 3, 1, 1, 1, "conv"),
    # 72 steps (cap 18; id 13: 36, id 15: 144), M 4092, Cout 136: 64x64 64 x 3 -> 4 (6); 64x128 64 x 2 -> 6 (8); 128x64 32 x 3 -> 8 (11);
    # 128x128 32 x 2 -> 12 (16); 128x32 32 x 5 -> 5 (7); id 15 -> 12 (16) of 36 -- the small tiles
    ("split-small",  256, 136,  62,  66, 1, 3, 1, 1, 1, "conv"),
    # Winograd: 128 blocks of 64 tiles x 1 channel block; 41-43: 24 steps (cap 6), 40: 48 (cap 12) -> 512 / 128 = 4 (768 would give 6; 1024: 6 / 8)
    ("wino-target",  384,  64, 128, 256, 1, 3, 1, 1, 1, "conv"),
]
# layers large enough for the other answers of conv_pick_tile: without tile= only (they need no kernel id to tell them apart)
_PICK = [
    ("pick-1",         8,  64, 256, 256, 1, 1, 1, 0, 1, "conv"),    # Cout_store 64 with 512 blocks of 128x64: id 1
    ("pick-2",         8, 128, 128, 192, 1, 1, 1, 0, 1, "conv"),    # 384 blocks of 64x128: id 2
    ("pick-0",         8, 128, 256, 256, 1, 1, 1, 0, 1, "conv"),    # 512 blocks of 128x128: id 0
    ("pick-4",        32,  18,  13,  19, 3, 3, 1, 1, 1, "conv"),    # Cout_store <= 32: id 4 (3 in f16 mode)
]
_KEYS = ("Cin", "Cout", "H", "W", "N", "k", "s", "p", "d", "mode")
LAYERS = collections.OrderedDict((l[0], dict(zip(_KEYS, l[1:]), ids=IDS)) for l in _L)
LAYERS.update((l[0], dict(zip(_KEYS, l[1:]), ids=[None])) for l in _PICK)


def plan_text(layer, mode, tile, split):
    g = LAYERS[layer]
    b = Builder(g["N"])
    b.options += ["graph=0", MODES[mode]]
    if g["mode"] == "deconv2x":
        Ho, Wo = 2 * g["H"], 2 * g["W"]
    else:
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(g["k"]), pair(g["s"]), pair(g["p"]), pair(g["d"])
        Ho, Wo = (g["H"] + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (g["W"] + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if mode == "f16-half":
        x, y = b.hbuf((g["Cin"] + 7) // 8 * 8, g["H"], g["W"]), b.hbuf((g["Cout"] + 7) // 8 * 8, Ho, Wo)
        x, y = x.sub(0, g["Cin"]), y.sub(0, g["Cout"])
    else:
        x, y = b.buf(g["Cin"], g["H"], g["W"]), b.buf(g["Cout"], Ho, Wo)
    t = ["conv name=c in=%s out=%s w=c_w act=0 slope=0.1 cin=%d cout=%d mode=%s" % (x.ref(), y.ref(), g["Cin"], g["Cout"], g["mode"])]
    if g["mode"] == "conv":
        t.append("k=%d,%d s=%d,%d p=%d,%d d=%d,%d" % (pair(g["k"]) + pair(g["s"]) + pair(g["p"]) + pair(g["d"])))
    if tile is not None:
        t.append("tile=%d" % tile)
    if SPLITS[split]:
        t.append(SPLITS[split])
    b.lines.append(" ".join(t))
    return b.text()


def weights(layer):
    g = LAYERS[layer]
    kh, kw = pair(g["k"])
    shape = (g["Cin"], g["Cout"], 4, 4) if g["mode"] == "deconv2x" else (g["Cout"], g["Cin"], kh, kw)
    return (np.random.default_rng(0).standard_normal(shape) / np.sqrt(g["Cin"] * kh * kw)).astype(np.float32)


def rows(layers=None):
    """the grid (of the layers named: all) in file order: (key, layer, mode, split); a row holds one answer per id of the layer"""
    for layer in LAYERS:
        if layers is None or layer in layers:
            for mode in MODES:
                for split in SPLITS:
                    yield "%s|%s|%s" % (layer, mode, split), layer, mode, split


def write(table, path):
    """the table as a file with one line per refusal and per row"""
    import json
    with open(path, "w") as f:
        f.write('{"errors": [\n')
        f.write(",\n".join(" " + json.dumps(e) for e in table["errors"]))
        f.write('\n],\n"rows": {\n')
        f.write(",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table["rows"].items()))
        f.write("\n}}\n")


def merge(table, more):
    """the rows of `more` added to (or replacing those of) `table`, its refusals renumbered into the table's list; rows in grid order"""
    errors = list(table["errors"])
    merged = dict(table["rows"])
    for key, answers in more["rows"].items():
        out = []
        for a in answers:
            if isinstance(a, int):
                if more["errors"][a] not in errors:
                    errors.append(more["errors"][a])
                a = errors.index(more["errors"][a])
            out.append(a)
        merged[key] = out
    return {"errors": errors, "rows": collections.OrderedDict((k, merged[k]) for k, _, _, _ in rows() if k in merged)}


def record(ctx, layers=None, keys=None):
    """{"errors": [distinct messages], "rows": {key: [answer per id]}} of the layers (of the rows) named, default all; an answer is
    [tile, ksplit, narrow] or the index of its message"""
    from accel_amd import runtime
    saved = {k: os.environ.pop(k, None) for k in ("ACCEL_SPLIT", "ACCEL_WITHHOLD", "ACCEL_WB3_FORCE")}
    saved["ACCEL_AUTOTUNE"] = os.environ.get("ACCEL_AUTOTUNE")
    os.environ["ACCEL_AUTOTUNE"] = "0"
    errors, out = [], collections.OrderedDict()
    try:
        for key, layer, mode, split in rows(layers):
            if keys is not None and key not in keys:
                continue
            m = runtime.Model(ctx)      # (one model per row: its plans share the weights)
            try:
                m.set_params({"c_w": weights(layer)})
                answers = []
                for i, tile in enumerate(LAYERS[layer]["ids"]):
                    try:
                        plan = m.add_plan("p%d" % i, plan_text(layer, mode, tile, split))
                        plan.finalize()
                        (op,) = plan.ops()
                        answers.append([op["tile"], op["ksplit"], op["narrow"]])
                    except runtime.AccelError as e:
                        if str(e) not in errors:
                            errors.append(str(e))
                        answers.append(errors.index(str(e)))
                out[key] = answers
            finally:
                m.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return {"errors": errors, "rows": out}
