#!/usr/bin/env python
"""Record what finalize answers for the launch-geometry grid of tests/conv_geometry.py into tests/golden/conv_geometry.json: run it on
the MI355X at the commit whose behaviour is to be pinned and commit the file; tests/test_conv_geometry_gpu.py replays the grid against
it.  Plans are finalized and never run: no convolution is launched.
    record_conv_geometry.py [--out FILE] [--layers a,b,...]
--layers records those layers alone and merges their rows into the file that is there (layers added to the grid later)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

import conv_geometry as G      # noqa: E402
from accel_amd import runtime      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=G.GOLDEN)
    ap.add_argument("--layers", default=None)
    a = ap.parse_args()
    layers = a.layers.split(",") if a.layers else None
    ctx = runtime.Context(0)
    t0 = time.time()
    try:
        got = G.record(ctx, layers)
    finally:
        ctx.close()
    if layers:
        with open(a.out) as f:
            got = G.merge(json.load(f, object_pairs_hook=G.collections.OrderedDict), got)
    G.write(got, a.out)
    n = sum(len(v) for v in got["rows"].values())
    print("%d answers (%d distinct refusals) in the file, recorded in %.1f s -> %s" % (n, len(got["errors"]), time.time() - t0, a.out))


if __name__ == "__main__":
    main()
