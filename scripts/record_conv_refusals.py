#!/usr/bin/env python
"""Record the texts finalize refuses the cases of tests/conv_refusals.py with into tests/golden/conv_refusals.json: run it on the MI355X
at the commit whose behaviour is to be pinned and commit the file; tests/test_conv_finalize_gpu.py replays the cases against it.  Plans
are finalized and never run: no convolution is launched.
    record_conv_refusals.py [--out FILE]"""
import argparse
import collections
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

import conv_refusals as R      # noqa: E402
from accel_amd import runtime      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=R.GOLDEN)
    a = ap.parse_args()
    ctx = runtime.Context(0)
    try:
        got = collections.OrderedDict((name, R.answer(ctx, name)) for name in R.CASES)
    finally:
        ctx.close()
    taken = [name for name, text in got.items() if text is None]
    if taken:
        raise SystemExit("finalize takes these cases, nothing to pin: %s" % ", ".join(taken))
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in got.items()) + "\n}\n")
    print("%d refusals -> %s" % (len(got), a.out))


if __name__ == "__main__":
    main()
