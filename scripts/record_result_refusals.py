"""Records what the library answers to the refused calls of tests/result_refusals.py into tests/golden/result_refusals.json (or the file given):
    ACCEL_LIB_PATH=<the library to pin> python scripts/record_result_refusals.py [out.json]
Needs the GPU (a context and three small models are created); the refused calls themselves enqueue nothing.  A case that is NOT refused is an
error of the case list, and nothing is written."""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import result_refusals
    from accel_amd import runtime
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "result_refusals.json")
    ctx = runtime.Context(0)
    try:
        got = result_refusals.replay(runtime, ctx)
    finally:
        ctx.close()
    accepted = [k for k, v in got.items() if v["rc"] == 0]
    if accepted:
        sys.exit("accepted, not refused: %s" % ", ".join(accepted))
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d refusals of %s -> %s" % (len(got), runtime.LIB_PATH, out))


if __name__ == "__main__":
    main()
