"""The result half of the C ABI refuses what it refused before it was rewritten, in the same order and in the same words: every case of
result_refusals.py gives the return code and the whole message recorded in golden/result_refusals.json (scripts/record_result_refusals.py;
addresses printed by %p are one fixed token on both sides).  Refused calls enqueue nothing: the test takes a second or two."""
import json
import os

import pytest

import result_refusals

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "result_refusals.json")


def test_every_refusal_is_the_recorded_one(ctx):
    from accel_amd import runtime
    with open(GOLDEN) as f:
        want = json.load(f)
    got = result_refusals.replay(runtime, ctx)
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    wrong = ["%s: (%d) %r, recorded (%d) %r" % (k, got[k]["rc"], got[k]["message"], want[k]["rc"], want[k]["message"])
             for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "\n".join(wrong)
    assert all(v["rc"] != 0 for v in got.values())
