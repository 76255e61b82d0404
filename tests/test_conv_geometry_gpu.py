"""What finalize answers for every launch geometry id, pinned: the grid of conv_geometry.py (layers x plan modes x ids 0..99 and no
tile= x split settings) against tests/golden/conv_geometry.json, which scripts/record_conv_geometry.py recorded from this code base
before the launch-geometry table (csrc/conv_tiles.h) replaced the hand-written id ranges.  Equality, answer by answer: the
(tile, ksplit, narrow) of Plan.ops(), or the error text of the refusal.  The plans are finalized and never run.  One case per row of the grid
(layer, mode, split setting): the deep layers cost up to 15 ms a finalize."""
import json

import pytest

import conv_geometry as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(G.GOLDEN) as f:
        return json.load(f)


def test_the_file_holds_the_grid(recorded):
    assert list(recorded["rows"]) == [key for key, _, _, _ in G.rows()]


@pytest.mark.parametrize("key", [key for key, _, _, _ in G.rows()])
def test_finalize_answers_as_recorded(ctx, recorded, key):
    """one row of the grid: a layer in one plan mode under one split setting, every id"""
    got = G.record(ctx, keys=[key])
    text = lambda table, a: table["errors"][a] if isinstance(a, int) else a
    ids = G.LAYERS[key.split("|")[0]]["ids"]
    assert list(got["rows"]) == [key] and len(got["rows"][key]) == len(recorded["rows"][key]) == len(ids), key
    wrong = ["tile=%s: %r, recorded %r" % (tile, text(got, g), text(recorded, w))
             for tile, g, w in zip(ids, got["rows"][key], recorded["rows"][key]) if text(got, g) != text(recorded, w)]
    assert not wrong, "%s: %d answers differ from the record:\n%s" % (key, len(wrong), "\n".join(wrong[:40]))
