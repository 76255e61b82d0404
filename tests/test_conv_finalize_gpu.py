"""What finalize_conv refuses on its own account, pinned: the cases of conv_refusals.py (a view too narrow for the layer, a weight of
the wrong shape, a deconvolution or convolution output of the wrong size, an out2 without its constants, views of different batch
sizes, a view beyond the 4 GiB of a buffer resource, a missing or mis-sized weight, bias or bias2, half views on a layer that cannot
take them) against tests/golden/conv_refusals.json, which scripts/record_conv_refusals.py recorded before finalize_conv was taken
apart into steps.  Whole strings.  The plans are finalized and never run."""
import json

import pytest

import conv_refusals as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(R.GOLDEN) as f:
        return json.load(f)


def test_the_file_holds_the_cases(recorded):
    assert list(recorded) == list(R.CASES)
    assert all(isinstance(text, str) and text for text in recorded.values()), "every case is a refusal"


@pytest.mark.parametrize("name", list(R.CASES))
def test_finalize_refuses_as_recorded(ctx, recorded, name):
    assert R.answer(ctx, name) == recorded[name]
