"""GPU: every refusal of the feature front end, byte for byte.  tests/front_refusal_cases.py runs its cases -- the feature
types a handle can and cannot take, every built type against all eight batch calls, a ROI and a grid under every type, the
shapes and batch sizes the families refuse -- and the list of [case, return code, sf_last_error text, feature type after, store
size after] must equal tests/golden/front_refusals.json, which was recorded from the library of the commit named in the
fixture ("recorded_at"), before the front end's host code was split by concern."""
import json

import pytest

from tests import front_refusal_cases as cases

pytestmark = pytest.mark.gpu


def test_refusals_match_the_recorded_parent():
    with open(cases.GOLDEN) as fh:
        golden = json.load(fh)
    want = golden["cases"]
    assert golden["recorded_at"] and len(want) == 4 * 11 + 8 * (16 + 4) + 8
    got = cases.run_all()
    assert [g[0] for g in got] == [w[0] for w in want], "the list of cases is not the recorded one: record the fixture again"
    for g, w in zip(got, want):
        assert g == w, "case %r: got %r, recorded %r" % (g[0], g[1:], w[1:])
    # the cases are worth their name: refusals of every code the front end gives, and calls that were let through
    codes = {w[1] for w in want}
    assert 0 in codes and len(codes) >= 3
