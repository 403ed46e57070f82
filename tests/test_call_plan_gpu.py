"""The plan of a call is what it was: the sweep of tests/call_plan_cases.py (every [first, last], tap, image count and option set over
nets that skip columns, groups, halves and the fourth group of a K walk, and nets that skip nothing) is replayed through the four
sicn_debug_net_* entry points and sicn_debug_plan and held, record for record, to tests/golden/call_plans.json, which was recorded from
the library as it stood before the walks over a call's layers became one (live::plan_call, csrc/sicn_live.h).  No layer is launched: the
device is needed for the nets' weight uploads alone."""
import json

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_every_call_plan_is_the_recorded_one():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    import call_plan_cases as cases
    want = json.loads(cases.FIXTURE.read_text())
    got = list(cases.records())
    assert len(got) == len(want["sweep"]), (len(got), len(want["sweep"]))
    bad = [(key, s, want["strings"][i]) for (key, s), i in zip(got, want["sweep"]) if s != want["strings"][i]]
    assert not bad, f"{len(bad)} of {len(got)} records differ; the first (key, got, recorded): {bad[:3]}"
    # the sweep is not vacuous: some call skips columns, a group, a half and the fourth group of a walk, and some call skips nothing
    layers = [s[i:i + 8] for key, s in got if not key.endswith("kinds") for i in range(0, len(s), 8)]
    for at, values in ((0, "358"), (1, "12"), (2, "34"), (3, "34"), (4, "34")):
        assert {row[at] for row in layers} == set(values), (at, {row[at] for row in layers})
