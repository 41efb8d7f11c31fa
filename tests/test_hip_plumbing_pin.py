"""The host side of the entry points -- operand staging, the rocPRIM calls, the maps between the caller's order and the
cell-sorted one -- held to what the MI355X returned before those pieces were folded into one definition each
(tests/golden/plumbing_pin.npz, written by tools/gen_golden_plumbing_pin.py on that build).  Per call of tests/plumbing_cases.py:
every output bit (as SHA-256), the number of host waits, and the launches per timer name.

The group `shot` was recorded again when K5 was given its order for neighbours at equal distance: every SHOT
entry point then makes one more launch, `k5_shot_ties`.  That recording was written only after it had been compared with the
first one: every output hash and every wait count equal, `k5_shot_ties` the one launch name that differs; the other groups are
the first record's, byte for byte."""
import json

import pytest

import plumbing_cases as P
from conftest import load_golden


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(P.GROUPS))
def test_calls_are_the_recorded_ones(group):
    want = json.loads(str(load_golden("plumbing_pin.npz")[group]))
    got = P.run_group(group)
    assert set(got) == set(want), set(got) ^ set(want)
    wrong = {c: (got[c], want[c]) for c in got if got[c] != want[c]}
    assert not wrong, wrong
