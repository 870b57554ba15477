"""The streaming attention kernels keep their bits: every case of tests/stream_bits_ref.py - all instantiations of the
streaming forward, the ragged forward, the two-launch backward and the ragged backward, in both operand builds - is recomputed through the public
ops wrappers and the sha256 of every buffer it writes is compared with tests/golden/stream_attention_bits.json, recorded by
scripts/make_golden_stream_bits.py on the build before the forward bodies, the launchers and the tile product were each written once."""
import json
import os

import pytest

from conftest import GOLDEN
import stream_bits_ref as SB
from test_hip_residual_sparse import _dev

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(GOLDEN, "stream_attention_bits.json")))


def test_fixture_holds_every_case_of_the_table():
    assert len(SB.case_ids()) == SB.N_CASES == 85
    assert sorted(FIXTURE) == sorted(SB.MODES)
    for mode in SB.MODES:
        assert sorted(FIXTURE[mode]) == sorted(SB.case_name(c) for c in SB.case_ids())


@pytest.mark.parametrize("mode", SB.MODES)
def test_every_case_has_the_recorded_bits(mode):
    dev = _dev()
    bad = []
    for cid in SB.case_ids():
        name = SB.case_name(cid)
        got, want = SB.run_case(cid, mode, dev), FIXTURE[mode][name]
        assert got["shapes"] == want["shapes"] and got["seed"] == want["seed"], name
        assert sorted(got["sha256"]) == sorted(want["sha256"]), name
        bad += [f"{name}:{k}" for k in want["sha256"] if got["sha256"][k] != want["sha256"][k]]
    assert not bad, f"{len(bad)} buffers changed their bits ({mode}): {bad[:12]}"
