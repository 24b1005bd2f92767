"""The lab option "zero_taps" on the GPU: the fp32 128-frame conv blocks leave out the MFMAs of an edge tap whose window of the
block's first / last 32-frame tile is all zero padding (csrc/zero_taps.h, csrc/gemm_body.h: stepx).  The products left out are
w * (+0) added to a chain that starts from +0, so NOTHING may change: zero_taps = 1 against zero_taps = 0 is held bit for bit - on
the roll of a 3-step guided chain and on layer 3's gated activation alone, where one wrong element cannot hide - and each to the
oracle at the suite's 1e-5.  tests/zero_taps_cases.py runs all of it once, in a child process whose per-phase kernels are
pinned to the flavours the fused 128-frame kernel is built from (as tests/test_gpu_fused.py pins them); every network has four
layers, because only layer 3 (d = 8) has such a tap at k = 9 - no case of the other suites reaches it on these blocks."""
import json
import os
import subprocess
import sys

import pytest

import zero_taps_cases as Z
from tools import tuning_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def records():
    env = tuning_env.env_with(tune__ksplit_max=1, tune__tile=3202, tune__pw_nw=4, tune__stack_fl=2, blocked_accumulation=2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "zero_taps_cases.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ZERO_TAPS_CASES ")][-1]
    return json.loads(line[len("ZERO_TAPS_CASES "):])


@pytest.mark.parametrize("i", range(len(Z.PER_PHASE)), ids=["k%d-T%d" % c for c in Z.PER_PHASE])
def test_per_phase_launches_give_the_same_bits_with_and_without_the_edge_taps(records, i):
    rec = records["per_phase"][i]
    assert tuple(rec["case"]) == Z.PER_PHASE[i] and rec["mode"] == "per_phase", rec
    assert rec["roll_equal"], rec                              # the 3-step chain's roll
    assert rec["g_equal"] and rec["g_finite_nonzero"], rec     # layer 3's gate, every element
    assert rec["on_vs_oracle"] <= 1e-5 and rec["off_vs_oracle"] <= 1e-5, rec


def test_fused_stack_gives_the_same_bits_with_and_without_the_edge_taps(records):
    rec = records["fused"]
    assert rec["per_phase_equal"] and rec["vs_oracle"] <= 1e-5, rec
    assert [run["xcd"] for run in rec["runs"]] == [1, 0], rec
    for run in rec["runs"]:
        assert run["timed_out"] == 0 and run["launches"] >= 2 and run["kernel"] == "stack_kernel<2>", rec
        assert run["on_equals_per_phase"] and run["off_equals_per_phase"] and run["on_equals_off"], rec
    assert rec["fallbacks"] == 0 and rec["yields"] == 0, rec
