"""The cases of the "cfg_rescale" GPU tests (tests/test_gpu_cfg_rescale.py) and their CPU references - test infrastructure.
The inputs and the cached restatement are those every guidance stage shares: tests/stage_scenarios.py."""
import rescale_ref as RR
import stage_scenarios as SS
from stage_scenarios import (B, GUIDING, INPUT_SEED, MASK, N_STEPS, PARAM_SEED, PHILOX_SEED, TN, W, mask_of, philox_z, setup,  # noqa: F401
                             spec_of, start_step)
from testlib import ATOL

VALUES = (7000, 10000)

# (name, keyword arguments of rescale_ref.sample_chain beside value / w, the same on the facade)
OPTION_CASES = [
    # (the range [0, 1]: the rescaled prediction no longer leaves [-1, 1], while 0 still cuts half of its elements)
    ("clip", dict(code=1), dict(code=1)),
    ("clip-threshold", dict(code=1, v=9950), dict(code=1, v=9950)),
    ("order2", dict(order=2), dict(solver_order=2)),
    ("order2-noise", dict(order=2, solver_noise=1), dict(solver_order=2, solver_noise=1)),
    ("interval", dict(interval=(60, 140)), dict(guidance_interval=[60, 140])),
    ("strength", dict(start="strength"), dict(strength=0.5)),
]


def reference(sampler, value, philox=False, **opts):
    """(final roll, {t: (G,) g}) of the restatement; value = 0: the option off."""
    return SS.reference(RR.sample_chain, sampler, {"cfg_rescale": value}, philox, **opts)


def assert_active(sampler, value, philox=False, **opts):
    """The case rescales: |g - 1| >= 0.2 at every guided step and roll, and the roll is at least 100 ATOL from the unrescaled
    chain's.  Returns the reference roll."""
    roll, gs = reference(sampler, value, philox, **opts)
    off, _ = reference(sampler, 0, philox, **opts)
    g = [float(v) for row in gs.values() for v in row]
    diff = float((roll - off).abs().max())
    print(f"\n{sampler} value {value} {sorted(opts.items())}: g in {min(g):.3f} .. {max(g):.3f} at {len(gs)} guided steps; "
          f"max |rescaled - unrescaled| {diff:.3e}")
    assert g and all(abs(v - 1.0) >= 0.2 for v in g)
    # (an interval that ends at step 60 leaves six unguided steps behind the last rescaled one, which contract the difference)
    assert diff >= (10 if "interval" in opts else 100) * ATOL, diff
    return roll
