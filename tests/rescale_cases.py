"""The inputs of the "cfg_rescale" GPU tests (tests/test_gpu_cfg_rescale.py) and their CPU references - test
infrastructure.  Each reference is computed once per process and shared; it is never modified.

Shapes: B = 2, T = 40, hp_of() of test_gpu_respaced.py (64 channels, 4 layers, k = 9, 200 steps), 20 visited steps, w = 3.
The inpainting sampler's time mask covers spectrogram frames [10, 20)."""
import functools

from oracle import diffroll_ref as R
from test_gpu_respaced import S, hp_of, inputs

import chain_ref as CR
import rescale_ref as RR

B, TN, N_STEPS, W = 2, 40, 20, 3.0
PARAM_SEED, INPUT_SEED, PHILOX_SEED = 0, 100, 9
MASK = [10, 20]
GUIDING = ("cfdg_ddpm_x0", "inpainting_ddpm_x0", "cfdg_ddim_x0")
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


def mask_of(sampler):
    return MASK if sampler == "inpainting_ddpm_x0" else None


@functools.lru_cache(maxsize=None)
def setup():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=PARAM_SEED)
    wav, x, noise = inputs(B, TN, INPUT_SEED)
    return hp, p, wav, x, noise


@functools.lru_cache(maxsize=None)
def spec_of(sampler):
    hp, _, wav, _, _ = setup()
    return R.frontend(wav, hp, TN, inpainting_t=mask_of(sampler))


@functools.lru_cache(maxsize=None)
def philox_z():
    return CR.philox_noise(PHILOX_SEED, 0, S, B, TN)


def start_step(strength=0.5):
    """The visited step a chain of that strength begins at (schedule.check_start)."""
    from diffroll_amd.schedule import check_start
    return check_start(None, strength, CR.visited(S, N_STEPS))


@functools.lru_cache(maxsize=None)
def _reference(sampler, value, philox, opts):
    hp, p, _, x, noise = setup()
    kw = dict(opts)
    if kw.get("start") == "strength":
        kw["start"] = start_step()
    return RR.sample_chain(p, hp, sampler, x, spec_of(sampler), philox_z() if philox else noise, N_STEPS, value=value, w=W, **kw)


def reference(sampler, value, philox=False, **opts):
    """(final roll, {t: (G,) g}) of the restatement; value = 0: the option off."""
    return _reference(sampler, value, philox, tuple(sorted(opts.items())))


def assert_active(sampler, value, philox=False, **opts):
    """The case rescales: |g - 1| >= 0.2 at every guided step and roll, and the roll is at least 100 ATOL from the unrescaled
    chain's.  Returns the reference roll."""
    from test_gpu_respaced import ATOL
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
