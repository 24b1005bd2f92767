"""The inputs of the "guidance_stride" tests (tests/test_guidance_stride_cpu.py, tests/test_gpu_guidance_stride.py) and their CPU
references - test infrastructure.  Each reference is computed once per process and shared; it is never modified.

The inputs are those every guidance stage shares (tests/stage_scenarios.py): B = 2, T = 40, testlib.hp_of() (64 channels,
4 layers, k = 9, 200 steps), 20 visited steps, w = 3; the inpainting sampler's time mask covers spectrogram frames [10, 20)."""
import functools

import stage_scenarios as SS
import stride_ref as SR
from stage_scenarios import B, GUIDING, N_STEPS, PHILOX_SEED, TN, W, mask_of, philox_z, setup, spec_of, start_step  # noqa: F401
from testlib import ATOL

STRIDES = (2, 3)
MAIN = 2

# (name, keyword arguments of stride_ref.sample_chain beside the stride and w, the same on the facade; n: visited steps)
OPTION_CASES = [
    ("steps", dict(n=10), dict(n=10)),
    # (behind step 60 six unguided steps contract what the reuse steps did: the roll parts from the guided chain's by a few ATOL
    # only - assert_active; the second interval reaches step 0 and keeps the whole difference)
    ("interval", dict(interval=(60, 140)), dict(guidance_interval=[60, 140])),
    ("interval-to-0", dict(interval=(0, 140)), dict(guidance_interval=[0, 140])),
    ("order2", dict(order=2), dict(solver_order=2)),
    ("order2-noise", dict(order=2, solver_noise=1), dict(solver_order=2, solver_noise=1)),
    ("strength", dict(start="strength"), dict(strength=0.5)),
    # (the range [0, 1]: 0 cuts about half of the prediction's elements, at the refresh and at the reuse steps alike)
    ("clip", dict(code=1), dict(code=1)),
]


def values(stride):
    """The stage's value by option name (stage_scenarios: the keyword of the restatement and the key of hparams.sampling)."""
    return {"guidance_stride": stride}


def set_values(m, vals):
    """stage_scenarios.set_values for this stage: the key holds the integer itself (0: None), not a fraction of 10000."""
    for name, value in vals.items():
        setattr(m.hparams.sampling, name, value or None)


def stride_model(hp, p, sampler, stride, **kw):
    """The facade with hparams.sampling.guidance_stride = stride and the other sampling keys of stage_scenarios.stage_model."""
    m = SS.stage_model(hp, p, sampler, {}, **kw)
    set_values(m, values(stride))
    return m


@functools.lru_cache(maxsize=None)
def _chain(sampler, stride, variant, philox, n, opts):
    hp, p, _, x, noise = setup()
    kw = dict(opts)
    if kw.get("start") == "strength":
        kw["start"] = start_step()
    return SR.sample_chain(p, hp, sampler, x, spec_of(sampler), philox_z() if philox else noise, n, w=W, guidance_stride=stride,
                           variant=variant, **kw)


def reference(sampler, stride, philox=False, variant="d", n=N_STEPS, **opts):
    """(final roll, [(t, what)]) of the restatement on the shared inputs; stride 0: the option off."""
    return _chain(sampler, stride, variant, philox, n, tuple(sorted(opts.items())))


def rms(d):
    return float(d.double().pow(2).mean().sqrt())


def assert_active(sampler, stride, philox=False, **opts):
    """The case reuses: at least one step of the restated chain reuses, the first guided step refreshes, and the roll is at least
    100 ATOL from the fully guided chain's - 5 ATOL where unguided steps follow the interval and contract the difference: an
    engine within ATOL of this roll is then still 4 ATOL from the guided chain's.  Returns the reference roll."""
    roll, sched = reference(sampler, stride, philox, **opts)
    off, sched_off = reference(sampler, 0, philox, **opts)
    whats = [w for _, w in sched]
    guided = [w for w in whats if w != "unguided"]
    diff = float((roll - off).abs().max())
    print(f"\n{sampler} guidance_stride {stride} {sorted(opts.items())}: {whats.count('refresh')} refresh, {whats.count('reuse')} reuse, "
          f"{whats.count('unguided')} unguided steps; max |strided - guided| {diff:.3e}")
    assert "reuse" in whats and guided[0] == "refresh" and sched[-1] == (0, "refresh" if sched_off[-1][1] != "unguided" else "unguided")
    assert [w for _, w in sched_off].count("reuse") == 0
    assert diff >= (5 if sched[-1][1] == "unguided" else 100) * ATOL, diff
    return roll
