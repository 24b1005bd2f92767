"""The inputs of the "x0_threshold" GPU tests (tests/test_gpu_x0_threshold.py) and their CPU references - test
infrastructure, on the shapes, seeds and tensors of clip_cases.py.  Each reference is computed once per process and shared:
tests/test_x0_threshold_cpu.py checks on the references alone that every case is active (s > r at every visited step and
roll) or inert (at none) as it claims, the GPU tests hold the engine to the same tensors.

With the synthetic network of clip_cases.setup() an unguided or weakly guided prediction lies in about [-0.6, 0.6], at w = 3
a few per cent leave [-1, 1].  So under code 2 ([-1, 1], m = 0, r = 1) only w = 3 at a high percentile is active, while under
code 1 ([0, 1], m = r = 0.5) |y - 0.5| exceeds 0.5 on the half of the elements below 0: every case is active."""
import functools

import clip_cases as CC
import thresh_ref as TR
from testlib import ATOL

# (sampler, w, code, v)
ACTIVE = [
    ("cfdg_ddpm_x0", 3.0, 2, 9950),
    ("cfdg_ddpm_x0", 3.0, 1, 9950),
    ("cfdg_ddpm_x0", 0.5, 1, 9000),
    ("ddpm_x0", 0.0, 1, 9950),
    ("generation_ddpm_x0", 0.0, 1, 9000),
    ("cfdg_ddim_x0", 0.5, 1, 9950),
]
INERT = [
    ("cfdg_ddpm_x0", 3.0, 2, 9000),
    ("cfdg_ddpm_x0", 0.5, 2, 9950),
    ("ddpm_x0", 0.0, 2, 9000),
]
NS = CC.NS
CASES = [(s, w, c, v, n) for s, w, c, v in ACTIVE for n in NS]
CASE_IDS = [f"{s}-w{w:g}-code{c}-v{v}-n{n or CC.S}" for s, w, c, v, n in CASES]
GUIDED = ("cfdg_ddpm_x0", 3.0, 2, 9950)          # the guided active case the option tests run, n = 20

OPTION_CASES = [
    ("order1", dict(order=1)),
    ("order2", dict(order=2)),
    ("order2-noise", dict(order=2, solver_noise=1)),
    ("interval", dict(interval=(0, 140))),           # (guided to the end: an interval that ends early leaves the last steps inert)
]


@functools.lru_cache(maxsize=None)
def _reference(sampler, w, code, v, n, philox, opts):
    hp, p, _, x, noise, spec = CC.setup()
    return TR.sample_chain(p, hp, sampler, x, spec, CC.philox_z() if philox else noise, n, code=code, v=v, w=w, **dict(opts))


def reference(sampler, w, code, v, n, philox=False, **opts):
    """(final roll, {t: (G, 2) {q, s}}, r) of the restatement - shared, never modified.  v = 0: the clipped chain, which is
    clip_cases' reference."""
    if v == 0:
        return CC.reference(sampler, w, code, n, philox, **opts)[0], {}, TR.centre(code)[1]
    return _reference(sampler, w, code, v, n, philox, tuple(sorted(opts.items())))


def assert_active(sampler, w, code, v, n, philox=False, **opts):
    """An active case: s > r at every visited step and roll - under a guidance interval at every guided step and at no other -
    and the roll at least 100 ATOL from the clipped chain's.  Returns the reference roll."""
    roll, stats, r = reference(sampler, w, code, v, n, philox, **opts)
    flags = TR.active(stats, r)
    if "interval" in opts:      # an unguided step thresholds the conditional prediction alone: under code 2 that is inert
        lo, hi = opts["interval"]
        inside = [lo <= t <= hi for t, s in stats.items() for _ in range(s.shape[0])]
        assert any(inside) and not all(inside)
        assert code == 2 and not any(f for f, i in zip(flags, inside) if not i)
        flags = [f for f, i in zip(flags, inside) if i]
    qs = [float(s[g, 0]) for s in stats.values() for g in range(s.shape[0])]
    clipped = reference(sampler, w, code, 0, n, philox, **opts)[0]
    diff = float((roll - clipped).abs().max())
    print(f"\n{sampler} w {w} code {code} v {v} n {n or CC.S}: q in {min(qs):.3f} .. {max(qs):.3f} (r = {r}), active at {sum(flags)} of "
          f"{len(flags)}; max |thresholded - clipped| {diff:.3e}")
    assert flags and all(flags)
    assert diff >= 100 * ATOL, diff
    return roll


def assert_inert(sampler, w, code, v, n, philox=False):
    """An inert case: s > r at no visited step and roll, and the roll IS the clipped chain's."""
    import torch
    roll, stats, r = reference(sampler, w, code, v, n, philox)
    flags = TR.active(stats, r)
    qs = [float(s[g, 0]) for s in stats.values() for g in range(s.shape[0])]
    print(f"\n{sampler} w {w} code {code} v {v} n {n or CC.S}: q <= {max(qs):.3f} (r = {r})")
    assert flags and not any(flags)
    assert torch.equal(roll, reference(sampler, w, code, 0, n, philox)[0])
    return roll


# ---------------------------------------------------------------------------------------------- the two larger geometries
@functools.lru_cache(maxsize=None)
def fused_reference(v=9950, code=2, seed=5):
    """Clips FUSED_SEL of clip_cases.fused_case(): cfdg_ddpm_x0, w = 3, n = 20, stochastic order 2, Philox of `seed` replayed."""
    import chain_ref as CR
    from oracle import diffroll_ref as R
    hp, p, wav, x = CC.fused_case()
    z = CR.philox_rows(seed, CC.FUSED_SEL, CC.S, 20, 125)
    return TR.sample_chain(p, hp, "cfdg_ddpm_x0", x[CC.FUSED_SEL], R.frontend(wav[CC.FUSED_SEL], hp, 125), z, 20, code=code, v=v, w=3.0,
                           order=2, solver_noise=1)


@functools.lru_cache(maxsize=None)
def long_reference(v=9950, code=2):
    """cfdg_ddpm_x0, w = 3, n = 20 on the windows of clip_cases.long_case(): one q per step over the recording's canvas."""
    hp, p, plan, _, _ = CC.long_case()
    xw, spec, z = CC.long_inputs()
    return TR.sample_chain(p, hp, "cfdg_ddpm_x0", xw, spec, z, 20, code=code, v=v, w=3.0, plan=plan)
