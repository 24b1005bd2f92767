"""The inputs of the "x0_clip" GPU tests (tests/test_gpu_x0_clip.py) and their CPU references - test infrastructure.  Each
reference is computed once per process and shared: tests/test_x0_clip_cpu.py checks on the references alone that every
case exercises the bounds it claims, the GPU tests hold the engine to the same tensors.

Shapes: B = 2, T = 40, testlib.hp_of(layers=3, k=3) (64 channels, 200 steps).  The seeds below were picked
on the CPU, before any GPU run, until the conditions of test_x0_clip_cpu.py::test_gpu_cases_exercise_the_clamp held: with
this synthetic network an unguided or weakly guided (w = 0.5) prediction lies in about [-0.6, 0.6] - it crosses 0 on half
of its elements and never reaches 1 or -1 - while at w = 3 a few per cent leave [-1, 1] on either side.  So the lower
bound of code 1 is claimed by every case, the upper bound and both bounds of code 2 by the w = 3 cases alone; code 2 at
w <= 0.5 moves nothing (asserted as such) and is kept as the engine's inert case."""
import functools

import torch

from oracle import diffroll_ref as R
from testlib import ATOL, HOP, S, hp_of, inputs

import chain_ref as CR
import clip_ref as CL

B, TN = 2, 40
PARAM_SEED, INPUT_SEED, PHILOX_SEED = 0, 100, 9

# (sampler, w, code, bounds the case claims to move: "lo" / "hi")
MATRIX = [
    ("ddpm_x0", 0.0, 1, ("lo",)),
    ("cfdg_ddpm_x0", 0.5, 1, ("lo",)),
    ("cfdg_ddpm_x0", 3.0, 1, ("lo", "hi")),
    ("generation_ddpm_x0", 0.0, 1, ("lo",)),
    ("cfdg_ddim_x0", 0.5, 1, ("lo",)),
    ("ddpm_x0", 0.0, 2, ()),
    ("cfdg_ddpm_x0", 0.5, 2, ()),
    ("cfdg_ddpm_x0", 3.0, 2, ("lo", "hi")),
    ("generation_ddpm_x0", 0.0, 2, ()),
    ("cfdg_ddim_x0", 0.5, 2, ()),
]
NS = (0, 4, 20)          # 0: all S steps; 4: the smallest chain with a second-order step; 20
CASES = [(s, w, c, n) for s, w, c, _ in MATRIX for n in NS]      # every case at every n: 30
CASE_IDS = [f"{s}-w{w:g}-code{c}-n{n or S}" for s, w, c, n in CASES]

# the guided case the option tests run: cfdg_ddpm_x0, w = 3, n = 20, code 1 - (name, keyword arguments of the chain)
OPTION_CASES = [
    ("order1", dict(order=1)),
    ("order2", dict(order=2)),
    ("order1-noise", dict(order=1, solver_noise=1)),
    ("order2-noise", dict(order=2, solver_noise=1)),
    ("interval", dict(interval=(60, 140))),
]


@functools.lru_cache(maxsize=None)
def setup():
    hp = hp_of(layers=3, k=3)
    p = R.synthetic_params(hp, seed=PARAM_SEED)
    wav, x, noise = inputs(B, TN, INPUT_SEED)
    return hp, p, wav, x, noise, R.frontend(wav, hp, TN)


@functools.lru_cache(maxsize=None)
def philox_z():
    return CR.philox_noise(PHILOX_SEED, 0, S, B, TN)


@functools.lru_cache(maxsize=None)
def _reference(sampler, w, code, n, philox, opts):
    hp, p, _, x, noise, spec = setup()
    return CL.sample_chain(p, hp, sampler, x, spec, philox_z() if philox else noise, n, code=code, w=w, **dict(opts))


def reference(sampler, w, code, n, philox=False, **opts):
    """(final roll, {t: (share below lo, share above hi)}) of the restatement - shared, never modified."""
    return _reference(sampler, w, code, n, philox, tuple(sorted(opts.items())))


def in_range(roll, hp, code) -> bool:
    """Every element of a clipped final roll lies in [lo / c2, hi / c2], c2 the committed fp32 sqrt_acp[0]: the last step is
    y / c2 of a clamped y, and a correctly rounded division is monotonic."""
    lo, hi = CL.BOUNDS[code]
    c2 = torch.tensor(CL.last_scale(hp), dtype=torch.float32)
    roll = roll.detach().cpu()
    return bool((roll >= torch.tensor(lo) / c2).all() and (roll <= torch.tensor(hi) / c2).all())


# ---------------------------------------------------------------------------------------------- the two larger geometries
FUSED_SEL = [0, 15]      # the restated clips of the fused case (clips are independent: the others add CPU time, not coverage)


@functools.lru_cache(maxsize=None)
def fused_case():
    """The fused path's geometry of test_gpu_solver_noise.py: 16 guided clips x 125 frames at C = 512, 3 layers - four row
    tiles of the tail kernel's part T3 recompute every update, every Philox draw and now every clamp.  w = 3, n = 20, the
    stochastic order 2 (the seed is read, the clamped prediction is the history), code 1."""
    hp = hp_of(channels=512, layers=3)
    p = R.synthetic_params(hp, seed=11)
    wav, x, _ = inputs(16, 125, 76)
    return hp, p, wav, x


@functools.lru_cache(maxsize=None)
def fused_reference(code=1, seed=5):
    """(roll, moved) of clips FUSED_SEL with the Philox draws of `seed` replayed; code 0: the unclipped chain."""
    hp, p, wav, x = fused_case()
    z = CR.philox_rows(seed, FUSED_SEL, S, 20, 125)
    return CL.sample_chain(p, hp, "cfdg_ddpm_x0", x[FUSED_SEL], R.frontend(wav[FUSED_SEL], hp, 125), z, 20, code=code, w=3.0,
                           order=2, solver_noise=1)


@functools.lru_cache(maxsize=None)
def long_case():
    """Long-form windows as test_gpu_solver_noise.py sizes them: three 640-frame windows sharing 160 frames, C = 128."""
    from diffroll_amd import longform
    hp = hp_of(channels=128, layers=3)
    p = R.synthetic_params(hp, seed=81)
    g = torch.Generator().manual_seed(81)
    L = 1400 * HOP - 100
    plan = longform.plan_windows(L, HOP, overlap=160)
    assert plan.n == 3
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    return hp, p, plan, wav, x_T


LONG_SEED, LONG_REC = 21, 2


@functools.lru_cache(maxsize=None)
def long_inputs(n=20):
    """(x_T gathered into its windows, their spectrograms, {t: the canvas draw of step t gathered into the windows})."""
    from diffroll_amd import longform
    from oracle import philox
    hp, p, plan, wav, x_T = long_case()
    z = {t: longform.gather_windows(torch.from_numpy(philox.step_noise(LONG_SEED, LONG_REC, 1, plan.T_c * 88, t)).reshape(plan.T_c, 88),
                                    plan).unsqueeze(1)
         for t in CR.visited(S, n) if t > 0}
    xw = longform.gather_windows(x_T.reshape(plan.T_c, 88), plan).unsqueeze(1)
    return xw, R.frontend(longform.window_audio(wav, plan, HOP), hp, plan.T), z


@functools.lru_cache(maxsize=None)
def long_reference(code=1):
    """cfdg_ddpm_x0, w = 3, n = 20 on the windows of long_case, Philox keyed by the canvas; code 0: the unclipped chain."""
    hp, p, plan, _, _ = long_case()
    xw, spec, z = long_inputs()
    return CL.sample_chain(p, hp, "cfdg_ddpm_x0", xw, spec, z, 20, code=code, w=3.0, plan=plan)


# ---------------------------------------------------------------------------------------------- do the inputs clamp at all?
def exercised(moved, claims, roll, unclipped):
    """The conditions a case's reference must meet for the case to test the clamp: each bound it claims moves at least 1 % of
    the elements at some visited step, no step has more than 90 % moved, and the clipped roll is at least 100 ATOL away from
    the unclipped one.  A case that claims nothing is the inert one: nothing moves and the two rolls are equal."""
    lo = max(v[0] for v in moved.values())
    hi = max(v[1] for v in moved.values())
    worst = max(v[0] + v[1] for v in moved.values())
    diff = float((roll - unclipped).abs().max())
    print(f"\nmoved by lo: up to {lo:.3f} of a step's elements, by hi: up to {hi:.3f}; max |clipped - unclipped| {diff:.3e}")
    if not claims:
        assert lo == 0.0 and hi == 0.0 and torch.equal(roll, unclipped)
        return
    for bound, share in (("lo", lo), ("hi", hi)):
        if bound in claims:
            assert share >= 0.01, (bound, share)
    assert worst <= 0.90, worst
    assert diff >= 100 * ATOL, diff


def claims_of(sampler, w, code):
    return next(c for s, w_, code_, c in MATRIX if (s, w_, code_) == (sampler, w, code))


def assert_exercised(sampler, w, code, n, philox=False, **opts):
    """... of a case of MATRIX (or the guided case under options), and the final roll's range; returns the reference roll."""
    roll, moved = reference(sampler, w, code, n, philox, **opts)
    unclipped, _ = reference(sampler, w, 0, n, philox, **opts)
    exercised(moved, claims_of(sampler, w, code), roll, unclipped)
    assert in_range(roll, setup()[0], code)
    return roll
