"""CPU restatement of option "exact_below" (include/diffroll_amd.h) - test infrastructure.

It is the restated reduced-precision chain of tests/bf16_ref.py / tests/f16_ref.py - tests/chain_ref.py's chain on the oracle's
residual block with a rounding function at the four operands the header names - with that rounding applied only at the steps
t >= v: the network evaluations of a step t < v are the oracle's own.  Nothing else is restated: the rule is one comparison.
"""
import contextlib

import torch

import bf16_ref as Q
import chain_ref
import f16_ref as H
from bf16_ref import CHAIN_GEOMETRY, CHAIN_STEPS, rms  # noqa: F401  (lent to the tests)

ROUNDINGS = {"bf16": Q.rne, "f16": H.rne}
SAMPLERS = ("cfdg_ddpm_x0", "generation_ddpm_x0", "cfdg_ddim_x0")
W = 0.5
# the restated mixed chains the GPU band is held to (mode, sampler, v), and their rms distance from the fp32 chain as measured
# when the option was designed: all above 1e-5, where the fp32 chain's own noise ends (generation_ddpm_x0 at v = 2 is at 6.6e-6: not a band)
BAND_CASES = [("bf16", "cfdg_ddpm_x0", 1), ("bf16", "cfdg_ddpm_x0", 2), ("bf16", "cfdg_ddim_x0", 1), ("bf16", "cfdg_ddim_x0", 2),
              ("f16", "cfdg_ddpm_x0", 1)]


def step_precision(prec: int, exact_below: int, t: int) -> int:
    """launch_plan.h: step_precision."""
    return 0 if t < exact_below else prec


@contextlib.contextmanager
def patched(rnd, acc, v):
    """For the duration of the block chain_ref's chain takes the prediction of a step t >= v from the restated block with
    this rounding, and that of a step t < v from the oracle's."""
    saved = chain_ref.prediction

    def prediction(params, hp, sampler, x, spec_c, t, w, table):
        if t < v:
            return saved(params, hp, sampler, x, spec_c, t, w, table)
        with Q.patched(rnd, acc):
            return saved(params, hp, sampler, x, spec_c, t, w, table)
    chain_ref.prediction = prediction
    try:
        yield
    finally:
        chain_ref.prediction = saved


def sample_chain(rnd, acc, v, *args, **kw):
    """tests/chain_ref.py's sample_chain, the steps t >= v on the restated block (v = 0: bf16_ref.sample_chain)."""
    with patched(rnd, acc, v):
        return chain_ref.sample_chain(*args, **kw)


_inputs = {}


def chain_inputs():
    """hp, params, x, wav, spec, noise of the 8-step chains on CHAIN_GEOMETRY: the inputs of tests/test_gpu_bf16.py's chains."""
    if not _inputs:
        from oracle import diffroll_ref as R
        hp, p, x, wav, _ = Q.case_inputs(CHAIN_GEOMETRY, timesteps=CHAIN_STEPS)
        B, T = CHAIN_GEOMETRY[3:]
        nz = torch.randn(CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
        with torch.no_grad():
            spec = R.frontend(wav, hp, T)
        _inputs["v"] = (hp, p, x, wav, spec, nz)
    return _inputs["v"]


_chains = {}


def chain(mode, sampler, v, acc=None):
    """The final roll of the restated 8-step chain (computed once per process): mode None = the oracle's fp32 chain."""
    key = (mode, sampler, v if mode else 0, acc)
    if key not in _chains:
        hp, p, x, wav, spec, nz = chain_inputs()
        sc = None if sampler == "generation_ddpm_x0" else spec
        if mode is None:
            _chains[key] = chain_ref.sample_chain(p, hp, sampler, x, sc, nz, 0, w=W)
        else:
            _chains[key] = sample_chain(ROUNDINGS[mode], acc, v, p, hp, sampler, x, sc, nz, 0, w=W)
    return _chains[key]


def distance(mode, sampler, v, acc=None) -> float:
    """rms distance of the restated mixed chain's final roll from the oracle's fp32 chain."""
    return rms(chain(mode, sampler, v, acc) - chain(None, sampler, 0))


# The combinations whose state runs across the boundary and has no twin (dr_set_precision ends it): name -> (the restated chain
# of the combination's own file, what that chain takes, the options of dr_set_option).  Their chain loops ask chain_ref.prediction
# through the module, so patched() restates their mixed chains as it does chain_ref's own.
def _stateful():
    import momentum_ref as MR
    import stride_ref as SR
    return {"cfg_project+cfg_momentum": (MR.sample_chain, dict(cfg_project=10000, cfg_momentum=-5000), dict(cfg_project=10000, cfg_momentum=-5000)),
            "guidance_stride-2": (SR.sample_chain, dict(guidance_stride=2), dict(guidance_stride=2))}


STATEFUL_BAND = [(name, v) for name in ("cfg_project+cfg_momentum", "guidance_stride-2") for v in (1, 3)]


def stateful_options(name):
    return _stateful()[name][2]


def stateful_distance(name, v, acc=None, sampler="cfdg_ddpm_x0", mode="bf16") -> float:
    """rms distance of the restated mixed chain of a stateful combination (8 steps, the steps t >= v in `mode`) from the same
    restated chain in fp32 (computed once per process)."""
    key = ("stateful", name, v, acc, sampler, mode)
    if key not in _chains:
        fn, kw, _ = _stateful()[name]
        hp, p, x, wav, spec, nz = chain_inputs()
        ref_key = ("stateful", name, sampler)
        if ref_key not in _chains:
            _chains[ref_key] = fn(p, hp, sampler, x, spec, nz, 0, w=W, **kw)[0]
        with patched(ROUNDINGS[mode], acc, v):
            _chains[key] = rms(fn(p, hp, sampler, x, spec, nz, 0, w=W, **kw)[0] - _chains[ref_key])
    return _chains[key]
