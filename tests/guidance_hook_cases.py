"""Child of tests/test_gpu_guidance_interval.py::test_checked_rerun_uses_the_same_interval: runs under DR_LIB=<the "hook"
variant>, the only build of the library that knows the option "stack_fault_test" (tests/hook_cases.py).  Not collected by a
plain `pytest tests` (the file name does not match)."""
import pytest
import torch

from oracle import diffroll_ref as R
from testlib import make_model, maxdiff

import chain_ref as CR

pytestmark = pytest.mark.gpu


def test_this_is_the_hook_build():
    import os
    from diffroll_amd import _cabi
    assert "hook" in os.path.basename(_cabi.LIB_PATH), "run through tests/test_gpu_guidance_interval.py (DR_LIB = the hook variant)"


def test_checked_rerun_returns_the_per_phase_roll_of_the_same_interval():
    """stack_fault_test = 1: the first group barrier of the chain's first fused launch runs into its spin bound, the rest of
    the chain returns at once, dr_sample_checked heals and re-runs per phase - under the interval that is still set."""
    S, B, T, W = 12, 2, 125, 0.5
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=64, residual_layers=3, kernel_size=3, timesteps=S)
    p = R.synthetic_params(hp, seed=70)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=W)
    m.hparams.sampling.guidance_interval = [4, 8]
    g = torch.Generator().manual_seed(81)
    wav = 0.1 * torch.randn(B, T * 512, generator=g)
    x = torch.randn(B, 1, T, 88, generator=g)
    noise = torch.randn(S, B, 1, T, 88, generator=g)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, T), noise, 0, w=W, interval=(4, 8))
    eng = m.engine
    eng.set_option("fused_stack", 0)
    per_phase, _ = m.sample(x, wav, noise=noise)
    assert maxdiff(per_phase.cpu(), ref) <= 1e-5
    eng.set_option("fused_stack", 2)
    eng.set_option("stack_fault_test", 1)
    try:
        roll, _ = m.sample(x, wav, noise=noise)               # ONE call of dr_sample_checked
    finally:
        eng.set_option("stack_fault_test", 0)
    assert eng.fallbacks == 1 and eng.guidance_interval == (4, 8)
    assert eng.launch_state()["mode"] == "per_phase"
    assert torch.equal(roll, per_phase)
    full = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, T), noise, 0, w=W, interval=(0, S - 1))
    assert maxdiff(roll.cpu(), full) > 1e-5                    # ... not the fully guided chain: it would miss the tolerance
