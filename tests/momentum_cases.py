"""The inputs of the "cfg_momentum" GPU tests (tests/test_gpu_cfg_momentum.py) and their CPU references - test
infrastructure.  Each reference is computed once per process and shared; it is never modified.

The inputs are those of tests/rescale_cases.py / project_cases.py: B = 2, T = 40, testlib.hp_of() (64 channels,
4 layers, k = 9, 200 steps), 20 visited steps, w = 3."""
import momentum_ref as MR
import project_cases as PC  # noqa: F401  (MC.PC: the partners' cases)
import stage_scenarios as SS
from project_cases import B, GUIDING, N_STEPS, OPTION_CASES, PHILOX_SEED, TN, W, mask_of, philox_z, setup, spec_of, start_step  # noqa: F401
from testlib import ATOL

# (cfg_momentum, cfg_project, cfg_norm): the paper's reverse momentum beside both partners, a forward one beside the projection alone
VALUES = ((-5000, 10000, 500), (5000, 10000, 0))
MAIN = VALUES[0]


def reference(sampler, momentum, project, norm, philox=False, **opts):
    """(final roll, {t: [(k, rho, s, a, b) per roll]}, {t: (rms |m|, rms |d|)}) of the restatement; momentum = 0: project_ref's chain."""
    return SS.reference(MR.sample_chain, sampler, {"cfg_momentum": momentum, "cfg_project": project, "cfg_norm": norm}, philox, **opts)


def assert_active(sampler, momentum, project, norm, philox=False, **opts):
    """The case has momentum.  The state: at every guided step after the one that starts it, rms |m| differs from rms |d| by at
    least a tenth (|beta| = 0.5 against updates that point alike from step to step gives about 1 -+ 0.4).  The roll: at least
    100 ATOL from the chain with "cfg_momentum" 0 under the same partners - except under the guidance interval, where the six
    unguided steps behind step 60 contract what the eight guided ones did and the bound r fixes the update's size whatever m
    is: there the roll's distance is printed and only has to exist.  Returns the reference roll."""
    roll, seen, rms = reference(sampler, momentum, project, norm, philox, **opts)
    off, _, _ = reference(sampler, 0, project, norm, philox, **opts)
    diff = float((roll - off).abs().max())
    steps = sorted(rms, reverse=True)
    ratio = [rms[t][0] / rms[t][1] for t in steps]
    print(f"\n{sampler} cfg_momentum {momentum} cfg_project {project} cfg_norm {norm} {sorted(opts.items())}: {len(seen)} guided steps; "
          f"rms |m| / rms |d| in {min(ratio[1:]):.3f} .. {max(ratio[1:]):.3f} behind the first; max |with - without momentum| {diff:.3e}")
    assert len(rms) == len(seen) > 1 and ratio[0] == 1.0
    assert all(abs(r - 1.0) >= 0.1 for r in ratio[1:]), ratio
    assert diff >= 100 * ATOL if "interval" not in opts else diff > 0.0, diff
    return roll
