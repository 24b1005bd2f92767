"""The inputs of the "cfg_project" / "cfg_norm" GPU tests (tests/test_gpu_cfg_project.py) and their CPU references - test
infrastructure.  Each reference is computed once per process and shared; it is never modified.

The inputs are those of tests/rescale_cases.py: B = 2, T = 40, testlib.hp_of() (64 channels, 4 layers, k = 9,
200 steps), 20 visited steps, w = 3; the inpainting sampler's time mask covers spectrogram frames [10, 20)."""
import project_ref as PR
import rescale_cases as RC
import stage_scenarios as SS
from rescale_cases import B, GUIDING, MASK, N_STEPS, PHILOX_SEED, TN, W, mask_of, philox_z, setup, spec_of, start_step  # noqa: F401
from testlib import ATOL

# (cfg_project, cfg_norm): rho = 0.5 and 1, alone and with r = 0.05; the last bound never binds
VALUES = ((5000, 0), (10000, 0), (5000, 500), (10000, 500), (10000, 100000))
MAIN = (10000, 500)

# rescale_cases.OPTION_CASES without the row that sets "x0_threshold" (refused beside these options); the restatement's
# keyword arguments beside project / norm / w, and the same on the facade
OPTION_CASES = [(name, kw, facade) for name, kw, facade in RC.OPTION_CASES if name != "clip-threshold"]


def reference(sampler, project, norm, philox=False, **opts):
    """(final roll, {t: [(k, rho, s, a, b) per roll]}) of the restatement; project = norm = 0: the options off."""
    return SS.reference(PR.sample_chain, sampler, {"cfg_project": project, "cfg_norm": norm}, philox, **opts)


def assert_active(sampler, project, norm, philox=False, **opts):
    """The case projects: rho k >= 0.2 at every guided step and roll of the restated chain, s <= 0.9 there where r = 0.05, and
    the roll is at least 100 ATOL (10 ATOL under the guidance interval, as in rescale_cases) from the chain with the options
    off.  Returns the reference roll."""
    roll, seen = reference(sampler, project, norm, philox, **opts)
    off, _ = reference(sampler, 0, 0, philox, **opts)
    rows = [row for step in seen.values() for row in step]
    rk = [float(rho * k) for k, rho, _, _, _ in rows]
    s = [float(row[2]) for row in rows]
    diff = float((roll - off).abs().max())
    print(f"\n{sampler} cfg_project {project} cfg_norm {norm} {sorted(opts.items())}: rho k in {min(rk):.3f} .. {max(rk):.3f}, "
          f"s in {min(s):.3f} .. {max(s):.3f} at {len(seen)} guided steps; max |projected - plain| {diff:.3e}")
    assert rows and all(v >= 0.2 for v in rk), (min(rk), max(rk))
    if norm == 500:
        assert all(v <= 0.9 for v in s), max(s)
    if norm == 100000:
        assert all(v == 1.0 for v in s)               # (the bound that never binds)
    assert diff >= (10 if "interval" in opts else 100) * ATOL, diff
    return roll
