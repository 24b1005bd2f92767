"""CPU restatement of a chain under a guidance interval (options "guidance_t_min" / "guidance_t_max" of
include/diffroll_amd.h) - test infrastructure: tests/respaced_ref.py's chain loop with interval= (the weight is w where
lo <= t <= hi and 0 elsewhere; both network branches evaluated at every step)."""
import respaced_ref as RR


def sample_chain(params, hp, sampler, x_T, spec_c, noise, n, w, interval, plan=None, trajectory=False):
    """respaced_ref.sample_chain's arguments + interval = (lo, hi) in real diffusion steps (hi inclusive)."""
    return RR.sample_chain(params, hp, sampler, x_T, spec_c, noise, n, w, plan, trajectory, interval=interval)
