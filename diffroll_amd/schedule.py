"""Host-side constant tables of the sampler (tiny, built once per model).

The reference keeps these as plain CPU tensors computed in its constructor
(task/diffusion.py:239-256) and evaluates the per-step scalars inline at every step
(:957-967).  They are evaluated here with the same torch fp32 expressions so the
coefficients the update kernel reads are bit-equal to the reference's, then handed to the
engine through dr_set_tables().
"""
from __future__ import annotations

import math
from typing import Dict, List

import torch
import torch.nn.functional as F


def linear_beta_schedule(beta_start: float, beta_end: float, timesteps: int) -> torch.Tensor:
    """task/diffusion.py:28-29."""
    return torch.linspace(beta_start, beta_end, timesteps)


_BETA_LO, _BETA_HI = 0.0001, 0.02     # the fixed end points of the quadratic / sigmoid schedules


def cosine_beta_schedule(timesteps, s=0.008):
    """Nichol & Dhariwal's cosine schedule (arXiv:2102.09672) as model/unet.py:558-567 evaluates it: the
    normalised squared-cosine curve f on timesteps + 1 grid points, beta_t = 1 - f[t+1] / f[t], clipped."""
    grid = torch.linspace(0, timesteps, timesteps + 1)
    f = torch.cos(((grid / timesteps) + s) / (1 + s) * torch.pi * 0.5) ** 2
    f = f / f[0]
    return torch.clip(1 - (f[1:] / f[:-1]), 0.0001, 0.9999)


def quadratic_beta_schedule(timesteps):
    """model/unet.py:570-573: linear in sqrt(beta)."""
    return torch.linspace(_BETA_LO**0.5, _BETA_HI**0.5, timesteps) ** 2


def sigmoid_beta_schedule(timesteps):
    """model/unet.py:575-579: a sigmoid ramp over [-6, 6] between the two end points."""
    ramp = torch.sigmoid(torch.linspace(-6, 6, timesteps))
    return ramp * (_BETA_HI - _BETA_LO) + _BETA_LO


def make_schedule(beta_start: float, beta_end: float, timesteps: int, betas: torch.Tensor = None) -> Dict[str, torch.Tensor]:
    """The six schedule vectors of SpecRollDiffusion.__init__ (task/diffusion.py:239-256).  `betas` replaces the
    linear schedule (e.g. one of the model/unet.py schedules above): everything downstream - the coefficient
    tables the engine reads - only sees these vectors."""
    betas = linear_beta_schedule(beta_start, beta_end, timesteps) if betas is None else betas.to(torch.float32)
    alphas = 1. - betas
    alphas_cumprod = torch.cumprod(alphas, axis=0)
    alphas_cumprod_prev = F.pad(alphas_cumprod[:-1], (1, 0), value=1.0)
    return {
        "betas": betas,
        "alphas": alphas,
        "sqrt_recip_alphas": torch.sqrt(1.0 / alphas),
        "sqrt_alphas_cumprod": torch.sqrt(alphas_cumprod),
        "sqrt_one_minus_alphas_cumprod": torch.sqrt(1. - alphas_cumprod),
        "posterior_variance": betas * (1. - alphas_cumprod_prev) / (1 - alphas_cumprod),
    }


def posterior_coef_table(sch: Dict[str, torch.Tensor]) -> torch.Tensor:
    """(S, 5) fp32: [sqrt_acp[t-1], sqrt(1 - sqrt_acp[t-1]**2 - sigma**2), sqrt_acp[t],
    sqrt_1m_acp[t], sigma] - the scalars of the x0-prediction DDPM update,
    task/diffusion.py:957-967 (identical in ddpm_x0 / cfdg / generation / inpainting).
    Row 0 only uses column 2 (x = x0 / sqrt_acp[0]; no noise)."""
    sac = sch["sqrt_alphas_cumprod"]
    s1m = sch["sqrt_one_minus_alphas_cumprod"]
    alphas = sch["alphas"]
    S = sac.shape[0]
    out = torch.zeros(S, 5, dtype=torch.float32)
    for t in range(S):
        if t == 0:
            sigma = (1 / s1m[t]) * torch.sqrt(1 - alphas[t])
            out[t, 2] = sac[t]
            out[t, 3] = s1m[t]
            out[t, 4] = sigma
        else:
            sigma = (s1m[t - 1] / s1m[t]) * torch.sqrt(1 - alphas[t])
            out[t, 0] = sac[t - 1]
            out[t, 1] = torch.sqrt(1 - sac[t - 1] ** 2 - sigma ** 2)
            out[t, 2] = sac[t]
            out[t, 3] = s1m[t]
            out[t, 4] = sigma
    return out


def build_embedding(max_steps: int) -> torch.Tensor:
    """Sinusoidal step table (S, 128) of DiffusionEmbedding (model/diffwave.py:83-88)."""
    steps = torch.arange(max_steps).unsqueeze(1)
    dims = torch.arange(64).unsqueeze(0)
    table = steps * 10.0 ** (dims * 4.0 / 63.0)
    return torch.cat([torch.sin(table), torch.cos(table)], dim=1)


def check_sampling_steps(n, timesteps: int) -> int:
    """Option "sampling_steps" (include/diffroll_amd.h): None / 0 = every step, else 2 <= n <= timesteps.  Returns n
    (0 for None); anything else raises ValueError."""
    if n is None:
        return 0
    if isinstance(n, bool) or not isinstance(n, int) or (n != 0 and not 2 <= n <= int(timesteps)):
        raise ValueError(f"sampling steps must be 0 / None (every step) or an integer in [2, timesteps = {timesteps}], "
                         f"got {n!r}")
    return n


X0_SAMPLERS = ("ddpm_x0", "cfdg_ddpm_x0", "generation_ddpm_x0", "inpainting_ddpm_x0", "ddim_x0", "cfdg_ddim_x0")


def check_solver_order(order, sampler: str = None) -> int:
    """Option "solver_order" (include/diffroll_amd.h) as hparams.sampling.solver_order: None / 0 = the sampler's own update,
    1 = the first-order exponential integrator in lambda, 2 = DPM-Solver++ (2M).  Returns the option's value; any other
    value, or a non-zero order with a sampler that predicts epsilon, raises ValueError."""
    if order is None:
        return 0
    if isinstance(order, bool) or not isinstance(order, int) or order not in (0, 1, 2):
        raise ValueError(f"solver_order must be 0 / None (the sampler's own update), 1 or 2 (DPM-Solver++ 2M), got {order!r}")
    if order and sampler is not None and sampler not in X0_SAMPLERS:
        raise ValueError(f"solver_order = {order} integrates an x0 prediction ({', '.join(X0_SAMPLERS)}); '{sampler}' "
                         f"predicts epsilon")
    return order


def check_solver_noise(value, sampler: str = None, order=None) -> int:
    """Option "solver_noise" (include/diffroll_amd.h) as hparams.sampling.solver_noise: None / 0 / False = the deterministic
    solver, 1 / True = its stochastic form (SDE-DPM-Solver++), which draws the z's of the ddpm_x0 chain.  `order` is the
    configured solver_order.  Returns the option's value; any other value, or a set value while solver_order is absent / 0
    or with a sampler that predicts epsilon, raises ValueError."""
    if value is None:
        return 0
    if not isinstance(value, (bool, int)) or value not in (0, 1):
        raise ValueError(f"solver_noise must be 0 / None (the deterministic solver) or 1 (its stochastic form), got {value!r}")
    value = int(value)
    if value and sampler is not None and sampler not in X0_SAMPLERS:
        raise ValueError(f"solver_noise = 1 is the stochastic form of solver_order = 1 / 2, which integrates an x0 prediction "
                         f"({', '.join(X0_SAMPLERS)}); '{sampler}' predicts epsilon")
    if value and not check_solver_order(order):
        raise ValueError(f"solver_noise = 1 is the stochastic form of solver_order = 1 / 2, but solver_order is {order!r} (the "
                         f"sampler's own update): set solver_order too")
    return value


X0_CLIP_RANGES = {(0.0, 1.0): 1, (-1.0, 1.0): 2}      # the range the rolls were normalised to -> the option's code


def check_x0_clip(value, sampler: str = None, norm_args=(0, 1)) -> int:
    """Option "x0_clip" (include/diffroll_amd.h) as hparams.sampling.x0_clip: None / 0 / False = off, 1 / True = clamp the
    x0 prediction every update consumes to the range the rolls were normalised to, norm_args[0] .. norm_args[1].  Returns
    the option's value - 1 for the range (0, 1), 2 for (-1, 1), 0 for off; any other value, a range the engine has no code
    for, or a set value with a sampler that predicts epsilon (it has no x0 prediction to clamp) raises ValueError."""
    if value is None:
        return 0
    if not isinstance(value, (bool, int)) or value not in (0, 1):
        raise ValueError(f"x0_clip must be 0 / None (off) or 1 (clamp the x0 prediction to the roll's range), got {value!r}")
    if not value:
        return 0
    if sampler is not None and sampler not in X0_SAMPLERS:
        raise ValueError(f"x0_clip = 1 clamps an x0 prediction ({', '.join(X0_SAMPLERS)}); '{sampler}' predicts epsilon")
    try:
        rng = (float(norm_args[0]), float(norm_args[1])) if isinstance(norm_args, (list, tuple)) else None
    except (TypeError, ValueError, IndexError):
        rng = None
    if rng not in X0_CLIP_RANGES:
        shown = list(norm_args[:2]) if isinstance(norm_args, (list, tuple)) else norm_args
        raise ValueError(f"x0_clip = 1 clamps to the roll's range norm_args[0] .. norm_args[1], which must be 0 .. 1 or -1 .. 1, "
                         f"got {shown!r}")
    return X0_CLIP_RANGES[rng]


def check_x0_threshold(value, sampler: str = None, x0_clip=None) -> int:
    """Option "x0_threshold" (include/diffroll_amd.h) as hparams.sampling.x0_threshold: None / 0 / False = off, a float p
    with 0.5 <= p <= 1 = dynamic thresholding at that quantile of |y - m| over each roll (0.995 is Imagen's 99.5 %).  Returns
    the option's value round(p * 10000) - 5000 .. 10000, or 0 for off; x0_clip is hparams.sampling.x0_clip, which the
    threshold refines: a set value without it, any other value, or a sampler that predicts epsilon raises ValueError."""
    if value is None or value is False or (not isinstance(value, bool) and isinstance(value, (int, float)) and value == 0):
        return 0
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.5 <= value <= 1.0:
        raise ValueError(f"x0_threshold must be 0 / None (off) or a quantile p with 0.5 <= p <= 1 (0.995 = the 99.5th percentile), "
                         f"got {value!r}")
    if sampler is not None and sampler not in X0_SAMPLERS:
        raise ValueError(f"x0_threshold = {value!r} and x0_clip act on an x0 prediction ({', '.join(X0_SAMPLERS)}); '{sampler}' "
                         f"predicts epsilon")
    if not x0_clip:
        raise ValueError(f"x0_threshold = {value!r} needs x0_clip = 1: the threshold is compared with the roll's range, which x0_clip "
                         f"names, got x0_clip = {x0_clip!r}")
    return int(round(float(value) * 10000))


def check_start(start_step, strength, visited) -> int:
    """Options "start_step" / "start_noise" (include/diffroll_amd.h) as hparams.sampling.start_step / .strength: where a
    chain over the steps `visited` (chain order) begins.  The two keys are mutually exclusive.  strength s in (0, 1] runs
    k = min(n, max(1, floor(s n + 0.5))) of the n visited steps - the start is visited[n - k]; start_step names the visited
    step itself.  Returns the option's value: the step, or -1 for neither key and for k = n (the whole chain).  Anything
    else raises ValueError."""
    visited = [int(t) for t in visited]
    n = len(visited)
    if start_step is not None and strength is not None:
        raise ValueError(f"start_step and strength are mutually exclusive (got start_step = {start_step!r}, strength = {strength!r})")
    if strength is not None:
        if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 < float(strength) <= 1.0:
            raise ValueError(f"strength must be a number in (0, 1] (or None: the whole chain), got {strength!r}")
        k = min(n, max(1, int(math.floor(float(strength) * n + 0.5))))
        return -1 if k == n else visited[n - k]
    if start_step is None:
        return -1
    if isinstance(start_step, bool) or not isinstance(start_step, int) or start_step not in visited:
        near = ""
        if isinstance(start_step, int) and not isinstance(start_step, bool) and visited[-1] < start_step < visited[0]:
            near = (f": the visited steps on either side of it are {min(t for t in visited if t > start_step)} and "
                    f"{max(t for t in visited if t < start_step)}")
        raise ValueError(f"start_step must be one of the {n} steps the chain visits ({visited[0]} .. {visited[-1]}; or None: "
                         f"the whole chain), got {start_step!r}{near}")
    return start_step


GUIDING_SAMPLERS = ("cfdg_ddpm_x0", "inpainting_ddpm_x0", "cfdg_ddim_x0")


def check_guidance_interval(interval, timesteps: int, sampler: str = None):
    """Options "guidance_t_min" / "guidance_t_max" (include/diffroll_amd.h) as hparams.sampling.guidance_interval = [lo, hi]:
    the steps lo <= t <= hi of a guiding sampler run both evaluations, the others the conditional one alone.  None = the
    whole chain.  Returns the options' values (lo, hi), (0, -1) for None; a malformed interval - not two integers,
    outside [0, timesteps), lo > hi - or a sampler that does not guide raises ValueError."""
    if interval is None:
        return 0, -1
    S = int(timesteps)
    ok = isinstance(interval, (list, tuple)) and len(interval) == 2 and all(
        isinstance(v, int) and not isinstance(v, bool) for v in interval)
    if not ok or not 0 <= interval[0] <= interval[1] < S:
        raise ValueError(f"guidance_interval must be [lo, hi] with integers 0 <= lo <= hi < timesteps = {S} (or None: the "
                         f"whole chain), got {interval!r}")
    if sampler is not None and sampler not in GUIDING_SAMPLERS:
        raise ValueError(f"guidance_interval needs a sampler that guides ({', '.join(GUIDING_SAMPLERS)}), not '{sampler}'")
    return int(interval[0]), int(interval[1])


def check_cfg_rescale(value, sampler: str = None) -> int:
    """Option "cfg_rescale" (include/diffroll_amd.h) as hparams.sampling.cfg_rescale: None / 0 / False = off, a float phi with
    0 < phi <= 1 = the guidance rescale of Lin et al. 2024 at the steps that guide (0.7 is the paper's value).  Returns the
    option's value round(phi * 10000) - 1 .. 10000, or 0 for off; any other value (a phi that rounds to 0 included) or a set
    value with a sampler that does not guide raises ValueError."""
    if value is None or value is False or (not isinstance(value, bool) and isinstance(value, (int, float)) and value == 0):
        return 0
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 < value <= 1.0 or int(round(float(value) * 10000)) < 1:
        raise ValueError(f"cfg_rescale must be 0 / None (off) or a factor phi with 0 < phi <= 1 in steps of 1 / 10000 (0.7 = the "
                         f"paper's value), got {value!r}")
    if sampler is not None and sampler not in GUIDING_SAMPLERS:
        raise ValueError(f"cfg_rescale = {value!r} needs a sampler that guides ({', '.join(GUIDING_SAMPLERS)}), not '{sampler}'")
    return int(round(float(value) * 10000))


def _check_projected(name: str, what: str, value, hi: float, sampler, x0_threshold, cfg_rescale) -> int:
    if value is None or value is False or (not isinstance(value, bool) and isinstance(value, (int, float)) and value == 0):
        return 0
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 < value <= hi or int(round(float(value) * 10000)) < 1:
        raise ValueError(f"{name} must be 0 / None (off) or {what} in (0, {hi:g}] in steps of 1 / 10000, got {value!r}")
    if sampler is not None and sampler not in GUIDING_SAMPLERS:
        raise ValueError(f"{name} = {value!r} needs a sampler that guides ({', '.join(GUIDING_SAMPLERS)}), not '{sampler}'")
    for other, theirs in (("x0_threshold", x0_threshold), ("cfg_rescale", cfg_rescale)):
        if theirs is not None and theirs is not False and theirs != 0:
            raise ValueError(f"{name} = {value!r} does not combine with {other} = {theirs!r}: set one of them None")
    return int(round(float(value) * 10000))


def check_cfg_project(value, sampler: str = None, x0_threshold=None, cfg_rescale=None) -> int:
    """Option "cfg_project" (include/diffroll_amd.h) as hparams.sampling.cfg_project: None / 0 / False = off, a float rho with
    0 < rho <= 1 = the share of the guidance update's component parallel to the conditional prediction that a guided step
    removes (adaptive projected guidance, Sadat et al. 2024; 1.0 is the paper's eta = 0).  Returns the option's value
    round(rho * 10000) - 1 .. 10000, or 0 for off; any other value, a set value with a sampler that does not guide, or one
    beside a set x0_threshold or cfg_rescale raises ValueError."""
    return _check_projected("cfg_project", "a share rho", value, 1.0, sampler, x0_threshold, cfg_rescale)


def check_cfg_norm(value, sampler: str = None, x0_threshold=None, cfg_rescale=None) -> int:
    """Option "cfg_norm" (include/diffroll_amd.h) as hparams.sampling.cfg_norm: None / 0 / False = off, a float r with
    0 < r <= 10 = the bound on the per-element rms of the guidance update c - u over the roll at a guided step.  Returns the
    option's value round(r * 10000) - 1 .. 100000, or 0 for off; refusals as check_cfg_project's."""
    return _check_projected("cfg_norm", "an rms bound r", value, 10.0, sampler, x0_threshold, cfg_rescale)


def check_cfg_momentum(value, sampler: str = None, cfg_project=None, cfg_norm=None) -> int:
    """Option "cfg_momentum" (include/diffroll_amd.h) as hparams.sampling.cfg_momentum: None / 0 / False = off, a float beta with
    0 < |beta| < 1 = the momentum of adaptive projected guidance (Sadat et al. 2024; the paper's values are -0.5 .. -0.75): a
    guided step's update becomes d + beta m_prev.  Returns the option's value round(beta * 10000) - -9999 .. 9999, or 0 for
    off; any other value (a beta that rounds to 0 or to +-1 included), a set value with a sampler that does not guide, or one
    beside neither cfg_project nor cfg_norm raises ValueError.  (Beside x0_threshold or cfg_rescale those two are refused.)"""
    if value is None or value is False or (not isinstance(value, bool) and isinstance(value, (int, float)) and value == 0):
        return 0
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 < abs(value) < 1.0 or \
            not 1 <= abs(int(round(float(value) * 10000))) <= 9999:
        raise ValueError(f"cfg_momentum must be 0 / None (off) or a momentum beta with 0 < |beta| < 1 in steps of 1 / 10000 (-0.5 = the "
                         f"paper's value), got {value!r}")
    if sampler is not None and sampler not in GUIDING_SAMPLERS:
        raise ValueError(f"cfg_momentum = {value!r} needs a sampler that guides ({', '.join(GUIDING_SAMPLERS)}), not '{sampler}'")
    if all(v is None or v is False or v == 0 for v in (cfg_project, cfg_norm)):
        raise ValueError(f"cfg_momentum = {value!r} needs cfg_project or cfg_norm: it acts on the update those two shape, and "
                         f"cfg_project = {cfg_project!r} and cfg_norm = {cfg_norm!r} are both off")
    return int(round(float(value) * 10000))


STRIDE_PARTNERS = ("x0_threshold", "cfg_rescale", "cfg_project", "cfg_norm", "cfg_momentum")


def check_guidance_stride(value, sampler: str = None, **partners) -> int:
    """Option "guidance_stride" (include/diffroll_amd.h) as hparams.sampling.guidance_stride: None / 0 / 1 = off, an integer n
    in 2 .. 64 = of the steps that guide, every n-th one (and step 0) runs both evaluations and the others reuse its guidance
    update beside the conditional evaluation alone.  partners: hparams.sampling's x0_threshold, cfg_rescale, cfg_project,
    cfg_norm, cfg_momentum.  Returns the option's value, n or 0 for off; any other value, a set value with a sampler that does
    not guide, or one beside a set partner (their statistics need the unconditional prediction) raises ValueError."""
    if value is None or (not isinstance(value, bool) and isinstance(value, int) and value in (0, 1)):
        return 0
    if isinstance(value, bool) or not isinstance(value, int) or not 2 <= value <= 64:
        raise ValueError(f"guidance_stride must be 0 / 1 / None (off) or an integer stride n with 2 <= n <= 64 (2 = every second "
                         f"guided step runs both evaluations), got {value!r}")
    if sampler is not None and sampler not in GUIDING_SAMPLERS:
        raise ValueError(f"guidance_stride = {value!r} needs a sampler that guides ({', '.join(GUIDING_SAMPLERS)}), not '{sampler}'")
    for other in STRIDE_PARTNERS:
        theirs = partners.get(other)
        if theirs is not None and theirs is not False and theirs != 0:
            raise ValueError(f"guidance_stride = {value!r} does not combine with {other} = {theirs!r}: its statistics need the "
                             f"unconditional prediction, which a step that reuses the guidance update does not evaluate; set one "
                             f"of them None")
    return int(value)


def check_exact_below(value, timesteps: int) -> int:
    """Option "exact_below" (include/diffroll_amd.h) as hparams.sampling.exact_below: None / 0 = off, an integer v with
    0 <= v <= timesteps = the reverse steps at diffusion step t < v run in exact fp32 whatever precision the model selected
    (v = timesteps: every step).  Keyed by the real step, so it means the same under `steps`; inert under precision 'f32'.
    Returns the option's value, v or 0 for off; anything else raises ValueError."""
    if value is None:
        return 0
    S = int(timesteps)
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= S:
        raise ValueError(f"exact_below must be 0 / None (off) or an integer v with 0 <= v <= timesteps = {S} (the steps t < v run "
                         f"in exact fp32), got {value!r}")
    return int(value)


def respaced_steps(timesteps: int, n: int) -> List[int]:
    """The steps a chain of n network evaluations visits, in chain order: t_i = round-half-up(i (S - 1) / (n - 1)) in
    integer arithmetic for i = n-1 .. 0 - strictly decreasing from S - 1 to 0.  n = 0 or n = S: every step."""
    S = int(timesteps)
    n = check_sampling_steps(n, S)
    if n in (0, S):
        return list(range(S - 1, -1, -1))
    return [(2 * i * (S - 1) + (n - 1)) // (2 * (n - 1)) for i in range(n - 1, -1, -1)]


def sampling_options(sampling, timesteps, norm_args=(0, 1)) -> Dict[str, object]:
    """hparams.sampling (the CLI's task.sampling) read once: every key above through its validator, in this order, and the
    values the engine's options take, by option name - "guidance_interval" is the pair of "guidance_t_min" / "guidance_t_max",
    "start_step" comes from the keys start_step / strength.  A refusal is the validator's own ValueError, with the key it
    belongs to as its attribute `key`."""
    from .ensemble import check_draws
    get, sampler = sampling.get, sampling.get("type")
    started = get("start_step") is not None or get("strength") is not None      # (the visited steps are only needed then)
    checks = (
        ("sampling_steps", "steps", lambda: check_sampling_steps(get("steps"), timesteps)),
        ("draws", "draws", lambda: check_draws(get("draws"))),
        ("guidance_interval", "guidance_interval", lambda: check_guidance_interval(get("guidance_interval"), timesteps, sampler)),
        ("solver_order", "solver_order", lambda: check_solver_order(get("solver_order"), sampler)),
        ("solver_noise", "solver_noise", lambda: check_solver_noise(get("solver_noise"), sampler, get("solver_order"))),
        ("start_step", "start_step" if get("strength") is None else "strength",
         lambda: check_start(get("start_step"), get("strength"), respaced_steps(timesteps, get("steps") or 0) if started else ())),
        ("x0_clip", "x0_clip", lambda: check_x0_clip(get("x0_clip"), sampler, norm_args)),
        ("x0_threshold", "x0_threshold", lambda: check_x0_threshold(get("x0_threshold"), sampler, get("x0_clip"))),
        ("cfg_rescale", "cfg_rescale", lambda: check_cfg_rescale(get("cfg_rescale"), sampler)),
        ("cfg_project", "cfg_project", lambda: check_cfg_project(get("cfg_project"), sampler, get("x0_threshold"), get("cfg_rescale"))),
        ("cfg_norm", "cfg_norm", lambda: check_cfg_norm(get("cfg_norm"), sampler, get("x0_threshold"), get("cfg_rescale"))),
        ("cfg_momentum", "cfg_momentum", lambda: check_cfg_momentum(get("cfg_momentum"), sampler, get("cfg_project"), get("cfg_norm"))),
        ("guidance_stride", "guidance_stride",
         lambda: check_guidance_stride(get("guidance_stride"), sampler, **{k: get(k) for k in STRIDE_PARTNERS})),
        ("exact_below", "exact_below", lambda: check_exact_below(get("exact_below"), timesteps)),
    )
    options = {}
    for option, key, check in checks:
        try:
            options[option] = check()
        except ValueError as err:
            err.key = key
            raise
    return options


def sampler_coef_tables(sch: Dict[str, torch.Tensor]) -> torch.Tensor:
    """(5, S, 5) fp32: one table of per-step scalars per coefficient family (DR_COEF_* in
    include/diffroll_amd.h), each scalar evaluated with the reference's own torch expression:
      0 ddpm_x0 family   task/diffusion.py:957-967   (posterior_coef_table)
      1 ddim_x0 family   :864-873, :1044-1053        (sigma = 0)
      2 ddpm  (epsilon)  :807-829    [sqrt_recip_alphas[t], betas[t], sqrt_1m_acp[t], sqrt(posterior_variance[t]), 0]
      3 ddim  (epsilon)  :885-890    [sqrt_acp[t-1], sqrt_1m_acp[t-1], sqrt_acp[t], sqrt_1m_acp[t], 0]
      4 ddim2ddpm (eps)  :902-909    [sqrt_acp[t-1], sqrt(1 - sqrt_acp[t-1]**2 - sigma**2), sqrt_acp[t], sqrt_1m_acp[t], sigma]
    """
    sac = sch["sqrt_alphas_cumprod"]
    s1m = sch["sqrt_one_minus_alphas_cumprod"]
    alphas = sch["alphas"]
    S = sac.shape[0]
    out = torch.zeros(5, S, 5, dtype=torch.float32)
    out[0] = posterior_coef_table(sch)
    for t in range(S):
        out[1, t, 2] = sac[t]
        out[1, t, 3] = s1m[t]
        out[2, t, 0] = sch["sqrt_recip_alphas"][t]
        out[2, t, 1] = sch["betas"][t]
        out[2, t, 2] = s1m[t]
        out[2, t, 3] = torch.sqrt(sch["posterior_variance"][t])
        for fam in (3, 4):
            out[fam, t, 2] = sac[t]
            out[fam, t, 3] = s1m[t]
        if t > 0:
            sigma = 0
            out[1, t, 0] = sac[t - 1]
            out[1, t, 1] = torch.sqrt(1 - sac[t - 1] ** 2 - sigma ** 2)
            out[3, t, 0] = sac[t - 1]
            out[3, t, 1] = s1m[t - 1]
            sigma = (s1m[t - 1] / s1m[t]) * torch.sqrt(1 - alphas[t])
            out[4, t, 0] = sac[t - 1]
            out[4, t, 1] = torch.sqrt(1 - sac[t - 1] ** 2 - sigma ** 2)
            out[4, t, 4] = sigma
    return out
