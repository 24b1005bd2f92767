"""CPU restatement of the reverse chain under every option the engine accepts (include/diffroll_amd.h: "sampling_steps",
"guidance_t_min" / "guidance_t_max", "solver_order", "solver_noise", "start_step" / "start_noise", long-form windows) - test
infrastructure: the one chain the GPU parity tests are held to.

Composed from oracle.diffroll_ref.denoise (the network), oracle.philox (the engine's noise), the header's rule for the
visited steps and their coefficient rows (float64 from the committed fp32 scalars, one rounding to fp32) and the fp32
expression order of update_quad / solver_quad in diffroll_amd/csrc/update_quad.h.  The committed rows are the tables the
engine is handed (diffroll_amd.schedule.sampler_coef_tables, pinned to the reference by tests/test_oracle_golden.py); no
other product logic is read.  The solver is the exponential integrator in lambda = log(sqrt_acp / sqrt_1m_acp) on the x0
prediction: first order and DPM-Solver++ (2M), deterministic or in the stochastic form (SDE-DPM-Solver++), Lu et al. 2022.
In float64 there are the pure integrator for any denoiser and the exact covariance propagation of the stochastic chain on
a Gaussian prior (the integrator's own error, no network).
"""
from typing import Callable, List, Optional

import numpy as np
import torch

from oracle import diffroll_ref as R
from oracle import philox

# sampler -> (coefficient family, guided branch: None / "uncond" (spec = -1) / "zero" (spec = 0))
SAMPLERS = {
    "ddpm_x0": (0, None), "cfdg_ddpm_x0": (0, "uncond"), "generation_ddpm_x0": (0, None),
    "inpainting_ddpm_x0": (0, "uncond"), "ddim_x0": (1, None), "cfdg_ddim_x0": (1, "zero"),
    "ddpm": (2, None), "ddim": (3, None), "ddim2ddpm": (4, None),
}


# ---------------------------------------------------------------------------------------------- steps and scalars
def visited(S: int, n: int) -> List[int]:
    """t_i = (2 i (S - 1) + (n - 1)) // (2 (n - 1)), i = n-1 .. 0; n = 0 or S: every step."""
    if n in (0, S):
        return list(range(S - 1, -1, -1))
    return [(2 * i * (S - 1) + (n - 1)) // (2 * (n - 1)) for i in range(n - 1, -1, -1)]


def start_of(S: int, n: int, t_s: int) -> int:
    """The effective start step: t_s, or the chain's first visited step for -1."""
    return visited(S, n)[0] if t_s < 0 else t_s


def committed(hp) -> np.ndarray:
    """(5, S, 5) fp32: the coefficient tables the engine holds."""
    from diffroll_amd.schedule import make_schedule, sampler_coef_tables
    return sampler_coef_tables(make_schedule(hp["beta_start"], hp["beta_end"], int(hp["timesteps"]))).numpy()


def scalars(hp) -> np.ndarray:
    """(S, 2) float64 of the committed fp32 sqrt_acp / sqrt_1m_acp (family 0, columns 2 and 3)."""
    return committed(hp)[0, :, 2:4].astype(np.float64)


# ---------------------------------------------------------------------------------------------- rows
def derived_rows(A, Ap, Sm, Smp) -> np.ndarray:
    """(5, 5) fp32: the five families' rows for a step with sqrt_acp A / sqrt_1m_acp Sm and successor Ap / Smp."""
    A, Ap, Sm, Smp = (float(np.float32(v)) for v in (A, Ap, Sm, Smp))       # float64 of the fp32 scalars
    r2 = (A / Ap) * (A / Ap)
    sigma = (Smp / Sm) * np.sqrt(1.0 - r2)
    direction = np.sqrt(max(0.0, 1.0 - Ap * Ap - sigma * sigma))
    beta = 1.0 - r2
    rows = [[Ap, direction, A, Sm, sigma],
            [Ap, np.sqrt(1.0 - Ap * Ap), A, Sm, 0.0],
            [Ap / A, beta, Sm, np.sqrt(beta * Smp * Smp / (Sm * Sm)), 0.0],
            [Ap, Smp, A, Sm, 0.0],
            [Ap, direction, A, Sm, sigma]]
    return np.asarray(rows, dtype=np.float64).astype(np.float32)


def rows_for(tab: np.ndarray, steps: List[int]) -> dict:
    """t -> (5, 5) fp32 rows used at visited step t (committed when t == 0 or its successor is t - 1)."""
    out = {}
    for i, t in enumerate(steps):
        tp = steps[i + 1] if i + 1 < len(steps) else None
        if tp is None or tp == t - 1:
            out[t] = tab[:, t, :].copy()
        else:
            out[t] = derived_rows(tab[0, t, 2], tab[0, tp, 2], tab[0, t, 3], tab[0, tp, 3])
    return out


def solver_rows64(AS: np.ndarray, steps: List[int], order: int, noise: int = 0) -> dict:
    """t -> float64 solver row of visited step t; AS: (S, 2) float64 A / Sm per step.  With h the step in lambda and c the
    weight of the 2M history term (0 at the chain's first step, before step 0 and under order 1):
    noise = 0: [Smp / Sm, -Ap expm1(-h), A, c, 0];  1: [(Smp / Sm) exp(-h), Ap (-expm1(-2h)), A, c, Smp sqrt(-expm1(-2h))]."""
    lam = np.log(AS[:, 0] / AS[:, 1])
    out = {}
    for i, t in enumerate(steps):
        A, Sm = AS[t]
        if t == 0:
            out[t] = np.array([0.0, 0.0, A, 0.0, 0.0])
            continue
        tp = steps[i + 1]
        Ap, Smp = AS[tp]
        h = lam[tp] - lam[t]
        c = h / (2.0 * (lam[t] - lam[steps[i - 1]])) if order == 2 and i > 0 and tp != 0 else 0.0
        if noise:
            g = -np.expm1(-2.0 * h)
            out[t] = np.array([(Smp / Sm) * np.exp(-h), Ap * g, A, c, Smp * np.sqrt(g)])
        else:
            out[t] = np.array([Smp / Sm, -Ap * np.expm1(-h), A, c, 0.0])
    return out


def solver_rows(hp, n: int, order: int, noise: int = 0) -> dict:
    """t -> (5,) fp32 row of visited step t of the n-step chain: float64 from the committed fp32 scalars, rounded once."""
    steps = visited(int(hp["timesteps"]), n)
    return {t: r.astype(np.float32) for t, r in solver_rows64(scalars(hp), steps, order, noise).items()}


def chain_rows(hp, sampler: str, n: int, order: int = 0, solver_noise: int = 0, start: Optional[int] = None) -> dict:
    """t -> the (5,) fp32 row the chain reads at visited step t, in chain order from `start` (None: the first visited step)
    on: the sampler's family of rows_for, or under a solver order solver_rows - where the first row returned has c = 0,
    since a chain has no previous prediction at the step it starts at."""
    steps = visited(int(hp["timesteps"]), n)
    if order:
        rows = solver_rows(hp, n, order, solver_noise)
    else:
        rows = {t: r[SAMPLERS[sampler][0]] for t, r in rows_for(committed(hp), steps).items()}
    steps = steps if start is None else steps[steps.index(start):]
    rows = {t: rows[t] for t in steps}
    if order:
        rows[steps[0]] = rows[steps[0]].copy()
        rows[steps[0]][3] = 0.0
    return rows


# ---------------------------------------------------------------------------------------------- updates
def update(family: int, t: int, row: np.ndarray, x: torch.Tensor, y: torch.Tensor, z: Optional[torch.Tensor]) -> torch.Tensor:
    """update_quad.h's expressions, one fp32 rounding per operation (y: x0 prediction, families 0/1; epsilon, 2-4)."""
    c0, c1, c2, c3, c4 = (torch.tensor(float(v), dtype=torch.float32) for v in row)
    if z is None:
        z = torch.zeros_like(x)
    if family <= 1:
        if t == 0:
            return y / c2
        t1 = c0 * y
        t2 = (c1 * (x - c2 * y)) / c3
        return (t1 + t2) + c4 * z if family == 0 else t1 + t2
    if family == 2:
        m = c0 * (x - (c1 * y) / c2)
        return m if t == 0 else m + c3 * z
    xe = (x - c3 * y) / c2
    if t == 0:
        return xe
    return c0 * xe + c1 * y if family == 3 else (c0 * xe + c1 * y) + c4 * z


def solver_update(t: int, row: np.ndarray, x: torch.Tensor, y: torch.Tensor, p: Optional[torch.Tensor],
                  z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """solver_quad's expressions, one rounding per operation in the tensors' dtype: y the prediction, p the previous
    step's (read where the row's c is not 0), z the step's noise (read where the row's c4 is not 0)."""
    c0, c1, c2, c, c4 = (torch.tensor(float(v), dtype=x.dtype) for v in row)
    if t == 0:
        return y / c2
    d = y + c * (y - p) if float(c) != 0.0 else y
    o = c0 * x + c1 * d
    return o + c4 * z if float(c4) != 0.0 else o


# ---------------------------------------------------------------------------------------------- the loop
def prediction(params, hp, sampler, x, spec_c, t, w, table):
    """The network output an update consumes: guided as task/diffusion.py:953 / :1039-1041 where the sampler guides."""
    family, branch = SAMPLERS[sampler]
    tt = torch.tensor(t).repeat(x.shape[0])
    if sampler == "generation_ddpm_x0":
        spec_u = R.uncond_spec(params, hp, torch.empty(x.shape[0], int(hp["n_mels"]), x.shape[2]))
        return R.denoise(params, hp, x, spec_u, tt, table)
    y_c = R.denoise(params, hp, x, spec_c, tt, table)
    if branch is None:
        return y_c
    spec_2 = R.uncond_spec(params, hp, spec_c) if branch == "uncond" else torch.zeros_like(spec_c)
    return (1 + w) * y_c - w * R.denoise(params, hp, x, spec_2, tt, table)


def shared_mean(y: torch.Tensor, plan) -> torch.Tensor:
    """Long-form windows (n, 1, T, 88): frames two windows share take the mean of both predictions."""
    ym = y.clone()
    H, O, T = plan.stride, plan.overlap, plan.T
    for b in range(plan.n - 1):
        m = 0.5 * (y[b, :, H:T] + y[b + 1, :, 0:O])
        ym[b, :, H:T] = m
        ym[b + 1, :, 0:O] = m
    return ym


def sample_chain(params, hp, sampler: str, x: torch.Tensor, spec_c: Optional[torch.Tensor], noise, n: int, *, w: float = 0.0,
                 plan=None, trajectory: bool = False, interval=None, order: int = 0, solver_noise: int = 0,
                 start: Optional[int] = None, hook: Optional[Callable] = None):
    """THE chain loop of the tests: predict -> shared-frame mean -> update, over the rows of chain_rows - the n visited steps
    (0: all) from `start` on (None: all of them).  x (B, 1, T, 88) is x at the step the chain starts at, spec_c
    (B, n_mels, T) (conditional samplers), noise (S, B, 1, T, 88) or a dict t -> (B, 1, T, 88): noise[t] is the z of visited
    step t > 0 (None where no step draws: families 1 / 3, a solver order without solver_noise).
    plan: long-form windows (B = plan.n), the shared-frame mean before each update (and in the solver's history).
    interval = (lo, hi): a guidance interval - the weight is w at lo <= t <= hi and 0 elsewhere, as the reference's sampler
    with hparams.sampling.w set per step; BOTH network branches are evaluated at every step and combined as
    (1 + w_t) c - w_t u, so this is the reference's arithmetic, not the engine's shortcut.
    order = 1 / 2: option "solver_order" - solver_rows and solver_update on the x0 prediction, the previous step's
    prediction carried along, noise drawn only under solver_noise = 1; 0: the sampler's own rows and update.
    hook(t, y) -> y: what an option does to the prediction behind the shared-frame mean (clip_ref, thresh_ref); the update
    and the solver's history see what it returns.
    Returns the final roll, or the roll after every step run (steps, B, 1, T, 88) with trajectory=True."""
    S = int(hp["timesteps"])
    family = SAMPLERS[sampler][0]
    draws = solver_noise if order else family in (0, 2, 4)
    lo, hi = (0, S - 1) if interval is None else interval
    table = R.build_embedding(S)
    prev, traj = None, []
    with torch.no_grad():
        for t, row in chain_rows(hp, sampler, n, order, solver_noise, start).items():      # (insertion order: chain order)
            y = prediction(params, hp, sampler, x, spec_c, t, w if lo <= t <= hi else 0.0, table)
            if plan is not None:
                y = shared_mean(y, plan)
            if hook is not None:
                y = hook(t, y)
            z = noise[t] if draws and t > 0 else None
            x = solver_update(t, row, x, y, prev, z) if order else update(family, t, row, x, y, z)
            prev = y
            traj.append(x)
    return torch.stack(traj, 0) if trajectory else x


def diffuse(hp, x0: torch.Tensor, t_s: int, z: torch.Tensor) -> torch.Tensor:
    """dr_q_sample's fp32 expression (A * x0) + (Sm * z), each product rounded once, then the sum: A / Sm the committed
    scalars of step t_s."""
    tab = committed(hp)
    A, Sm = (torch.tensor(float(tab[0, t_s, c]), dtype=torch.float32) for c in (2, 3))
    return (A * x0.to(torch.float32)) + (Sm * z.to(torch.float32))


def refine_chain(params, hp, sampler: str, x0: torch.Tensor, spec_c, noise, n: int, t_s: int, z: torch.Tensor, **kw):
    """Option "start_noise": the clean roll x0 diffused to the start step (t_s, -1: the first visited) with z, then the chain
    started there."""
    t0 = start_of(int(hp["timesteps"]), n, t_s)
    return sample_chain(params, hp, sampler, diffuse(hp, x0, t0, z), spec_c, noise, n, start=t0, **kw)


# ---------------------------------------------------------------------------------------------- the engine's noise
def philox_noise(seed: int, first_sample: int, S: int, B: int, T: int) -> torch.Tensor:
    """The injected-noise tensor (S, B, 1, T, 88) equal to the engine's Philox draws (keyed by the real step)."""
    return philox.chain_noise(seed, first_sample, S, B, T)


def philox_rows(seed: int, keys: List[int], S: int, n: int, T: int) -> dict:
    """t -> (len(keys), 1, T, 88): the engine's Philox z of every visited step t > 0 of the n-step chain for the clips with
    sample keys `keys` (first_sample + row; under "draws" / sharding whatever key the row has) - oracle.philox replayed."""
    return {t: torch.from_numpy(np.concatenate([philox.step_noise(seed, k, 1, T * 88, t) for k in keys], 0)).reshape(len(keys), 1, T, 88)
            for t in visited(S, n) if t > 0}


def diffusion_noise(seed: int, first_sample: int, S: int, B: int, T: int, t_s: int) -> torch.Tensor:
    """(B, 1, T, 88): the engine's Philox z of the diffusion to t_s (step word timesteps + t_s) for rows first_sample ..
    first_sample + B - 1."""
    return torch.from_numpy(philox.step_noise(seed, first_sample, B, T * 88, S + t_s).reshape(B, 1, T, 88).copy())


def window_noise(seed: int, recording: int, S: int, plan, t_s: int) -> torch.Tensor:
    """(n, 1, T, 88): one canvas draw of the recording (keyed by the canvas element), gathered into its windows."""
    from diffroll_amd import longform
    canvas = torch.from_numpy(philox.step_noise(seed, recording, 1, plan.T_c * 88, S + t_s).reshape(plan.T_c, 88).copy())
    return longform.gather_windows(canvas, plan).unsqueeze(1)


# ---------------------------------------------------------------------------------------------- float64 analysis
def integrate64(denoise: Callable, AS: np.ndarray, steps: List[int], order: int, x_T: np.ndarray, final: bool = True):
    """The pure integrator in float64: denoise(x, t) -> x0 prediction; AS (S, 2) float64 A / Sm.  final=False returns the
    state BEFORE the last step's y / A_0 (the state at t = 0)."""
    rw = solver_rows64(AS, steps, order)
    x, p = np.asarray(x_T, dtype=np.float64), None
    for t in steps:
        if t == 0:
            return denoise(x, t) / rw[t][2] if final else x
        y = denoise(x, t)
        c0, c1, _, c, _ = rw[t]
        d = y + c * (y - p) if c != 0.0 else y
        x = c0 * x + c1 * d
        p = y
    return x


def variance_error(AS: np.ndarray, steps: List[int], order: int, s2: float) -> float:
    """Relative error of the final variance of the stochastic chain on the prior N(0, s2), in float64 and in closed form.
    The denoiser of that prior is linear - E[x0 | x_t] = k_t x, k_t = A s2 / (A^2 s2 + Sm^2) - so the covariance of the
    state (x, previous prediction) propagates exactly: with M = [[c0 + c1 (1 + c) k, -c1 c], [k, 0]],
    Cov' = M Cov M^T + diag(c4^2, 0).  x at the first visited step has its exact marginal variance A^2 s2 + Sm^2; the
    last step is x0 = k_0 x / A_0.  Returns |Var(x0) / s2 - 1|."""
    rw = solver_rows64(AS, steps, order, 1)
    k = AS[:, 0] * s2 / (AS[:, 0] ** 2 * s2 + AS[:, 1] ** 2)
    A, Sm = AS[steps[0]]
    cov = np.array([[A * A * s2 + Sm * Sm, 0.0], [0.0, 0.0]])
    for t in steps:
        c0, c1, c2, c, c4 = rw[t]
        if t == 0:
            return abs((k[t] / c2) ** 2 * cov[0, 0] / s2 - 1.0)
        M = np.array([[c0 + c1 * (1.0 + c) * k[t], -c1 * c], [k[t], 0.0]])
        cov = M @ cov @ M.T + np.diag([c4 * c4, 0.0])
    raise AssertionError("the chain does not end at step 0")
