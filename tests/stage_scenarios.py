"""What the GPU suites of the guidance stages share (tests/test_gpu_cfg_rescale.py, test_gpu_cfg_project.py,
test_gpu_cfg_momentum.py and their case modules): the inputs, the model builder, the cached restatement and, once each, the
scenarios every stage option is held to - test infrastructure, not collected.

A stage is plain data: `values`, its options by engine option name in units of 1 / 10000 (the same words are the keys of
hparams.sampling, there value / 10000 or None for 0, and the keywords of the restatements), and `chain`, the sample_chain of
its restatement.  A scenario runs the shared body and returns what the stage's own assertions look at.

Shapes: B = 2, T = 40, testlib.hp_of() (64 channels, 4 layers, k = 9, 200 steps), 20 visited steps, w = 3.  The inpainting
sampler's time mask covers spectrogram frames [10, 20).  Each reference is computed once per process and shared; it is never
modified."""
import contextlib
import functools

import pytest
import torch

from oracle import diffroll_ref as R
from testlib import S, agree, hp_of, inputs, make_model

import blend_cases as BC
import chain_ref as CR
import clip_ref as CL

from diffroll_amd import longform

B, TN, N_STEPS, W = 2, 40, 20, 3.0
PARAM_SEED, INPUT_SEED, PHILOX_SEED = 0, 100, 9
MASK = [10, 20]
GUIDING = ("cfdg_ddpm_x0", "inpainting_ddpm_x0", "cfdg_ddim_x0")


# ---------------------------------------------------------------------------------------------- inputs and the restatement
def mask_of(sampler):
    return MASK if sampler == "inpainting_ddpm_x0" else None


@functools.lru_cache(maxsize=None)
def setup():
    hp = hp_of()
    p = R.synthetic_params(hp, seed=PARAM_SEED)
    wav, x, noise = inputs(B, TN, INPUT_SEED)
    return hp, p, wav, x, noise


@functools.lru_cache(maxsize=None)
def spec_of(sampler):
    hp, _, wav, _, _ = setup()
    return R.frontend(wav, hp, TN, inpainting_t=mask_of(sampler))


@functools.lru_cache(maxsize=None)
def philox_z():
    return CR.philox_noise(PHILOX_SEED, 0, S, B, TN)


def start_step(strength=0.5):
    """The visited step a chain of that strength begins at (schedule.check_start)."""
    from diffroll_amd.schedule import check_start
    return check_start(None, strength, CR.visited(S, N_STEPS))


@functools.lru_cache(maxsize=None)
def _reference(chain, sampler, values, philox, opts):
    hp, p, _, x, noise = setup()
    kw = dict(opts)
    if kw.get("start") == "strength":
        kw["start"] = start_step()
    return chain(p, hp, sampler, x, spec_of(sampler), philox_z() if philox else noise, N_STEPS, w=W, **dict(values), **kw)


def reference(chain, sampler, values, philox=False, **opts):
    """What the restatement `chain` returns on the shared inputs under `values` (all 0: the options off) - the final roll first."""
    return _reference(chain, sampler, tuple(sorted(values.items())), philox, tuple(sorted(opts.items())))


# ---------------------------------------------------------------------------------------------- the model and the engines
def set_values(m, values):
    for name, value in values.items():
        setattr(m.hparams.sampling, name, value / 10000.0 if value else None)


def stage_model(hp, p, sampler, values, n=N_STEPS, w=W, code=0, v=0, **kw):
    """The facade with hparams.sampling.<option> = value / 10000 for every option of `values` and, where asked for, x0_clip /
    x0_threshold over the range of `code` and the other sampling keys."""
    options = {k: kw.pop(k) for k in ("solver_order", "solver_noise", "guidance_interval", "strength") if k in kw}
    m = make_model(hp, p, sampler=sampler, w=w, inpainting_t=mask_of(sampler), **kw)
    m.hparams.sampling.steps = n or None
    set_values(m, values)
    if code:
        m.hparams.sampling.x0_clip = 1
        m.hparams.norm_args[0:2] = list(CL.BOUNDS[code])
        m.hparams.sampling.x0_threshold = v / 10000.0 if v else None
    for k, val in options.items():
        setattr(m.hparams.sampling, k, val)
    return m


def lab_engine(names):
    """The body of a suite's module-scoped `lab` fixture: a committed engine whose options the kernel tests set; handed back
    with the window options and the options `names` off."""
    hp, p, _, _, _ = setup()
    eng = make_model(hp, p, sampler="cfdg_ddpm_x0").engine
    yield eng
    for name, value in (("window_overlap", 0), ("window_blend", 0), ("window_break", 0), ("draws", 1)) + tuple((n, 0) for n in names):
        eng.set_option(name, value)


def chain_engine(steps=4, sampler="cfdg_ddpm_x0", w=W):
    """(engine, x_T on its device) of a `steps`-step chain on the shared inputs, the front-end run."""
    hp, p, wav, x, _ = setup()
    m = make_model(hp, p, sampler=sampler, w=w)
    m.hparams.sampling.steps = steps
    eng = m.engine
    eng.frontend(wav, TN)
    return eng, x.squeeze(1).to(eng.device).contiguous()


def margin(label, d, note=""):
    print(f"\n{label}: max |d| {d:.3e}{note}")


# ---------------------------------------------------------------------------------------------- the kernel alone
def unconditional(name, B, T):
    """Normal noise beside the noise input, a constant beside the special ones (it keeps them all-equal / inf / NaN)."""
    return torch.randn(B, T, 88, generator=torch.Generator().manual_seed(T)) if name == "noise" else torch.full((B, T, 88), 0.25)


@contextlib.contextmanager
def window_canvases(lab, O, marks, draws):
    """The lab engine as a window batch of overlap O with recording marks and draws; yields the three blend modes, each set as
    it is reached.  Always hands the four options back off."""
    def modes():
        for mode in (0, 1, 2):
            lab.set_option("window_blend", mode)
            yield mode

    try:
        lab.set_option("window_overlap", O)
        lab.set_window_breaks(marks)
        lab.set_option("draws", draws)
        yield modes()
    finally:
        lab.set_option("draws", 1)
        lab.set_window_breaks(())
        lab.set_option("window_blend", 0)
        lab.set_option("window_overlap", 0)


# ---------------------------------------------------------------------------------------------- identities
def unguided_chain_is_untouched(sampler, w, values, off=None):
    """The engine ignores the values for a sampler that does not guide and for a w = 0 chain: the same bits, the captured chain
    replayed (no launch counted), the tail kernel's launches moving as without them.  `off`: the order the options go back to
    0 in (default: as set)."""
    eng, x_T = chain_engine(sampler=sampler, w=w)

    def run(**kw):
        t0 = eng.tail_launches
        return eng.sample(sampler, x_T.clone(), None, w=w, seed=PHILOX_SEED, **kw), eng.tail_launches - t0

    (first, tails), c0 = run(), eng.launch_counts()
    for name, value in values.items():
        eng.set_option(name, value)
    try:
        (again, tails_on), c1 = run(), eng.launch_counts()
        eager, _ = run(use_graph=False)
    finally:
        for name in off or values:
            eng.set_option(name, 0)
    assert torch.equal(again, first) and torch.equal(eager, first)
    assert tails_on == tails
    assert c1 == c0, (c0, c1)                         # (the values are not part of such a chain's key: replayed)


@contextlib.contextmanager
def captured_under(name, a, b, off):
    """The opening of "the value is part of the captured chain's key": a 4-step chain captured under option `name` = a; set to
    b and back, it replays, no launch counted; under b another chain is captured.  Yields (engine, run, the roll under a,
    the launch counts under b) with the option at b; always sets the options `off` to 0."""
    eng, x_T = chain_engine()

    def run():
        return eng.sample("cfdg_ddpm_x0", x_T.clone(), None, w=W, seed=PHILOX_SEED)

    eng.set_option(name, a)
    try:
        first, c0 = run(), eng.launch_counts()
        assert sum(c0) > 0
        eng.set_option(name, b)
        eng.set_option(name, a)
        assert torch.equal(run(), first) and eng.launch_counts() == c0
        eng.set_option(name, b)
        other, c1 = run(), eng.launch_counts()
        assert c1 != c0 and not torch.equal(other, first)
        yield eng, run, first, c1
    finally:
        for n in off:
            eng.set_option(n, 0)


def bad_values_and_step_history(bads, first, second):
    """`bads` {option: values set_option refuses}; then dr_step under solver order 2: setting `first` = (option, value) behind
    two steps ends the history, setting it again to the same value ends nothing, setting `second` ends it."""
    from diffroll_amd.engine import EngineError
    hp, p, wav, x, _ = setup()
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=W)
    eng = m.engine
    for name, values in bads.items():
        for bad in values:
            with pytest.raises(ValueError, match=f"{name}.*{bad}"):
                eng.set_option(name, bad)
    assert all(getattr(eng, name) == 0 for name in bads)
    eng.frontend(wav, TN)
    eng.set_option("sampling_steps", 20)
    eng.set_option("solver_order", 2)
    v = eng.visited_steps()
    xb = x.squeeze(1).to(eng.device).contiguous()

    def step(t):
        eng.step("cfdg_ddpm_x0", xb, None, t, w=W)

    try:
        step(v[0])
        step(v[1])
        eng.set_option(*first)                        # DR_ENAME (-> ValueError) before the option existed
        with pytest.raises(EngineError, match="continues no history"):
            step(v[2])
        step(v[0])
        step(v[1])
        eng.set_option(*first)                        # the same value: nothing ends
        step(v[2])
        eng.set_option(*second)
        with pytest.raises(EngineError, match="continues no history"):
            step(v[3])
    finally:
        for name in bads:
            eng.set_option(name, 0)
    eng.finish()


def steps_outside_the_interval(values, off):
    """dr_step over the visited steps under the interval [60, 140], with `values` and with the options `off` at None: the
    sequence ends where dr_sample ends, and the rolls behind the steps above 140 hold the same bits with and without.
    Returns (facade, dr_sample's roll, the trajectory with, the one without, the index of the first guided step)."""
    hp, p, wav, x, _ = setup()
    m = stage_model(hp, p, "cfdg_ddpm_x0", values, guidance_interval=[60, 140])
    kw = dict(seed=PHILOX_SEED)
    on, _ = m.sample_trajectory(x, wav, **kw)
    whole, _ = m.sample(x, wav, **kw)
    assert torch.equal(whole, on[-1])                 # dr_step follows the rule for its one step
    for name in off:
        setattr(m.hparams.sampling, name, None)
    without, _ = m.sample_trajectory(x, wav, **kw)
    visited = m.visited_steps()
    above = [i for i, t in enumerate(visited) if t > 140]
    first_guided = above[-1] + 1
    assert above and 60 <= visited[first_guided] <= 140
    for i in above:
        assert torch.equal(on[i], without[i]), visited[i]
    return m, whole, on, without, first_guided


# ---------------------------------------------------------------------------------------------- windows
def one(plan):
    return longform.BatchPlan(plans=[plan], first=[0], marks=[], n=plan.n)


def run_batch_windows(m, batch, wavs, x_T, noise, D=1, use_graph=True):
    """sample_long's chain over a batch plan (several recordings, D draws), keeping the windows on the host."""
    return m._sample_windows(batch, wavs, x_T, noise, D, 0, 0, use_graph, True).cpu()


def window_reference(chain, values, recs, marks=(), draws=1, x_T=None, noise=None):
    """The restated chain over the windows of the recordings `recs` (blend_cases.recording tuples) in one batch."""
    hp, p = recs[0][0], recs[0][1]
    if x_T is None:
        x = torch.cat([BC.windows_of(r[4].reshape(r[2].T_c, 88), r[2]) for r in recs], 0)
        z = torch.cat([BC.windows_of(r[5].reshape(-1, r[2].T_c, 88), r[2]) for r in recs], 1)
    else:
        plan = recs[0][2]
        x = torch.cat([BC.windows_of(x_T[d, 0], plan) for d in range(draws)], 0)
        z = torch.cat([BC.windows_of(noise[:, d, 0], plan) for d in range(draws)], 1)
    spec = torch.cat([r[6] for r in recs], 0).repeat(draws, 1, 1)
    return chain(p, hp, BC.SAMPLER, x, spec, z, 0, w=W, O=BC.OPT_O, marks=marks, draws=draws, **values)


# ---------------------------------------------------------------------------------------------- the fused geometry
@contextlib.contextmanager
def fused_geometry(values):
    """3 guided clips x 40 frames at C = 64, 3 layers, k = 9 - the smallest case of tests/fused_cases.py, which runs
    fused_stack+tail under "fused_stack" 2 (fused regardless: the planner's own choice at this size is per-phase), the
    per-phase kernels pinned to the flavours the fused ones are built from.  Yields (hp, p, facade under `values`, wav, x);
    always puts the pins and "fused_stack" back."""
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in ("fused_stack", "fused_tail", "blocked_accumulation")):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp = hp_of(channels=64, layers=3, k=9)
    p = R.synthetic_params(hp, seed=73)
    wav, x, _ = inputs(3, 40, 73)
    m = stage_model(hp, p, "cfdg_ddpm_x0", values)
    eng = m.engine
    pins = {"tune.ksplit_max": (1, 16), "tune.tile": (3201, 0), "tune.pw_nw": (2, 0), "tune.stack_fl": (1, 0)}
    for k, (val, _) in pins.items():
        eng.set_option(k, val)
    eng.set_option("fused_stack", 2)
    try:
        yield hp, p, m, wav, x
    finally:
        eng.set_option("fused_stack", 1)
        for k, (_, val) in pins.items():
            eng.set_option(k, val)


def fused_chain_with_the_options_off(m, wav, x, values):
    """With the stage's options at None the geometry takes the tail kernel; puts the values back and returns that roll."""
    eng = m.engine
    for name in values:
        setattr(m.hparams.sampling, name, None)
    t0 = eng.tail_launches
    off, _ = m.sample(x, wav, seed=5)
    st = eng.launch_state()
    assert st["mode"] == "fused_stack+tail" and eng.tail_launches > t0, st
    set_values(m, values)
    return off


def fused_guided_steps_leave_the_tail_kernel(m, wav, x):
    """Under the options a guided step keeps its fused stack launch and runs head projections, statistics and update as
    ordinary launches; under an interval the unguided steps go through the tail kernel again; captured = eager = per-phase
    launches of the pinned flavours, bit for bit.  Returns the captured roll of the whole-chain guidance."""
    eng = m.engine
    t0 = eng.tail_launches
    g, _ = m.sample(x, wav, seed=5)
    st = eng.launch_state()
    assert st["mode"] == "fused_stack" and eng.tail_launches == t0 and st["fallbacks"] == 0 and st["yields"] == 0, st
    e, _ = m.sample(x, wav, seed=5, use_graph=False)
    assert eng.launch_state()["mode"] == "fused_stack" and eng.tail_launches == t0
    m.hparams.sampling.guidance_interval = [60, 140]
    gi, _ = m.sample(x, wav, seed=5, use_graph=False)
    st = eng.launch_state()
    # 20 visited steps, 8 of them inside [60, 140]: the last steps are unguided and end in the tail kernel
    assert st["mode"] == "fused_stack+tail" and 0 < eng.tail_launches - t0 <= 12 and st["fallbacks"] == 0 and st["yields"] == 0, st
    gig, _ = m.sample(x, wav, seed=5)
    eng.set_option("fused_stack", 0)                  # per-phase launches of the pinned flavours: the same bits
    ppi, _ = m.sample(x, wav, seed=5)
    m.hparams.sampling.guidance_interval = None
    pp, _ = m.sample(x, wav, seed=5)
    assert eng.launch_state()["mode"] == "per_phase"
    assert torch.equal(g, e) and torch.equal(g, pp)
    assert torch.equal(gi, gig) and torch.equal(gi, ppi) and not torch.equal(gi, g)
    return g


def fused_roll_vs_restatement(chain, values, hp, p, wav, x, g, label, note=""):
    """The fused geometry's roll against the restated 20-step chain on the replayed Philox draws; returns what `chain` returns."""
    out = chain(p, hp, "cfdg_ddpm_x0", x, R.frontend(wav, hp, 40), CR.philox_noise(5, 0, S, 3, 40), 20, w=W, **values)
    ok, d = agree(g, out[0])
    margin(label, d, note)
    assert ok, d
    return out


# ---------------------------------------------------------------------------------------------- bf16x3 and bf16
def split_bf16_vs_restatement(chain, values, label, note=""):
    """An 8-step bf16x3 chain on the shared inputs against the restatement; returns what `chain` returns."""
    hp, p, wav, x, noise = setup()
    m = stage_model(hp, p, "cfdg_ddpm_x0", values, n=8, precision="bf16x3")
    out = chain(p, hp, "cfdg_ddpm_x0", x, spec_of("cfdg_ddpm_x0"), noise, 8, w=W, **values)
    assert len(out[1]) == 8
    roll, _ = m.sample(x, wav, noise=noise)
    ok, d = agree(roll, out[0])
    margin(label, d, note)
    assert ok, d
    return out


def bf16_chain_lies_in_the_restatements_band(chain, values, name):
    """tests/test_gpu_bf16.py's chain (8 steps, C = 128, w = 0.5) under `values`: the rms distance of the bf16 roll from the
    restated fp32 chain lies within 0.5 .. 1.5 x that of the restated bf16 chain - both restatements run the stage.  Returns
    (what the fp32 restatement returns, the batch size)."""
    import bf16_ref as Q
    hp, p, x, wav, _ = Q.case_inputs(Q.CHAIN_GEOMETRY, timesteps=Q.CHAIN_STEPS)
    B, T = Q.CHAIN_GEOMETRY[3:]
    nz = torch.randn(Q.CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        spec = R.frontend(wav, hp, T)
    out = chain(p, hp, "cfdg_ddpm_x0", x, spec, nz, 0, w=0.5, **values)
    ref = out[0]
    assert len(out[1]) == Q.CHAIN_STEPS
    with Q.patched(Q.rne, None):
        d_ref = Q.rms(chain(p, hp, "cfdg_ddpm_x0", x, spec, nz, 0, w=0.5, **values)[0] - ref)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16")
    set_values(m, values)
    got = m.sample(x, wav, noise=nz)[0]
    d = Q.rms(got.cpu() - ref)
    print(f"\n{name} bf16 chain: rms distance from the fp32 chain {d:.3e} restated {d_ref:.3e} ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (d, d_ref)
    assert torch.equal(m.sample(x, wav, noise=nz)[0], got)
    assert torch.equal(m.sample(x, wav, noise=nz, use_graph=False)[0], got)
    assert all(getattr(m.engine, option) == value for option, value in values.items())
    return out, B
