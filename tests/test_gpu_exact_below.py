"""Option "exact_below" (include/diffroll_amd.h) on the MI355X: the reverse steps at diffusion step t < v run in exact fp32
whatever precision the engine has selected.

What is held bit for bit: v = timesteps against the f32 engine's chain; a mixed chain against its TWIN - a second engine that
runs the same chain as a dr_step loop and calls dr_set_precision(mode) before the steps t >= v and dr_set_precision(F32)
before the steps t < v; single steps on either side of v; 0 against an engine that never saw the option.  What is held in a
band: the rms distance of a mixed chain from the fp32 HIP chain, against the restated mixed chain's distance from the
oracle's fp32 chain (tests/exact_ref.py; the band 0.5 .. 1.5 of tests/test_gpu_bf16.py / tests/test_gpu_f16.py, whose
precondition tests/test_exact_below_cpu.py holds).

dr_set_precision ends the states a dr_step sequence continues - the history of "solver_order" 2, the states of "cfg_momentum"
and "guidance_stride" (it drops the captured chain, and with it what dr_step left) - so the twin is kept to the stateless
chains.  The stateful combinations are held by three other things: v = timesteps is the f32 engine's chain bit for bit; the
chain as a dr_step loop on ONE engine that has the option set (no dr_set_precision: the state runs across the boundary) is
dr_sample's chain bit for bit; and the band against the combination's own restated chain with the rounding at the steps t >= v
(chain_ref for the solver, tests/momentum_ref.py and tests/stride_ref.py for the other two).

Geometries: tests/bf16_ref.py's CHAIN_GEOMETRY (128 channels: the smallest that fuses, "fused_stack" = 2) and (64, 2, 9, 2,
40) (per phase); 8 or 20 steps."""
import os

import pytest
import torch

import bf16_ref as Q
import chain_ref
import exact_ref as X
from testlib import assert_shared_frames_agree, make_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W = X.W
S = X.CHAIN_STEPS
FUSING, PER_PHASE = X.CHAIN_GEOMETRY, (64, 2, 9, 2, 40)
# (geometry, option "fused_stack"): every step one launch per phase; every step a fused stack, the exact ones with the tail
# kernel; and 64 channels fused regardless - no reduced flavour fuses there, so the chain goes from per-phase launches to
# stack + tail at the boundary
LAUNCHES = {"per_phase": (PER_PHASE, 0), "fusing": (FUSING, 2), "per_phase_then_fused": (PER_PHASE, 2)}
GUIDING = ("cfdg_ddpm_x0", "inpainting_ddpm_x0", "cfdg_ddim_x0")


def _log(line):
    print(line)
    log = os.environ.get("DR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def weight(sampler):
    return W if sampler in GUIDING else 0.0


def build(sampler, prec, geometry=FUSING, steps=S, fused=2, rolls=None):
    """(engine, x (B, T, 88), noise (steps, B, T, 88)) of one geometry on the device; the 8-step inputs on CHAIN_GEOMETRY are
    those of tests/exact_ref.py's restated chains.  rolls: more rolls than clips (option "draws")."""
    hp, p, x, wav, _ = Q.case_inputs(geometry, timesteps=steps)
    B, T = geometry[3:]
    m = make_model(hp, p, sampler=sampler, w=W, precision=prec)
    eng = m.engine
    eng.model = m                                     # (the model owns the engine: keep it alive with it)
    eng.set_option("fused_stack", fused)
    if sampler != "generation_ddpm_x0":
        eng.frontend(wav, T, return_spec=False)
    nz = torch.randn(steps, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    if rolls:
        g = torch.Generator().manual_seed(6)
        x = torch.cat([x, torch.randn(rolls - B, 1, T, 88, generator=g)])
        nz = torch.cat([nz, torch.randn(steps, rolls - B, 1, T, 88, generator=g)], 1)
    return eng, x.squeeze(1).to(eng.device).contiguous(), nz.squeeze(2).to(eng.device).contiguous()


def chain(eng, sampler, x, z, graph=True, seed=0):
    xb = x.clone()
    eng.sample(sampler, xb, z, weight(sampler), seed, 0, graph, True)
    return xb.cpu()


def step_loop(eng, sampler, x, z, visited, seed=0, mode=None, v=0):
    """The chain as dr_steps.  mode: the twin - dr_set_precision(mode) before the steps t >= v, dr_set_precision(F32) before the
    others, on an engine that never saw the option; None: the engine as it is."""
    xb = x.clone()
    for t in visited:
        if mode is not None:
            eng.set_precision(mode if t >= v else "f32")
        eng.step(sampler, xb, None if z is None else z[t], t, weight(sampler), seed, 0)
    eng.finish()
    return xb.cpu()


def down(n):
    return list(range(n - 1, -1, -1))


# ---------------------------------------------------------------------------------------------- 1. all exact is the fp32 chain
@pytest.mark.parametrize("launches", list(LAUNCHES))
def test_every_step_exact_is_the_f32_engines_chain(launches):
    sampler = "cfdg_ddpm_x0"
    geometry, fused = LAUNCHES[launches]
    eng, x, z = build(sampler, "f32", geometry, fused=fused)
    want = chain(eng, sampler, x, z)
    assert torch.equal(chain(eng, sampler, x, z, graph=False), want)
    exact_mode = eng.launch_state()["mode"]
    assert exact_mode == ("fused_stack+tail" if fused else "per_phase")
    for mode in ("bf16", "f16", "bf16x3"):
        eng, x, z = build(sampler, mode, geometry, fused=fused)
        reduced = chain(eng, sampler, x, z)
        assert eng.launch_state()["mode"] != "fused_stack+tail"          # (the tail kernel is fp32 only)
        eng.set_option("exact_below", S)
        for graph in (False, True):
            got = chain(eng, sampler, x, z, graph=graph)
            assert torch.equal(got, want), (mode, graph, float((got - want).abs().max()))
            assert eng.launch_state()["mode"] == exact_mode, (mode, graph)
        assert not torch.equal(reduced, want)
        eng.set_option("exact_below", 0)
        assert torch.equal(chain(eng, sampler, x, z), reduced)


# ---------------------------------------------------------------------------------------------- 2. the twin
TWINS = [("bf16", "cfdg_ddpm_x0", "philox"), ("bf16", "generation_ddpm_x0", "injected"), ("bf16", "cfdg_ddim_x0", "injected"),
         ("f16", "cfdg_ddpm_x0", "philox"), ("bf16x3", "cfdg_ddpm_x0", "philox")]


@pytest.mark.parametrize("launches", list(LAUNCHES))
@pytest.mark.parametrize("mode,sampler,noise", TWINS, ids=["%s-%s-%s" % c for c in TWINS])
def test_a_mixed_chain_is_its_twin(mode, sampler, noise, launches):
    v = 3
    geometry, fused = LAUNCHES[launches]
    eng, x, z = build(sampler, mode, geometry, fused=fused)
    two, _, _ = build(sampler, mode, geometry, fused=fused)
    z = z if noise == "injected" else None
    eng.set_option("exact_below", v)
    want = step_loop(two, sampler, x, z, down(S), seed=3, mode=mode, v=v)
    for graph in (False, True):
        got = chain(eng, sampler, x, z, graph=graph, seed=3)
        assert torch.equal(got, want), (graph, float((got - want).abs().max()))
    # ... and it is neither the all-reduced chain nor the exact one
    two.set_precision(mode)
    assert not torch.equal(chain(two, sampler, x, z, seed=3), want)
    two.set_precision("f32")
    assert not torch.equal(chain(two, sampler, x, z, seed=3), want)


# ---------------------------------------------------------------------------------------------- 3. the band
_f32_chain = {}


def f32_hip_chain(sampler):
    if sampler not in _f32_chain:
        eng, x, z = build(sampler, "f32")
        _f32_chain[sampler] = chain(eng, sampler, x, z)
    return _f32_chain[sampler]


@pytest.mark.parametrize("mode,sampler,v", X.BAND_CASES, ids=["%s-%s-v%d" % c for c in X.BAND_CASES])
def test_a_mixed_chain_lies_in_the_restated_chains_band(mode, sampler, v):
    d_ref = X.distance(mode, sampler, v)
    eng, x, z = build(sampler, mode)
    eng.set_option("exact_below", v)
    got = chain(eng, sampler, x, z)
    d = Q.rms(got - f32_hip_chain(sampler))
    _log(f"exact_below_chain[{mode},{sampler},{S} steps,v={v}] rms distance from the fp32 HIP chain {d:.3e} restated (from the oracle's fp32 chain) "
         f"{d_ref:.3e} ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (mode, sampler, v, d, d_ref)
    assert torch.equal(chain(eng, sampler, x, z, graph=False), got)


# ---------------------------------------------------------------------------------------------- 4. which kernels ran
LABEL = {"bf16": ", bf16, ", "f16": ", f16, ", "bf16x3": ", split-bf16, "}


@pytest.mark.parametrize("mode", ["bf16", "f16", "bf16x3"])
def test_the_selected_modes_kernels_above_the_boundary_and_the_fp32_ones_below(mode):
    sampler, v = "cfdg_ddpm_x0", 3
    eng, x, z = build(sampler, mode)
    eng.set_option("exact_below", v)
    eng.profile_enable(True)
    xb = x.clone()
    for t in down(S):
        eng.step(sampler, xb, z[t], t, W)
        n, _, _, name = eng.profile_read_ex()
        assert n >= 1 and name.startswith("stack_kernel<"), (t, name)
        if t >= v:
            assert LABEL[mode] in name and eng.launch_state()["mode"] == "fused_stack", (t, name)
        else:
            assert not any(lab in name for lab in LABEL.values()), (t, name)
            assert "blocked accumulation)" in name or "one fp32 chain per output)" in name, (t, name)
            assert eng.launch_state()["mode"] == "fused_stack+tail", (t, eng.launch_state())
    eng.profile_enable(False)
    # the launches of an eager chain: a reduced step is input layer, shared first conv, stack (and heads, update); the first
    # exact step computes its own input layer and first conv, every later one is stack + tail alone
    eng.stack_status()
    s0, c0 = eng.launch_state(), eng.launch_counts()
    chain(eng, sampler, x, z, graph=False)
    s1, c1 = eng.launch_state(), eng.launch_counts()
    assert s1["stack_launches"] - s0["stack_launches"] == S
    assert s1["tail_launches"] - s0["tail_launches"] == v
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (S - v + 1, S - v + 1), (c0, c1)
    assert s1["mode"] == "fused_stack+tail" and s1["fallbacks"] == s0["fallbacks"]


# ---------------------------------------------------------------------------------------------- 5. dr_step alone
@pytest.mark.parametrize("launches", list(LAUNCHES))
def test_single_steps_on_either_side_of_the_boundary(launches):
    sampler, v = "cfdg_ddpm_x0", 3
    geometry, fused = LAUNCHES[launches]
    eng, x, z = build(sampler, "bf16", geometry, fused=fused)
    eng.set_option("exact_below", v)
    exact, _, _ = build(sampler, "f32", geometry, fused=fused)
    plain, _, _ = build(sampler, "bf16", geometry, fused=fused)

    def one(e, t):
        xb = x.clone()
        e.step(sampler, xb, z[t], t, W)
        e.finish()
        return xb.cpu()
    assert torch.equal(one(eng, v - 1), one(exact, v - 1))           # t = v - 1 is exact
    assert torch.equal(one(eng, 0), one(exact, 0))
    assert torch.equal(one(eng, v), one(plain, v))                   # t = v is the selected mode's
    assert not torch.equal(one(plain, v), one(exact, v)) and not torch.equal(one(plain, v - 1), one(exact, v - 1))
    # dr_forward is a network evaluation, not a chain step: it keeps the engine's mode at every t
    for t in (0, v - 1, v):
        assert torch.equal(eng.forward(x, t, False), plain.forward(x, t, False)), t
        assert not torch.equal(eng.forward(x, t, False), exact.forward(x, t, False)), t
    steps = [0, v][: x.shape[0]] + [v - 1] * max(0, x.shape[0] - 2)
    assert torch.equal(eng.forward_steps(x, steps, False), plain.forward_steps(x, steps, False))


# ---------------------------------------------------------------------------------------------- 6. off is off
def _replay_marks(eng):
    st = eng.launch_state()
    return eng.cold_times()[3], eng.launch_counts(), st["stack_launches"], st["tail_launches"]


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16", "f16"])
def test_zero_is_an_engine_that_never_saw_the_option(mode):
    sampler = "cfdg_ddpm_x0"
    never, x, z = build(sampler, mode)
    want = chain(never, sampler, x, z)
    eng, _, _ = build(sampler, mode)
    first = chain(eng, sampler, x, z)
    marks = _replay_marks(eng)
    assert torch.equal(first, want)
    eng.set_option("exact_below", 0)
    assert torch.equal(chain(eng, sampler, x, z), want) and _replay_marks(eng) == marks      # replayed: no capture, no launch counted
    eng.set_option("exact_below", 5)
    moved = chain(eng, sampler, x, z)
    if mode == "f32":                                 # accepted, changes nothing: the same chain is replayed
        assert torch.equal(moved, want) and _replay_marks(eng) == marks
        return
    marks5 = _replay_marks(eng)
    assert marks5 != marks and not torch.equal(moved, want)           # 0 -> 5 drops the chain
    eng.set_option("exact_below", 5)
    assert torch.equal(chain(eng, sampler, x, z), moved) and _replay_marks(eng) == marks5      # 5 -> 5 keeps it
    eng.set_option("exact_below", 0)
    assert torch.equal(chain(eng, sampler, x, z), want)


# ---------------------------------------------------------------------------------------------- 7. combinations
def _visited(n_steps, n):
    return chain_ref.visited(n_steps, n)


STATELESS = {
    # name -> (steps of the model, v, options of dr_set_option)
    "steps-5-of-20": (20, 7, dict(sampling_steps=5)),                  # visited 19 14 10 5 0: v between 5 and 10
    "guidance_interval": (8, 3, dict(guidance_t_min=2, guidance_t_max=5)),
    "strength": (8, 3, dict(start_step=5)),                            # strength 0.75 of 8 steps: the chain starts at step 5
    "x0_clip+x0_threshold": (8, 3, dict(x0_clip=1, x0_threshold=9950)),
    "solver_order-1+noise": (8, 3, dict(solver_order=1, solver_noise=1)),
}


@pytest.mark.parametrize("name", list(STATELESS))
def test_stateless_combinations_are_their_twins(name):
    steps, v, options = STATELESS[name]
    sampler, mode = "cfdg_ddpm_x0", "bf16"
    eng, x, z = build(sampler, mode, steps=steps)
    two, _, _ = build(sampler, mode, steps=steps)
    for e in (eng, two):
        for k, val in options.items():
            e.set_option(k, val)
    eng.set_option("exact_below", v)
    visited = _visited(steps, options.get("sampling_steps", 0))
    if "start_step" in options:
        visited = visited[visited.index(options["start_step"]):]
    assert any(t >= v for t in visited) and any(t < v for t in visited)
    if name == "steps-5-of-20":
        assert visited == [19, 14, 10, 5, 0] and v not in visited          # v falls between two visited steps
    want = step_loop(two, sampler, x, z, visited, mode=mode, v=v)
    for graph in (False, True):
        got = chain(eng, sampler, x, z, graph=graph)
        assert torch.equal(got, want), (name, graph, float((got - want).abs().max()))
    two.set_precision(mode)
    assert not torch.equal(chain(two, sampler, x, z), want)


def test_draws_are_their_twin():
    sampler, mode, v = "cfdg_ddpm_x0", "bf16", 3
    B = FUSING[3]
    eng, x, z = build(sampler, mode, rolls=2 * B)
    two, _, _ = build(sampler, mode, rolls=2 * B)
    for e in (eng, two):
        e.set_option("draws", 2)
    eng.set_option("exact_below", v)
    want = step_loop(two, sampler, x, z, down(S), mode=mode, v=v)
    for graph in (False, True):
        assert torch.equal(chain(eng, sampler, x, z, graph=graph), want), graph
    # Philox: the two draws of a clip differ, and the chain is its twin too
    want = step_loop(two, sampler, x, None, down(S), seed=4, mode=mode, v=v)
    got = chain(eng, sampler, x, None, seed=4)
    assert torch.equal(got, want)


def test_windows_with_the_linear_blend_are_their_twin_and_share_their_frames():
    """Three 32-frame windows sharing 5 frames, the linear cross-fade, 8 steps."""
    import blend_cases as BC
    from diffroll_amd import longform
    sampler, mode, v, O = BC.SAMPLER, "bf16", 3, 5
    hp, p, plan, wav, x_T, noise, _ = BC.recording(O, 3205, steps=S)
    engines = []
    for _ in range(2):
        m = make_model(hp, p, sampler=sampler, w=BC.W, precision=mode)
        e = m.engine
        e.model = m
        e.set_option("fused_stack", 2)
        e.frontend(longform.window_audio(wav, plan, BC.HOP), plan.T, return_spec=False)
        e.set_option("window_overlap", O)
        e.set_option("window_blend", 1)
        engines.append(e)
    eng, two = engines
    xw = longform.gather_windows(x_T.reshape(plan.T_c, 88), plan).to(eng.device).contiguous()
    z = longform.gather_windows(noise.reshape(S, plan.T_c, 88), plan).to(eng.device).contiguous()
    eng.set_option("exact_below", v)
    want = step_loop(two, sampler, xw, z, down(S), mode=mode, v=v)
    for graph in (False, True):
        got = chain(eng, sampler, xw, z, graph=graph)
        assert torch.equal(got, want), graph
        assert_shared_frames_agree(got, plan)
    two.set_precision(mode)
    assert not torch.equal(chain(two, sampler, xw, z), want)


STATEFUL = {
    "solver_order-2": dict(solver_order=2),
    "solver_order-2+noise": dict(solver_order=2, solver_noise=1),
    "cfg_project+cfg_momentum": dict(cfg_project=10000, cfg_momentum=-5000),
    "guidance_stride-2": dict(guidance_stride=2),
}


@pytest.mark.parametrize("name", list(STATEFUL))
def test_stateful_combinations(name):
    """The states run across the boundary: dr_set_precision would end them, so no twin.  v = S is the f32 engine's chain, and
    the chain as a dr_step loop on the engine that has the option set is dr_sample's chain, bit for bit.  That the mixed chain
    is the right one is the next two tests' business: the band against the combination's own restated chain."""
    sampler, mode, v, options = "cfdg_ddpm_x0", "bf16", 3, STATEFUL[name]
    exact, x, z = build(sampler, "f32")
    eng, _, _ = build(sampler, mode)
    for e in (exact, eng):
        for k, val in options.items():
            e.set_option(k, val)
    want32 = chain(exact, sampler, x, z)
    reduced = chain(eng, sampler, x, z)
    eng.set_option("exact_below", S)
    for graph in (False, True):
        assert torch.equal(chain(eng, sampler, x, z, graph=graph), want32), graph
    eng.set_option("exact_below", v)
    mixed = chain(eng, sampler, x, z)
    assert torch.equal(chain(eng, sampler, x, z, graph=False), mixed)
    assert torch.equal(step_loop(eng, sampler, x, z, down(S)), mixed)
    assert not torch.equal(mixed, want32) and not torch.equal(mixed, reduced)


@pytest.mark.parametrize("name,v", X.STATEFUL_BAND, ids=["%s-v%d" % c for c in X.STATEFUL_BAND])
def test_momentum_and_stride_lie_in_their_restated_chains_band(name, v):
    """ "cfg_project" + "cfg_momentum" and "guidance_stride" 2 with the state carried across the boundary: the rms distance of
    the mixed HIP chain from the f32 HIP chain under the same options lies within 0.5 .. 1.5 x the distance of the
    combination's own restated chain (tests/momentum_ref.py / tests/stride_ref.py), rounded at the steps t >= v, from that
    restated chain in fp32.  A state that restarted, or was lost, at the boundary is another chain: at v = 3 the restated
    distance is 3.5e-5 / 1.7e-5, a twentieth of the all-reduced chain's."""
    sampler, mode, options = "cfdg_ddpm_x0", "bf16", X.stateful_options(name)
    assert options == STATEFUL[name]
    d_ref = X.stateful_distance(name, v)
    assert d_ref > 1e-5, d_ref
    exact, x, z = build(sampler, "f32")
    eng, _, _ = build(sampler, mode)
    for e in (exact, eng):
        for k, val in options.items():
            e.set_option(k, val)
    eng.set_option("exact_below", v)
    got = chain(eng, sampler, x, z)
    d = Q.rms(got - chain(exact, sampler, x, z))
    _log(f"exact_below_chain[{mode},{sampler},{name},{S} steps,v={v}] rms distance from the fp32 HIP chain {d:.3e} restated {d_ref:.3e} "
         f"ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (name, v, d, d_ref)
    assert torch.equal(chain(eng, sampler, x, z, graph=False), got)


@pytest.mark.parametrize("noise", [0, 1], ids=["2M", "2M-sde"])
def test_solver_order_2_lies_in_the_restated_chains_band(noise):
    sampler, mode, v = "cfdg_ddpm_x0", "bf16", 1
    hp, p, x, wav, spec, nz = X.chain_inputs()
    kw = dict(w=W, order=2, solver_noise=noise)
    ref = chain_ref.sample_chain(p, hp, sampler, x, spec, nz, 0, **kw)
    d_ref = Q.rms(X.sample_chain(Q.rne, None, v, p, hp, sampler, x, spec, nz, 0, **kw) - ref)
    assert d_ref > 1e-5, d_ref
    exact, xd, z = build(sampler, "f32")
    eng, _, _ = build(sampler, mode)
    for e in (exact, eng):
        e.set_option("solver_order", 2)
        e.set_option("solver_noise", noise)
    eng.set_option("exact_below", v)
    d = Q.rms(chain(eng, sampler, xd, z) - chain(exact, sampler, xd, z))
    _log(f"exact_below_chain[{mode},{sampler},solver_order 2 solver_noise {noise},{S} steps,v={v}] rms distance from the fp32 HIP chain {d:.3e} "
         f"restated {d_ref:.3e} ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (d, d_ref)


@pytest.mark.parametrize("G", [2, 3])
def test_fake_ranks_take_the_option_with_the_model(G):
    """sample_sharded hands the model - precision and hparams.sampling - to every rank.  With v = timesteps the assembled rolls
    are the f32 model's, bit for bit.  With v = 3 every rank's shard is its twin bit for bit - the same shard as a dr_step loop
    on a second engine that never saw the option, dr_set_precision switched at the boundary - and every rank's chain ran on an
    engine that had been given the value."""
    from diffroll_amd.distributed import sample_shard, sample_sharded_sequential, shard_bounds
    from testlib import shard_model
    sampler, mode, v = "cfdg_ddpm_x0", "bf16", 3
    hp, p, m32 = shard_model(steps=S)
    torch.manual_seed(5)
    B, Tn = 5, 40
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    noise = torch.randn(S, B, 1, Tn, 88)
    want = sample_sharded_sequential(m32, x, wav, noise, seed=3, world_size=G).cpu()
    m = make_model(hp, p, sampler=sampler, w=W, precision=mode)
    m.hparams.sampling.exact_below = S
    got = sample_sharded_sequential(m, x, wav, noise, seed=3, world_size=G).cpu()
    assert torch.equal(got, want), float((got - want).abs().max())
    m.hparams.sampling.exact_below = v
    eng = m.engine
    seen, sample = [], eng.sample

    def spy(*a, **k):
        seen.append((eng.exact_below, eng.precision))
        return sample(*a, **k)
    eng.sample = spy
    shards = [sample_shard(m, x, wav, noise, 3, r, G).cpu() for r in range(G)]
    eng.sample = sample
    assert seen == [(v, mode)] * G, seen              # (B = 5 over 2 or 3 ranks: no shard is empty)
    mt = make_model(hp, p, sampler=sampler, w=W, precision=mode)
    two = mt.engine
    for r in range(G):
        lo, hi = shard_bounds(B, r, G)
        two.frontend(wav[lo:hi], Tn, return_spec=False)
        xs = x[lo:hi].squeeze(1).to(two.device).contiguous()
        zs = noise[:, lo:hi].squeeze(2).to(two.device).contiguous()
        twin = step_loop(two, sampler, xs, zs, down(S), seed=3, mode=mode, v=v)
        assert torch.equal(shards[r].squeeze(1), twin), (r, float((shards[r].squeeze(1) - twin).abs().max()))
    mixed = sample_sharded_sequential(m, x, wav, noise, seed=3, world_size=G).cpu()
    assert torch.equal(mixed, torch.cat(shards, 0)) and not torch.equal(mixed, want)


# ---------------------------------------------------------------------------------------------- 8. range
def test_values_out_of_range_are_refused_and_the_previous_value_stays():
    from diffroll_amd import _cabi
    sampler = "cfdg_ddpm_x0"
    eng, x, z = build(sampler, "bf16")
    eng.set_option("exact_below", 3)
    want = chain(eng, sampler, x, z)
    marks = _replay_marks(eng)
    for bad in (-1, S + 1):
        assert eng.lib.dr_set_option(eng.h, b"exact_below", bad) == _cabi.DR_EINVAL
        assert b"exact_below is 0 (off) or v in [1, timesteps = 8]" in eng.lib.dr_last_error(eng.h)
        with pytest.raises(ValueError, match="exact_below"):
            eng.set_option("exact_below", bad)
        assert eng.exact_below == 3
        assert torch.equal(chain(eng, sampler, x, z), want) and _replay_marks(eng) == marks
    for ok in (0, S):
        eng.set_option("exact_below", ok)
    plain, _, _ = build(sampler, "bf16")
    assert not torch.equal(chain(plain, sampler, x, z), want)
