"""Parity of the HIP engine (through the C-ABI) against the golden vectors produced by the
reference and against the CPU oracle.  Needs a real MI355X: ``pytest -m gpu``.

Tolerances: ATOL_FWD / ATOL_STEP / ATOL_SPEC / ATOL_SHARD of tests/testlib.py, where their reasons are given.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import diffroll_ref as R
from testlib import ATOL_FWD, ATOL_SHARD, ATOL_SPEC, ATOL_STEP, cfg2_inputs, make_model, maxdiff

pytestmark = pytest.mark.gpu


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return {k: z[k] for k in z.files}


def T(a):
    return torch.from_numpy(np.asarray(a))


def fixture_model(g, **kw):
    hp = json.loads(str(g["hp"]))
    p = R.synthetic_params(hp, seed=int(g["seed"]))
    return hp, p, make_model(hp, p, **kw)


# --------------------------------------------------------------------------------------------
def test_library_is_loaded_and_native():
    from diffroll_amd import _cabi
    lib = _cabi.load_library()
    assert lib.dr_abi_version() == _cabi.DR_ABI_VERSION
    maps = open("/proc/self/maps").read()
    assert "libdiffroll_amd.so" in maps


def test_frontend_golden(golden_dir):
    g = load(golden_dir, "frontend")
    hp = json.loads(str(g["hp"]))
    p = R.synthetic_params(hp, seed=1)
    m = make_model(hp, p)
    wav = T(g["wav"])
    Tn = int(g["T"])
    eng = m.engine
    for key, kw in (("spec", {}), ("spec_t", dict(inpainting_t=[4, 9])), ("spec_f", dict(inpainting_f=[20, 100])),
                    ("spec_tf", dict(inpainting_t=[4, 9], inpainting_f=[20, 100]))):
        spec = eng.frontend(wav, Tn, **kw).cpu().numpy()
        assert spec.shape == g[key].shape
        d = maxdiff(spec, g[key])
        assert d <= ATOL_SPEC, (key, d)
    # silence: NaN -> 0 exactly (model/utils.py:29-31)
    assert np.all(eng.frontend(wav, Tn).cpu().numpy()[3] == 0.0)


@pytest.mark.parametrize("name", ["forward_k3", "forward_k9", "forward_k15", "forward_wide_k9"])
def test_forward_golden(golden_dir, name):
    g = load(golden_dir, name)
    hp, p, m = fixture_model(g)
    x, wav = T(g["x"]), T(g["wav"])
    t = torch.tensor(int(g["t"])).repeat(x.shape[0])
    x0_c, spec = m(x, wav, t)
    x0_u, spec_u = m(x, torch.zeros_like(wav), t, sampling=True)
    assert x0_c.shape == g["x0_c"].shape
    assert maxdiff(x0_c.cpu(), g["x0_c"]) <= ATOL_FWD, maxdiff(x0_c.cpu(), g["x0_c"])
    assert maxdiff(x0_u.cpu(), g["x0_u"]) <= ATOL_FWD, maxdiff(x0_u.cpu(), g["x0_u"])
    assert bool((spec_u == -1).all())
    if "x0_i" in g:
        x0_i, spec_i = m(x, wav, t, inpainting_t=[10, 20])
        assert maxdiff(x0_i.cpu(), g["x0_i"]) <= ATOL_FWD
        assert maxdiff(spec_i.cpu(), g["spec_i"]) <= ATOL_SPEC
        assert maxdiff(spec.cpu(), g["spec"]) <= ATOL_SPEC


@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "inpainting_ddpm_x0", "generation_ddpm_x0", "ddpm_x0"])
def test_steps_and_chain_golden(golden_dir, sampler):
    g = load(golden_dir, "steps_chain_k9")
    it = [int(v) for v in g["inpainting_t"]] if sampler == "inpainting_ddpm_x0" else None
    hp, p, m = fixture_model(g, sampler=sampler, w=float(g["w"]), inpainting_t=it)
    S = hp["timesteps"]
    x, wav, noise = T(g["x"]), T(g["wav"]), T(g["noise"])
    for t_index in (S - 1, 1, 0):
        out, spec = m.reverse_diffusion(x, wav, t_index, noise=noise[t_index])
        d = maxdiff(out.cpu(), g[f"{sampler}_t{t_index}"])
        assert d <= ATOL_STEP, (t_index, d)
    for use_graph in (False, True):
        roll, _ = m.sample(x, wav, noise=noise, use_graph=use_graph)
        d = maxdiff(roll.cpu(), g[f"{sampler}_chain"])
        assert d <= ATOL_STEP, (use_graph, d)


@pytest.mark.parametrize("sampler", ["ddim_x0", "cfdg_ddim_x0", "ddpm", "ddim", "ddim2ddpm"])
def test_extra_samplers_golden(golden_dir, sampler):
    """the remaining samplers against vectors produced by the reference."""
    g = load(golden_dir, "steps_chain_extra_k9")
    hp, p, m = fixture_model(g, sampler=sampler, w=float(g["w"]))
    S = hp["timesteps"]
    x, wav, noise = T(g["x"]), T(g["wav"]), T(g["noise"])
    for t_index in (S - 1, 1, 0):
        out, spec = m.reverse_diffusion(x, wav, t_index, noise=noise[t_index])
        d = maxdiff(out.cpu(), g[f"{sampler}_t{t_index}"])
        assert d <= ATOL_STEP, (t_index, d)
    for use_graph in (False, True):
        roll, _ = m.sample(x, wav, noise=noise, use_graph=use_graph)
        d = maxdiff(roll.cpu(), g[f"{sampler}_chain"])
        assert d <= ATOL_STEP, (use_graph, d)


# --------------------------------------------------------------------------------------------
# full-size network (k=9, C=512, 15 layers) against the oracle
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_model():
    hp = dict(R.DEFAULT_HP)
    p = R.synthetic_params(hp, seed=0)
    return hp, p, make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)


def test_full_size_forward_vs_oracle(full_model):
    hp, p, m = full_model
    torch.manual_seed(0)
    B, L = 2, 64000
    Tn = L // 512
    wav = 0.1 * torch.randn(B, L)
    x = torch.randn(B, 1, Tn, 88)
    t = torch.tensor(117).repeat(B)
    with torch.no_grad():
        ref_c, ref_spec = R.forward(p, hp, x, wav, t)
        ref_u, _ = R.forward(p, hp, x, torch.zeros_like(wav), t, sampling=True)
    x0_c, spec = m(x, wav, t)
    x0_u, _ = m(x, wav, t, sampling=True)
    assert maxdiff(spec.cpu(), ref_spec) <= ATOL_SPEC
    assert maxdiff(x0_c.cpu(), ref_c) <= ATOL_FWD, maxdiff(x0_c.cpu(), ref_c)
    assert maxdiff(x0_u.cpu(), ref_u) <= ATOL_FWD, maxdiff(x0_u.cpu(), ref_u)


def test_config1_chain_vs_oracle():
    """BASELINE config 1: k=9, 50 steps, batch 1, 4 s clip, cfdg w=0.5 - whole chain vs the oracle,
    and the thresholded roll (> 0.5) identical except within the tolerance of the threshold."""
    hp = dict(R.DEFAULT_HP)
    hp["timesteps"] = 50
    p = R.synthetic_params(hp, seed=0)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    torch.manual_seed(0)
    L = 64000
    Tn = L // 512
    wav = 0.1 * torch.randn(1, L)
    x = torch.randn(1, 1, Tn, 88)
    noise = torch.randn(50, 1, 1, Tn, 88)
    with torch.no_grad():
        ref = R.sample_chain(p, hp, "cfdg_ddpm_x0", x, wav, noise, w=0.5)
    roll, _ = m.sample(x, wav, noise=noise)
    roll = roll.cpu()
    d = maxdiff(roll, ref)
    assert d <= ATOL_STEP, d
    near = (ref - 0.5).abs() < ATOL_STEP
    assert bool((((roll > 0.5) == (ref > 0.5)) | near).all())


def test_config5_shape_step_vs_oracle():
    """BASELINE config 5 geometry - k=15, 640-frame segments, 4 clips per GPU - full width and depth: one
    classifier-free-guidance step (2 x 4 evaluations: 160-frame conv blocks, 160-frame 1x1 blocks, the shared
    first-layer contraction) against the oracle with injected noise."""
    hp = dict(R.DEFAULT_HP)
    hp.update(kernel_size=15, timesteps=200)
    p = R.synthetic_params(hp, seed=15)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    torch.manual_seed(5)
    B, Tn = 4, 640
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    z = torch.randn(B, 1, Tn, 88)
    sch = R.schedule(hp["beta_start"], hp["beta_end"], 200)
    with torch.no_grad():
        spec = R.frontend(wav, hp, Tn)
        ref = R.reverse_step(p, hp, sch, "cfdg_ddpm_x0", x, spec, 150, z, 0.5)
    out, _ = m.reverse_diffusion(x, wav, 150, noise=z)
    assert maxdiff(out.cpu(), ref) <= ATOL_STEP, maxdiff(out.cpu(), ref)


def test_config5_shape_chain_vs_oracle():
    """BASELINE config 5 geometry as a chain: k=15 full-size network, one 640-frame clip, the last 12 reverse steps
    of a 200-step schedule run back to back (inpainting sampler with a masked spectrogram span) vs the oracle."""
    hp = dict(R.DEFAULT_HP)
    hp.update(kernel_size=15, timesteps=200)
    p = R.synthetic_params(hp, seed=15)
    m = make_model(hp, p, sampler="inpainting_ddpm_x0", w=0.5, inpainting_t=[200, 330])
    torch.manual_seed(6)
    Tn = 640
    wav = 0.1 * torch.randn(1, Tn * 512)
    x = torch.randn(1, 1, Tn, 88)
    steps = list(range(11, -1, -1))
    z = torch.randn(len(steps), 1, 1, Tn, 88)
    sch = R.schedule(hp["beta_start"], hp["beta_end"], 200)
    ref, out = x, x
    with torch.no_grad():
        spec = R.frontend(wav, hp, Tn, inpainting_t=[200, 330])
        for i, t in enumerate(steps):
            ref = R.reverse_step(p, hp, sch, "inpainting_ddpm_x0", ref, spec, t, z[i], 0.5)
    for i, t in enumerate(steps):
        out, _ = m.reverse_diffusion(out, wav, t, noise=z[i])
    assert maxdiff(out.cpu(), ref) <= ATOL_STEP, maxdiff(out.cpu(), ref)


def test_config3_generation_steps_vs_oracle(full_model):
    """BASELINE config 3 per-GPU geometry: unconditional generation (spec == -1), 16 clips of 125 frames - three
    consecutive reverse steps (one evaluation each, 64-frame blocks) against the oracle."""
    hp, p, _ = full_model
    m = make_model(hp, p, sampler="generation_ddpm_x0", w=0.0)
    torch.manual_seed(3)
    B, Tn = 16, 125
    x = torch.randn(B, 1, Tn, 88)
    z = torch.randn(3, B, 1, Tn, 88)
    sch = R.schedule(hp["beta_start"], hp["beta_end"], hp["timesteps"])
    spec = torch.full((B, hp["n_mels"], Tn), -1.0)
    ref, out = x, x
    with torch.no_grad():
        for i, t in enumerate((120, 119, 118)):
            ref = R.reverse_step(p, hp, sch, "generation_ddpm_x0", ref, spec, t, z[i], 0.0)
    for i, t in enumerate((120, 119, 118)):
        out, _ = m.reverse_diffusion(out, None, t, noise=z[i])
    assert maxdiff(out.cpu(), ref) <= ATOL_STEP, maxdiff(out.cpu(), ref)


def test_config2_real_batch_guided_step_vs_oracle(full_model):
    """BASELINE config 2 at its REAL batch: 16 clips of 125 frames through the full k=9 network, one classifier-free
    guided reverse step (cfdg_ddpm_x0, w=0.5: a 32-sample evaluation, the launch geometry of the bench line) and
    the conditional evaluation on its own, against the oracle (task/diffusion.py:943-969)."""
    hp, p, m = full_model
    torch.manual_seed(16)
    B, Tn = 16, 125
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    z = torch.randn(B, 1, Tn, 88)
    sch = R.schedule(hp["beta_start"], hp["beta_end"], hp["timesteps"])
    t = 150
    with torch.no_grad():
        spec = R.frontend(wav, hp, Tn)
        ref = R.reverse_step(p, hp, sch, "cfdg_ddpm_x0", x, spec, t, z, 0.5)
        ref_c, _ = R.forward(p, hp, x, wav, torch.tensor(t).repeat(B))
    out, sp = m.reverse_diffusion(x, wav, t, noise=z)
    assert maxdiff(sp.cpu(), spec) <= ATOL_SPEC
    assert maxdiff(out.cpu(), ref) <= ATOL_STEP, maxdiff(out.cpu(), ref)
    x0_c, _ = m(x, wav, torch.tensor(t).repeat(B))
    assert maxdiff(x0_c.cpu(), ref_c) <= ATOL_FWD, maxdiff(x0_c.cpu(), ref_c)


def test_config4_full_size_inpainting_step_vs_oracle(full_model):
    """BASELINE config 4 per-GPU geometry at full size: inpainting_ddpm_x0 (w=0.5) on 16 clips of 125 frames with
    the spectrogram frames [T/4, T/2) masked to -1 after normalisation (model/diffwave.py:649-654; the reference
    never masks the roll, task/diffusion.py:999-1025) - two consecutive reverse steps against the oracle."""
    hp, p, _ = full_model
    B, Tn = 16, 125
    it = [Tn // 4, Tn // 2]
    m = make_model(hp, p, sampler="inpainting_ddpm_x0", w=0.5, inpainting_t=it)
    torch.manual_seed(44)
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    z = torch.randn(2, B, 1, Tn, 88)
    sch = R.schedule(hp["beta_start"], hp["beta_end"], hp["timesteps"])
    ref, out = x, x
    with torch.no_grad():
        spec = R.frontend(wav, hp, Tn, inpainting_t=it)
        for i, t in enumerate((199, 198)):
            ref = R.reverse_step(p, hp, sch, "inpainting_ddpm_x0", ref, spec, t, z[i], 0.5)
    assert bool((spec[:, :, it[0]:it[1]] == -1).all()) and not bool((spec[:, :, :it[0]] == -1).any())
    for i, t in enumerate((199, 198)):
        out, sp = m.reverse_diffusion(out, wav, t, noise=z[i])
    assert maxdiff(sp.cpu(), spec) <= ATOL_SPEC
    assert maxdiff(out.cpu(), ref) <= ATOL_STEP, maxdiff(out.cpu(), ref)


def test_full_200_step_guided_chain_vs_oracle(full_model):
    """The north_star statement itself at full depth: the k=9, C=512, 15-layer network, all 200 reverse steps of
    cfdg_ddpm_x0 (w=0.5) on 4-s clips with identical injected noise - final roll within the fp32 tolerance of the
    oracle and the thresholded roll (> 0.5, what frame-F1 is computed from) identical except within the tolerance of the
    threshold; in both precisions."""
    hp, p, _ = full_model
    torch.manual_seed(200)
    B, Tn = 2, 125
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    noise = torch.randn(hp["timesteps"], B, 1, Tn, 88)
    with torch.no_grad():
        ref = R.sample_chain(p, hp, "cfdg_ddpm_x0", x, wav, noise, w=0.5)
    near = (ref - 0.5).abs() < ATOL_STEP
    for precision in ("f32", "bf16x3"):
        m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision=precision)
        roll, _ = m.sample(x, wav, noise=noise)
        roll = roll.cpu()
        d = maxdiff(roll, ref)
        assert d <= ATOL_STEP, (precision, d)
        assert bool((((roll > 0.5) == (ref > 0.5)) | near).all()), precision


# --------------------------------------------------------------------------------------------
# size-independent properties at BASELINE config 2 shape (B=16, T=125, k=9, 200 steps)
# --------------------------------------------------------------------------------------------
def test_full_chain_graph_equals_eager_and_is_deterministic(full_model):
    hp, p, m = full_model
    wav, x, noise = cfg2_inputs()
    a, _ = m.sample(x, wav, noise=noise, use_graph=True)
    b, _ = m.sample(x, wav, noise=noise, use_graph=False)
    c, _ = m.sample(x, wav, noise=noise, use_graph=True)
    assert torch.equal(a, b)
    assert torch.equal(a, c)
    assert bool(torch.isfinite(a).all())


def test_batch_shard_invariance_injected_and_philox(full_model):
    """Each sample's chain is independent: running the two halves of the batch separately
    gives the same rolls - with injected noise and with Philox keyed by the global sample index.  A
    smaller shard may be contracted in a different order (split-K / tile flavour are chosen per launch
    geometry), so across DIFFERENT local batch sizes the agreement is fp32 round-off, not bitwise; the
    bitwise statement for a fixed contraction order is test_batch_shard_bitwise_without_splitk."""
    hp, p, m = full_model
    wav, x, noise = cfg2_inputs(B=8)
    full, _ = m.sample(x, wav, noise=noise)
    lo, _ = m.sample(x[:4], wav[:4], noise=noise[:, :4])
    hi, _ = m.sample(x[4:], wav[4:], noise=noise[:, 4:])
    assert maxdiff(full.cpu(), torch.cat([lo, hi], 0).cpu()) <= ATOL_SHARD
    full, _ = m.sample(x, wav, seed=7)
    lo, _ = m.sample(x[:4], wav[:4], seed=7, first_sample=0)
    hi, _ = m.sample(x[4:], wav[4:], seed=7, first_sample=4)
    assert maxdiff(full.cpu(), torch.cat([lo, hi], 0).cpu()) <= ATOL_SHARD
    hi2, _ = m.sample(x[4:], wav[4:], seed=7, first_sample=4)
    assert torch.equal(hi, hi2)                      # same geometry: bitwise reproducible
    other, _ = m.sample(x, wav, seed=8)
    assert not torch.equal(full, other)


def test_batch_shard_bitwise_without_splitk():
    """With the contraction order pinned (split-K off: option tune.ksplit_max = 1, process-wide, hence the
    child process) sharding the batch changes nothing, bit for bit."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        sys.path.insert(0, %r)
        from tools import tuning_env; tuning_env.install()
        from oracle import diffroll_ref as R
        from tests.testlib import make_model, cfg2_inputs
        hp = dict(R.DEFAULT_HP); hp.update(kernel_size=9, timesteps=20)
        m = make_model(hp, R.synthetic_params(hp, seed=3), sampler="cfdg_ddpm_x0", w=0.5)
        wav, x, noise = cfg2_inputs(B=8, steps=20)
        full, _ = m.sample(x, wav, noise=noise)
        lo, _ = m.sample(x[:4], wav[:4], noise=noise[:, :4]); hi, _ = m.sample(x[4:], wav[4:], noise=noise[:, 4:])
        ok = torch.equal(full, torch.cat([lo, hi], 0))
        full, _ = m.sample(x, wav, seed=7)
        lo, _ = m.sample(x[:4], wav[:4], seed=7, first_sample=0); hi, _ = m.sample(x[4:], wav[4:], seed=7, first_sample=4)
        ok = ok and torch.equal(full, torch.cat([lo, hi], 0))
        print("BITWISE", int(ok))
    """ % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import tuning_env
    r = subprocess.run([sys.executable, "-c", code], env=tuning_env.env_with(tune__ksplit_max=1), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().endswith("BITWISE 1"), r.stdout[-500:]


def test_sample_trajectory_matches_chain(golden_dir):
    """sample_trajectory (every intermediate roll, the reference's noise_list of task/diffusion.py:779-788, kept
    on the device) ends bit for bit where the captured chain ends - with injected noise and with Philox - and
    its rows are the successive reverse steps."""
    g = load(golden_dir, "steps_chain_k9")
    hp, p, m = fixture_model(g, sampler="cfdg_ddpm_x0", w=float(g["w"]))
    x, wav, noise = T(g["x"]), T(g["wav"]), T(g["noise"])
    traj, _ = m.sample_trajectory(x, wav, noise=noise)
    roll, _ = m.sample(x, wav, noise=noise)
    S = hp["timesteps"]
    assert traj.shape == (S,) + tuple(roll.shape) and torch.equal(traj[-1], roll)
    assert maxdiff(traj[-1].cpu(), T(g["cfdg_ddpm_x0_chain"])) <= ATOL_STEP
    assert maxdiff(traj[0].cpu(), T(g[f"cfdg_ddpm_x0_t{S - 1}"])) <= ATOL_STEP      # first row = the step from x_T
    traj, _ = m.sample_trajectory(x, wav, seed=11, first_sample=3)
    roll, _ = m.sample(x, wav, seed=11, first_sample=3)
    assert torch.equal(traj[-1], roll)


def test_load_from_checkpoint_end_to_end(tmp_path):
    """A Lightning-shaped checkpoint ({'state_dict', 'hyper_parameters'} incl. the mel buffers and the
    non-persistent embedding a real one may carry) -> load_from_checkpoint(path, **overrides) (sampling.py:54-65)
    -> the same roll as a model built directly; the k=9 override of README.md:39 goes through the kwargs."""
    from diffroll_amd import ClassifierFreeDiffRoll
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=64, residual_layers=3, kernel_size=9, timesteps=6)
    p = R.synthetic_params(hp, seed=77)
    sd = dict(p)
    # the MelSpectrogram buffers a real checkpoint carries ARE used as the front-end tables (as load_state_dict would
    # load them into mel_layer in the reference): here torchaudio's own values
    from diffroll_amd.frontend_tables import frontend_tables
    sd["mel_layer.spectrogram.window"], _, sd["mel_layer.mel_scale.fb"] = frontend_tables(2048, 0.0, 8000.0, 229, 16000)
    hyper = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=229, norm_args=[0, 1, "imagewise"],
                 residual_layers=3, kernel_size=3, dilation_base=2, dilation_bound=4, spec_dropout=0.1,
                 spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000, center=True,
                                normalized=True, pad_mode="reflect"),
                 lr=1e-4, timesteps=6, loss_type="l2", loss_keys=["diffusion_loss"], beta_start=1e-4, beta_end=0.02,
                 frame_threshold=0.5, training={"mode": "x_0"}, sampling={"type": "ddpm_x0"}, debug=False,
                 generation_filter=0.02, inpainting_t=None, inpainting_f=None)
    path = tmp_path / "model.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": hyper, "epoch": 3, "pytorch-lightning_version": "1.6.4"}, path)
    m = ClassifierFreeDiffRoll.load_from_checkpoint(str(path), kernel_size=9, sampling={"type": "cfdg_ddpm_x0", "w": 0.5})
    assert m.hparams.kernel_size == 9 and m.hparams.sampling.type == "cfdg_ddpm_x0"
    ref = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    torch.manual_seed(1)
    wav = 0.1 * torch.randn(2, 40 * 512)
    x = torch.randn(2, 1, 40, 88)
    nz = torch.randn(6, 2, 1, 40, 88)
    a, _ = m.sample(x, wav, noise=nz)
    b, _ = ref.sample(x, wav, noise=nz)
    assert torch.equal(a, b)
    # ... and a checkpoint whose filterbank buffer differs (here: scaled) changes the spectrogram accordingly
    sd2 = dict(sd)
    sd2["mel_layer.mel_scale.fb"] = 4.0 * sd["mel_layer.mel_scale.fb"]
    m.load_state_dict(sd2, strict=False)
    _, spec_scaled = m(x, wav, torch.tensor([3, 3]))
    _, spec_ref = ref(x, wav, torch.tensor([3, 3]))
    assert float((spec_scaled - spec_ref).abs().max()) > 1e-3      # log(4 m + 1e-6) is not a pure shift of log(m + 1e-6)


def test_cli_drivers_end_to_end(tmp_path):
    """The sampling.py / infer.py command surface (diffroll_amd/cli.py) on the GPU: wav folder in (Custom dataset,
    utils/custom_dataset.py:55-91), rolls + raw / clean MIDI out, for the three tasks' samplers - and the written rolls
    are held to the ORACLE: its chain on the waveforms as the driver ingested them (stereo 22.05 kHz int16 -> mono ->
    windowed-sinc resampling -> crop / pad), from the same x_T, with the driver's Philox noise replayed on the CPU
    (oracle/philox.py, pinned by the Random123 known-answer vectors), the same weights (the driver's seeded draw)."""
    import scipy.io.wavfile as wavfile
    from diffroll_amd import cli, midi
    from oracle import philox
    wav_dir = tmp_path / "audio"
    wav_dir.mkdir()
    rng = np.random.default_rng(0)
    for i in range(3):
        n = 16000 * 2 + 700 * i                                   # ragged lengths, 22.05 kHz stereo -> resample + mono-mix
        data = (rng.standard_normal((int(n * 22050 / 16000), 2)) * 3000).astype(np.int16)
        wavfile.write(str(wav_dir / f"clip{i}.wav"), 22050, data)
    common = ["model.args.kernel_size=3", "model.args.residual_channels=64", "model.args.residual_layers=3",
              "task.timesteps=6", "dataloader.batch_size=2"]
    dev = torch.device("cuda", 0)

    def oracle_rolls(argv, model_seed):
        """What the driver must have written: per batch, the oracle chain with replayed Philox noise."""
        cfg = cli.build_config(argv)
        torch.manual_seed(model_seed)
        m = cli.make_model(cfg, dev)                                # the same weights the driver drew
        p = {k: v.detach().cpu().float() for k, v in m.state_dict().items()}
        a = cfg["model"]["args"]
        hp = dict(R.DEFAULT_HP)
        hp.update(residual_channels=a["residual_channels"], residual_layers=a["residual_layers"], kernel_size=a["kernel_size"],
                  timesteps=cfg["task"]["timesteps"])
        sampler = cfg["task"]["sampling"]["type"]
        g = torch.Generator().manual_seed(int(cfg["seed"]))
        S, hop = int(cfg["dataset"]["num_samples"]), int(cfg["hop_length"])
        if cfg["dataset"]["name"] == "Custom":
            wav = cli.load_wav_folder(cfg["dataset"]["args"])
            S = min(S, wav.shape[0])
            wav = wav[:S]
            T = wav.shape[1] // hop
        elif cfg["dataset"]["name"] == "Synthetic":
            wav = 0.1 * torch.randn(S, int(cfg["sequence_length"]), generator=g)
            T = int(cfg["sequence_length"]) // hop
        else:
            wav = torch.zeros(S, int(cfg["sequence_length"]))
            T = int(cfg["sequence_length"]) // hop
        x = torch.randn(S, 1, T, 88, generator=g)
        bs = min(int(cfg["dataloader"]["batch_size"]), S)
        out = []
        for bi, lo in enumerate(range(0, S, bs)):
            hi = min(lo + bs, S)
            z = philox.chain_noise(int(cfg["seed"]) + bi, 0, hp["timesteps"], hi - lo, T)
            with torch.no_grad():
                out.append(R.sample_chain(p, hp, sampler, x[lo:hi], wav[lo:hi], z, w=0.5,
                                          inpainting_t=cfg["task"]["inpainting_t"] if sampler == "inpainting_ddpm_x0" else None))
        return out

    out = tmp_path / "o_tr"
    argv = ["task=transcription", "dataset=Custom", f"dataset.args.audio_path={wav_dir}", "dataset.args.audio_ext=wav",
            "dataset.args.max_segment_samples=32000", f"output_dir={out}"] + common
    torch.manual_seed(71)
    cli.main(argv)
    rolls = np.load(out / "rolls_batch0.npy")
    assert rolls.shape == (2, 1, 32000 // 512, 88) and np.isfinite(rolls).all()
    assert (out / "rolls_batch1.npy").exists()                   # 3 clips, batch 2 -> a ragged last batch
    assert (out / "raw_midi_0_0.mid").exists() and (out / "clean_midi_e1_0.mid").exists()
    want = oracle_rolls(argv, 71)
    for bi, ref in enumerate(want):
        got = torch.from_numpy(np.load(out / f"rolls_batch{bi}.npy"))
        assert maxdiff(got, ref) <= ATOL_STEP, (bi, maxdiff(got, ref))
    # ... and the MIDI files are the notes of those rolls (extract_notes_wo_velocity at the 0.5 threshold)
    notes = midi.read_midi_notes(str(out / "raw_midi_0_1.mid"))
    ref_notes = R.extract_notes_wo_velocity(want[0][1, 0].numpy(), want[0][1, 0].numpy())
    assert len([e for e in notes if (e[1] & 0xF0) == 0x90 and e[3] > 0]) == len(ref_notes[0])
    out = tmp_path / "o_gen"
    argv = ["task=generation", "dataset.num_samples=2", "sequence_length=16384", f"output_dir={out}"] + common
    torch.manual_seed(72)
    cli.main(argv)
    got = torch.from_numpy(np.load(out / "rolls_batch0.npy"))
    assert got.shape == (2, 1, 32, 88)
    assert maxdiff(got, oracle_rolls(argv, 72)[0]) <= ATOL_STEP
    out = tmp_path / "o_inp"
    argv = ["task=inpainting", "task.inpainting_t=[4,12]", "dataset=Synthetic", "dataset.num_samples=2",
            "sequence_length=16384", f"output_dir={out}"] + common
    torch.manual_seed(73)
    cli.main(argv)
    got = torch.from_numpy(np.load(out / "rolls_batch0.npy"))
    assert maxdiff(got, oracle_rolls(argv, 73)[0]) <= ATOL_STEP


def test_device_philox_noise_equals_the_cpu_replay():
    """The production noise (on-device Philox4x32-10 keyed by (seed, global sample, step) + Box-Muller,
    task/diffusion.py:967's role) against its numpy restatement: a seeded chain on the GPU equals the oracle chain fed
    the replayed z's, also for a shard that starts at a global offset (first_sample)."""
    from oracle import philox
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=64, residual_layers=3, kernel_size=9, timesteps=8)
    p = R.synthetic_params(hp, seed=21)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    g = torch.Generator().manual_seed(2)
    B, Tn = 3, 50
    wav = 0.1 * torch.randn(B, Tn * 512, generator=g)
    x = torch.randn(B, 1, Tn, 88, generator=g)
    for seed, first in ((0, 0), (0x1234567890ABCDEF, 5)):
        got, _ = m.sample(x, wav, seed=seed, first_sample=first)
        z = philox.chain_noise(seed, first, 8, B, Tn)
        with torch.no_grad():
            ref = R.sample_chain(p, hp, "cfdg_ddpm_x0", x, wav, z, w=0.5)
        assert maxdiff(got.cpu(), ref) <= ATOL_STEP, (seed, first, maxdiff(got.cpu(), ref))


def test_odd_channel_padding_at_filled_launches():
    """C = 160 pads to 192 channels = 3 row tiles, so the residual / skip halves of the 1x1 do not fall on tile
    boundaries; a batch large enough for the direct-operand 1x1 (incl. the last layer's skip-only launch)."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=160, residual_layers=3, kernel_size=9, timesteps=6)
    p = R.synthetic_params(hp, seed=160)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    torch.manual_seed(16)
    B, Tn = 40, 125            # 80 evaluations: enough tiles for the skip-only launch of the last layer to be taken
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    z = torch.randn(B, 1, Tn, 88)
    sch = R.schedule(hp["beta_start"], hp["beta_end"], 6)
    with torch.no_grad():
        ref = R.reverse_step(p, hp, sch, "cfdg_ddpm_x0", x, R.frontend(wav, hp, Tn), 3, z, 0.5)
    out, _ = m.reverse_diffusion(x, wav, 3, noise=z)
    assert maxdiff(out.cpu(), ref) <= ATOL_STEP, maxdiff(out.cpu(), ref)


def test_large_batch_self_consistency(full_model):
    """Far beyond the oracle's reach (96 clips x 640 frames, k=9, guided: 192 evaluations per step, 1280-block
    launches): every clip of the big batch equals the same clip run in a batch of four (independent units,
    Philox keyed by the global index) to fp32 round-off, and everything is finite."""
    hp, p, _ = full_model
    hp3 = dict(hp)
    hp3["timesteps"] = 3
    m = make_model(hp3, p, sampler="cfdg_ddpm_x0", w=0.5)
    g = torch.Generator().manual_seed(0)
    B, Tn = 96, 640
    wav = 0.1 * torch.randn(B, Tn * 512, generator=g)
    x = torch.randn(B, 1, Tn, 88, generator=g)
    big, _ = m.sample(x, wav, seed=5)
    assert bool(torch.isfinite(big).all())
    for lo in (0, 40, 92):
        small, _ = m.sample(x[lo:lo + 4], wav[lo:lo + 4], seed=5, first_sample=lo)
        assert maxdiff(big[lo:lo + 4].cpu(), small.cpu()) <= ATOL_SHARD


def test_cfg_weight_zero_equals_conditional_sampler(full_model):
    """(1+w) c - w u with w = 0 is c: cfdg_ddpm_x0(w=0) == ddpm_x0 (task/diffusion.py:953).  The two run with
    different batch geometry (2B vs B evaluations), i.e. possibly different contraction orders: round-off."""
    hp, p, _ = full_model
    wav, x, noise = cfg2_inputs(B=2, steps=200)
    m0 = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.0)
    m1 = make_model(hp, p, sampler="ddpm_x0")
    a, _ = m0.sample(x, wav, noise=noise)
    b, _ = m1.sample(x, wav, noise=noise)
    assert maxdiff(a.cpu(), b.cpu()) <= ATOL_SHARD


def test_philox_noise_is_standard_normal(full_model):
    """One generation step from x = 0, x0-independent part: the injected term is sigma * z."""
    hp, p, m = full_model
    from diffroll_amd import _cabi  # noqa: F401
    eng = m.engine
    B, Tn = 4, 125
    t = 150
    x = torch.zeros(B, Tn, 88, device=eng.device)
    xz = x.clone()
    zero = torch.zeros_like(x)
    eng.step("generation_ddpm_x0", xz, zero, t)           # deterministic part
    xp = x.clone()
    eng.step("generation_ddpm_x0", xp, None, t, seed=123)  # + sigma * z
    sch = eng.schedule
    s1m = sch["sqrt_one_minus_alphas_cumprod"]
    sigma = float((s1m[t - 1] / s1m[t]) * torch.sqrt(1 - sch["alphas"][t]))
    z = ((xp - xz) / sigma).cpu().double().flatten()
    assert abs(float(z.mean())) < 0.02
    assert abs(float(z.std()) - 1.0) < 0.02
    assert abs(float((z ** 3).mean())) < 0.05
    assert abs(float((z ** 4).mean()) - 3.0) < 0.15


def test_frame_f1_matches_sklearn(full_model):
    """frame P/R/F1 of test_step (task/diffusion.py:381-383) = sklearn's binary
    precision_recall_fscore_support on the thresholded roll; counts are integer-exact."""
    from sklearn.metrics import precision_recall_fscore_support
    hp, p, m = full_model
    torch.manual_seed(3)
    B, Tn = 5, 125
    pred = torch.rand(B, 1, Tn, 88) * 1.4 - 0.2
    label = (torch.rand(B, Tn, 88) > 0.9).float()
    for thr in (0.5, 0.8):
        tp, fp, fn = m.engine.frame_counts(pred[:, 0], label, thr)
        pb = (pred.flatten() > thr).numpy()
        lb = label.flatten().numpy()
        assert tp == int((pb & (lb > 0.5)).sum()) and fp == int((pb & ~(lb > 0.5)).sum())
        assert fn == int((~pb & (lb > 0.5)).sum())
        sp, sr, sf, _ = precision_recall_fscore_support(lb, pb, average="binary")
        mp, mr, mf = m.frame_metrics(tp, fp, fn)
        assert abs(mp - sp) < 1e-12 and abs(mr - sr) < 1e-12 and abs(mf - sf) < 1e-12
    assert m.frame_metrics(0, 0, 0) == (0.0, 0.0, 0.0)
    # end to end: test_step on a batch (label normalisation is irrelevant for the metric)
    m2 = make_model(hp, p, sampler="ddim_x0")
    wav = 0.1 * torch.randn(2, 64000)
    out = m2.test_step({"frame": label[:2], "audio": wav}, 0)
    assert 0.0 <= out["Test/Frame_F1"] <= 1.0 and out["tp"] + out["fn"] == int(label[:2].sum())
    assert 0.0 <= out["Test/Note_F1"] <= 1.0 and len(out["note_scores"]) == 2
    # note-level score (task/diffusion.py:385-410): a prediction equal to the label scores 1, one shifted by a
    # frame (32 ms <= the 50 ms onset tolerance) still 1, shifted by two frames 0
    from diffroll_amd import midi, metrics
    lab = torch.zeros(1, Tn, 88)
    lab[0, 10:20, 40] = 1.0
    lab[0, 30:33, 52] = 1.0
    lab[0, 60:90, 12] = 1.0
    ref = midi.extract_notes_wo_velocity(m.engine, lab.cuda(), 0.5)
    for shift, want in ((0, 1.0), (1, 1.0), (2, 0.0)):
        est = midi.extract_notes_wo_velocity(m.engine, torch.roll(lab, shift, dims=1).cuda(), 0.5)
        assert metrics.note_scores(ref, est, 512, 16000)[0][2] == want


# --------------------------------------------------------------------------------------------
# opt-in split-bf16 precision (DR_PRECISION_BF16X3): held to the SAME tolerances as the exact-fp32 path
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["forward_k3", "forward_k9", "forward_k15", "forward_wide_k9"])
def test_bf16x3_forward_golden(golden_dir, name):
    g = load(golden_dir, name)
    hp, p, m = fixture_model(g, precision="bf16x3")
    x, wav = T(g["x"]), T(g["wav"])
    t = torch.tensor(int(g["t"])).repeat(x.shape[0])
    x0_c, _ = m(x, wav, t)
    x0_u, _ = m(x, torch.zeros_like(wav), t, sampling=True)
    assert m.engine.precision == "bf16x3"
    assert maxdiff(x0_c.cpu(), g["x0_c"]) <= ATOL_FWD, maxdiff(x0_c.cpu(), g["x0_c"])
    assert maxdiff(x0_u.cpu(), g["x0_u"]) <= ATOL_FWD, maxdiff(x0_u.cpu(), g["x0_u"])


@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "generation_ddpm_x0"])
def test_bf16x3_chain_golden(golden_dir, sampler):
    g = load(golden_dir, "steps_chain_k9")
    hp, p, m = fixture_model(g, sampler=sampler, w=float(g["w"]), precision="bf16x3")
    x, wav, noise = T(g["x"]), T(g["wav"]), T(g["noise"])
    for use_graph in (False, True):
        roll, _ = m.sample(x, wav, noise=noise, use_graph=use_graph)
        d = maxdiff(roll.cpu(), g[f"{sampler}_chain"])
        assert d <= ATOL_STEP, (use_graph, d)


def test_bf16x3_full_size_forward_and_config1_chain_vs_oracle():
    hp = dict(R.DEFAULT_HP)
    p = R.synthetic_params(hp, seed=0)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16x3")
    torch.manual_seed(0)
    B, L = 2, 64000
    Tn = L // 512
    wav = 0.1 * torch.randn(B, L)
    x = torch.randn(B, 1, Tn, 88)
    t = torch.tensor(117).repeat(B)
    with torch.no_grad():
        ref_c, _ = R.forward(p, hp, x, wav, t)
        ref_u, _ = R.forward(p, hp, x, torch.zeros_like(wav), t, sampling=True)
    x0_c, _ = m(x, wav, t)
    x0_u, _ = m(x, wav, t, sampling=True)
    dc, du = maxdiff(x0_c.cpu(), ref_c), maxdiff(x0_u.cpu(), ref_u)
    assert dc <= ATOL_FWD and du <= ATOL_FWD, (dc, du)
    # exact-fp32 engine on the same inputs: the two precisions agree far inside the tolerance
    m32 = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    y32, _ = m32(x, wav, t)
    assert maxdiff(x0_c.cpu(), y32.cpu()) <= ATOL_FWD
    # config 1 chain (50 steps)
    hp1 = dict(hp)
    hp1["timesteps"] = 50
    m1 = make_model(hp1, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16x3")
    wav1, x1 = wav[:1], x[:1]
    noise = torch.randn(50, 1, 1, Tn, 88)
    with torch.no_grad():
        ref = R.sample_chain(p, hp1, "cfdg_ddpm_x0", x1, wav1, noise, w=0.5)
    roll, _ = m1.sample(x1, wav1, noise=noise)
    d = maxdiff(roll.cpu(), ref)
    assert d <= ATOL_STEP, d


def test_note_extraction_bit_exact_and_midi(golden_dir, full_model, tmp_path):
    """GPU note scan == the reference's extract_notes_wo_velocity (integer work: bit exact),
    then MIDI export round trip."""
    from diffroll_amd import midi
    hp, p, m = full_model
    g = load(golden_dir, "notes")
    eng = m.engine
    for i in range(int(g["n"])):
        roll = T(g[f"roll{i}"])[None]
        for thr in (0.5, 0.8):
            (pitches, intervals), = midi.extract_notes_wo_velocity(eng, roll, thr)
            assert np.array_equal(pitches, g[f"pitches{i}_{thr}"]), (i, thr)
            assert np.array_equal(intervals, g[f"intervals{i}_{thr}"]), (i, thr)
            op, oi = R.extract_notes_wo_velocity(g[f"roll{i}"], g[f"roll{i}"], thr, thr)
            assert np.array_equal(pitches, np.asarray(op, dtype=np.int64))
    # batched call + export
    rolls = torch.stack([T(g["roll0"]), T(g["roll0"]).flip(1)])[:, None]
    paths = midi.export_midi(eng, rolls, str(tmp_path / "raw_midi_"), threshold=0.5, generation_filter=0.1,
                             clean_prefix=str(tmp_path / "clean_midi_e0_"))
    assert len(paths) == 2
    clean = midi.read_midi_notes(str(tmp_path / "clean_midi_e0_0.mid"))
    iv0 = g["intervals0_0.5"].reshape(-1, 2)
    n_long = int(((iv0[:, 1] - iv0[:, 0]) * (512 / 16000) > 0.1).sum())
    assert sum(1 for e in clean if e[1] == 0x90) == n_long       # the clean file drops the short notes only
    ev = midi.read_midi_notes(paths[0])
    n_notes = len(g["pitches0_0.5"])
    assert len(ev) == 2 * n_notes and sum(1 for e in ev if e[1] == 0x90) == n_notes
    assert all(midi.MIN_MIDI <= e[2] <= 108 for e in ev) and all(b[0] >= a[0] for a, b in zip(ev, ev[1:]))


# --------------------------------------------------------------------------------------------
# edge cases: ragged frame counts (T = 1, below the halo, around the 64/128-frame tile sizes), B = 1,
# all kernel sizes, every dilation, both precisions - one evaluation + one guided step vs the oracle
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 9, 15])
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_ragged_shapes_vs_oracle(k, precision):
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=64, residual_layers=4, kernel_size=k, timesteps=6)   # dilations 1,2,4,8
    p = R.synthetic_params(hp, seed=900 + k)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.7, precision=precision)
    sch = R.schedule(hp["beta_start"], hp["beta_end"], hp["timesteps"])
    g = torch.Generator().manual_seed(k)
    for B, Tn in ((1, 1), (2, 7), (1, 63), (3, 64), (1, 65), (2, 129), (1, 200)):
        L = max(Tn * 512, 2048)                      # reflect padding needs L > n_fft / 2
        wav = 0.1 * torch.randn(B, L, generator=g)
        x = torch.randn(B, 1, Tn, 88, generator=g)
        z = torch.randn(B, 1, Tn, 88, generator=g)
        t = torch.tensor(3).repeat(B)
        with torch.no_grad():
            ref, ref_spec = R.forward(p, hp, x, wav, t)
            spec_c = R.frontend(wav, hp, Tn)
            ref_step = R.reverse_step(p, hp, sch, "cfdg_ddpm_x0", x, spec_c, 3, z, 0.7)
        out, spec = m(x, wav, t)
        assert out.shape == ref.shape and spec.shape == ref_spec.shape
        d = maxdiff(out.cpu(), ref)
        assert d <= ATOL_FWD, (B, Tn, d)
        assert maxdiff(spec.cpu(), ref_spec) <= ATOL_SPEC
        step, _ = m.reverse_diffusion(x, wav, 3, noise=z)
        d = maxdiff(step.cpu(), ref_step)
        assert d <= ATOL_STEP, (B, Tn, d)


def test_random_configurations_vs_oracle():
    """Randomised (fixed seed) sweep over what the launch heuristics key on: channel counts incl. ones that need
    padding, depth, every odd kernel size 3..15, dilation base / bound (dilations up to 27), batch, ragged frame
    counts, all nine samplers, guidance weight, both precisions - one reverse step each against the oracle."""
    rng = np.random.default_rng(2024)
    samplers = ["ddpm_x0", "cfdg_ddpm_x0", "generation_ddpm_x0", "inpainting_ddpm_x0", "ddim_x0", "cfdg_ddim_x0",
                "ddpm", "ddim", "ddim2ddpm"]
    for case in range(150):
        hp = dict(R.DEFAULT_HP)
        hp.update(residual_channels=int(rng.choice([32, 64, 96, 128, 160])), residual_layers=int(rng.integers(1, 6)),
                  kernel_size=int(rng.choice([3, 5, 7, 9, 11, 13, 15])), dilation_base=int(rng.choice([1, 2, 3])),
                  dilation_bound=int(rng.integers(1, 5)), timesteps=int(rng.integers(2, 12)))
        sampler = samplers[case % 9]
        w = float(rng.choice([0.0, 0.5, 1.3]))
        B, Tn = int(rng.integers(1, 6)), int(rng.integers(1, 300))
        if case % 6 == 5:                 # every sixth case fills the chip: the large-launch kernel flavours
            B, Tn = int(rng.choice([24, 40])), int(rng.choice([64, 125, 160]))
        precision = "bf16x3" if case % 4 == 3 else "f32"
        it = [Tn // 4, max(Tn // 2, Tn // 4 + 1)] if sampler == "inpainting_ddpm_x0" else None
        p = R.synthetic_params(hp, seed=3000 + case)
        m = make_model(hp, p, sampler=sampler, w=w, inpainting_t=it, precision=precision)
        sch = R.schedule(hp["beta_start"], hp["beta_end"], hp["timesteps"])
        g = torch.Generator().manual_seed(case)
        wav = 0.1 * torch.randn(B, max(Tn * 512, 2048), generator=g)
        x = torch.randn(B, 1, Tn, 88, generator=g)
        z = torch.randn(B, 1, Tn, 88, generator=g)
        t = int(rng.integers(0, hp["timesteps"]))
        with torch.no_grad():
            spec = None if sampler == "generation_ddpm_x0" else R.frontend(wav, hp, Tn, inpainting_t=it)
            ref = R.reverse_step(p, hp, sch, sampler, x, spec, t, z, w)
        out, _ = m.reverse_diffusion(x, wav, t, noise=z)
        d = maxdiff(out.cpu(), ref)
        assert d <= ATOL_STEP, (case, hp, sampler, w, B, Tn, t, precision, d)


def test_random_full_width_geometries_vs_oracle():
    """Full width (C = 512) with random launch geometries - the tile / split-K / direct-1x1 / dual-epilogue choices
    are all made from (samples, frames): a shallow net keeps the oracle quick; one guided step per case."""
    rng = np.random.default_rng(512)
    for case in range(24):
        hp = dict(R.DEFAULT_HP)
        hp.update(residual_layers=int(rng.integers(2, 5)), kernel_size=int(rng.choice([9, 15])), timesteps=4)
        Tn = int(rng.choice([1, 33, 64, 65, 96, 125, 127, 128, 129, 160, 200, 256, 333, 640]))
        B = int(max(1, min(rng.integers(1, 33), 6000 // Tn)))
        sampler = ["cfdg_ddpm_x0", "generation_ddpm_x0", "ddpm_x0"][case % 3]
        precision = "bf16x3" if case % 4 == 3 else "f32"
        p = R.synthetic_params(hp, seed=7000 + case)
        m = make_model(hp, p, sampler=sampler, w=0.5, precision=precision)
        sch = R.schedule(hp["beta_start"], hp["beta_end"], 4)
        g = torch.Generator().manual_seed(case)
        wav = 0.1 * torch.randn(B, max(Tn * 512, 2048), generator=g)
        x = torch.randn(B, 1, Tn, 88, generator=g)
        z = torch.randn(B, 1, Tn, 88, generator=g)
        with torch.no_grad():
            spec = None if sampler == "generation_ddpm_x0" else R.frontend(wav, hp, Tn)
            ref = R.reverse_step(p, hp, sch, sampler, x, spec, 2, z, 0.5)
        out, _ = m.reverse_diffusion(x, wav, 2, noise=z)
        d = maxdiff(out.cpu(), ref)
        assert d <= ATOL_STEP, (case, hp["residual_layers"], hp["kernel_size"], sampler, B, Tn, precision, d)


@pytest.mark.gpu
def test_640_frame_family_picks_the_160_frame_stack_and_matches_the_oracle():
    """Round 6: the planner's NATURAL choice at the 640-frame geometries is the fused residual stack on 160-frame blocks
    (stack_kernel<5>): one resident round at 8 evaluations, balanced chunks beyond, nothing fused where a launch would leave
    the chip part-filled.  One step and a short captured chain per case against the oracle, full width, k = 9 and 15; the
    launch mode the engine reports is asserted where the geometry decides it."""
    from tools import tuning_env
    natural = not (tuning_env.is_forced("fused_stack") or tuning_env.is_forced("tune.stack_fl") or tuning_env.is_forced("fused_tail")
                   or tuning_env.is_forced("blocked_accumulation"))
    cases = [  # B, T, k, sampler, expected kernel prefix / mode under default options (None: not asserted)
        (4, 640, 9, "cfdg_ddpm_x0", "stack_kernel<5>", "fused_stack+tail"),        # the reference's shipping geometry
        (4, 640, 15, "cfdg_ddpm_x0", "stack_kernel<5>", "fused_stack+tail"),       # BASELINE config 5 per GPU
        (8, 640, 9, "generation_ddpm_x0", "stack_kernel<5>", "fused_stack+tail"),  # 8 evaluations, one per clip
        (16, 640, 9, "generation_ddpm_x0", "stack_kernel<5>", "fused_stack"),      # two chunks of 8: no tail kernel
        (4, 600, 9, "cfdg_ddpm_x0", "stack_kernel<5>", "fused_stack+tail"),        # ragged last tile (120 of 160 frames)
        (2, 640, 9, "cfdg_ddpm_x0", None, None),                                   # half the chip: the planner's split-K territory
        (3, 800, 9, "ddpm_x0", None, None),                                        # 5 tiles per clip
    ]
    for (B, Tn, k, sampler, want_kernel, want_mode) in cases:
        hp = dict(R.DEFAULT_HP)
        hp.update(residual_layers=2, kernel_size=k, timesteps=4)
        p = R.synthetic_params(hp, seed=640 + B + k)
        m = make_model(hp, p, sampler=sampler, w=0.5)
        sch = R.schedule(hp["beta_start"], hp["beta_end"], 4)
        g = torch.Generator().manual_seed(B * 31 + Tn)
        wav = 0.1 * torch.randn(B, Tn * 512, generator=g)
        x = torch.randn(B, 1, Tn, 88, generator=g)
        nz = torch.randn(4, B, 1, Tn, 88, generator=g)
        with torch.no_grad():
            spec = None if sampler == "generation_ddpm_x0" else R.frontend(wav, hp, Tn)
            ref = R.reverse_step(p, hp, sch, sampler, x, spec, 2, nz[0], 0.5)
            ref_chain = R.sample_chain(p, hp, sampler, x, None if sampler == "generation_ddpm_x0" else wav, nz, w=0.5)
        eng = m.engine
        eng.profile_enable(True)
        out, _ = m.reverse_diffusion(x, wav, 2, noise=nz[0])
        _, _, _, kname = eng.profile_read_ex()
        eng.profile_enable(False)
        d = maxdiff(out.cpu(), ref)
        assert d <= ATOL_STEP, (B, Tn, k, sampler, d)
        roll, _ = m.sample(x, wav, noise=nz)
        d = maxdiff(roll.cpu(), ref_chain)
        assert d <= ATOL_STEP, ("chain", B, Tn, k, sampler, d)
        st = eng.launch_state()
        assert st["fallbacks"] == 0 and st["yields"] == 0, st
        if natural and want_kernel:
            assert kname.startswith(want_kernel), (B, Tn, k, sampler, kname)
            assert st["mode"] == want_mode, (B, Tn, k, sampler, st)
        del m


def test_random_chains_vs_oracle():
    """Randomised (fixed seed) whole chains through dr_sample (captured graph) against the oracle's loop: random
    depth / width / kernel size / schedule length, the four x0-prediction samplers and the DDIM / epsilon ones,
    both conditioning modes ('fixed', 'trainable_spec'), both spectrogram normalisations, inpainting masks in time
    and frequency, Tn from 1 frame up, both precisions."""
    from diffroll_amd import ClassifierFreeDiffRoll
    rng = np.random.default_rng(77)
    samplers = ["cfdg_ddpm_x0", "generation_ddpm_x0", "inpainting_ddpm_x0", "ddpm_x0", "ddim_x0", "cfdg_ddim_x0", "ddpm",
                "ddim", "ddim2ddpm"]
    for case in range(120):
        hp = dict(R.DEFAULT_HP)
        hp.update(residual_channels=int(rng.choice([32, 64, 96, 128])), residual_layers=int(rng.integers(1, 5)),
                  kernel_size=int(rng.choice([3, 5, 9, 15])), timesteps=int(rng.integers(2, 7)),
                  condition=str(rng.choice(["fixed", "trainable_spec"])), norm_mode=str(rng.choice(["imagewise", "framewise"])))
        sampler = samplers[case % 9]
        w = float(rng.choice([0.0, 0.5, 2.0]))
        B, Tn = int(rng.integers(1, 5)), int(rng.integers(1, 200))
        it = [Tn // 3, max(2 * Tn // 3, Tn // 3 + 1)] if sampler == "inpainting_ddpm_x0" else None
        i_f = [20, 120] if (sampler == "inpainting_ddpm_x0" and case % 2) else None
        p = R.synthetic_params(hp, seed=5000 + case)
        m = ClassifierFreeDiffRoll(
            residual_channels=hp["residual_channels"], unconditional=False, condition=hp["condition"], n_mels=hp["n_mels"],
            norm_args=[0, 1, hp["norm_mode"]], residual_layers=hp["residual_layers"], kernel_size=hp["kernel_size"],
            dilation_base=hp["dilation_base"], dilation_bound=hp["dilation_bound"],
            spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=hp["n_mels"], f_min=0, f_max=8000,
                           normalized=True),
            inpainting_t=it, inpainting_f=i_f, timesteps=hp["timesteps"], training={"mode": "x_0"},
            sampling={"type": sampler, "w": w}, precision="bf16x3" if case % 5 == 4 else "f32")
        m.load_state_dict(p)
        g = torch.Generator().manual_seed(case)
        wav = 0.1 * torch.randn(B, max(Tn * 512, 2048), generator=g)
        x = torch.randn(B, 1, Tn, 88, generator=g)
        noise = torch.randn(hp["timesteps"], B, 1, Tn, 88, generator=g)
        with torch.no_grad():
            ref = R.sample_chain(p, hp, sampler, x, wav, noise, w=w, inpainting_t=it, inpainting_f=i_f)
        roll, _ = m.sample(x, wav, noise=noise)
        d = maxdiff(roll.cpu(), ref)
        assert d <= ATOL_STEP, (case, hp, sampler, w, B, Tn, d)


def test_forward_with_per_sample_steps_golden(golden_dir):
    """forward() with a (B,) step tensor whose entries differ (dr_forward_steps: the step-embedding row is
    selected per sample in the epilogues) against the reference run; also at full width vs the oracle."""
    g = np.load(os.path.join(golden_dir, "forward_steps.npz"))
    hp, p, m = fixture_model(g)
    x0_c, _ = m(T(g["x"]), T(g["wav"]), T(g["t"]))
    x0_u, _ = m(T(g["x"]), T(g["wav"]), T(g["t"]), sampling=True)
    assert maxdiff(x0_c.cpu(), T(g["x0_c"])) <= ATOL_FWD
    assert maxdiff(x0_u.cpu(), T(g["x0_u"])) <= ATOL_FWD
    for precision in ("f32", "bf16x3"):
        hp2 = dict(R.DEFAULT_HP)
        hp2.update(residual_channels=128, residual_layers=4, kernel_size=9, timesteps=20)
        p2 = R.synthetic_params(hp2, seed=8)
        m2 = make_model(hp2, p2, precision=precision)
        torch.manual_seed(2)
        wav = 0.1 * torch.randn(5, 200 * 512)
        x = torch.randn(5, 1, 200, 88)
        t = torch.tensor([19, 3, 3, 0, 11])
        with torch.no_grad():
            ref, _ = R.forward(p2, hp2, x, wav, t)
        out, _ = m2(x, wav, t)
        assert maxdiff(out.cpu(), ref) <= ATOL_FWD, precision


def test_framewise_normalisation_golden(golden_dir):
    """norm_args[2] = 'framewise' (model/utils.py:11-19: per-frame min-max over the mel bins, NaN -> 0) vs the
    reference run on random, sine and silent clips, with and without an inpainting mask."""
    from diffroll_amd import ClassifierFreeDiffRoll
    g = np.load(os.path.join(golden_dir, "framewise.npz"))
    hp = json.loads(str(g["hp"]))
    p = R.synthetic_params(hp, seed=int(g["seed"]))
    kw = dict(residual_channels=hp["residual_channels"], unconditional=False, condition="fixed", n_mels=hp["n_mels"],
              norm_args=[0, 1, "framewise"], residual_layers=hp["residual_layers"], kernel_size=hp["kernel_size"],
              dilation_base=hp["dilation_base"], dilation_bound=hp["dilation_bound"],
              spec_args=dict(sample_rate=16000, n_fft=hp["n_fft"], hop_length=hp["hop_length"], n_mels=hp["n_mels"], f_min=0,
                             f_max=8000, normalized=True), timesteps=hp["timesteps"], training={"mode": "x_0"},
              sampling={"type": "cfdg_ddpm_x0", "w": 0.5})
    m = ClassifierFreeDiffRoll(**kw)
    m.load_state_dict(p)
    t = torch.tensor(3).repeat(4)
    x0, spec = m(T(g["x"]), T(g["wav"]), t)
    assert maxdiff(spec.cpu(), T(g["spec"])) <= ATOL_SPEC
    assert maxdiff(x0.cpu(), T(g["x0"])) <= ATOL_FWD
    _, spec_t = m(T(g["x"]), T(g["wav"]), t, inpainting_t=[4, 9])
    assert maxdiff(spec_t.cpu(), T(g["spec_t"])) <= ATOL_SPEC
    with pytest.raises(ValueError):
        ClassifierFreeDiffRoll(**{**kw, "norm_args": [0, 1, "freqwise"]})


def test_trainable_spec_condition_golden(golden_dir):
    """condition='trainable_spec' (model/diffwave.py:600-606, :656-658): the unconditional branch reads the learned
    (n_mels, 641) spectrogram through every layer's conditioner (hoisted like the clip's); forward(sampling=True),
    a guided step (incl. the shared first-layer contraction) and a generation step against the reference run."""
    from diffroll_amd import ClassifierFreeDiffRoll
    g = np.load(os.path.join(golden_dir, "trainable_spec.npz"))
    hp = json.loads(str(g["hp"]))
    p = R.synthetic_params(hp, seed=int(g["seed"]))

    def build(sampler, w):
        m = ClassifierFreeDiffRoll(
            residual_channels=hp["residual_channels"], unconditional=False, condition="trainable_spec", n_mels=hp["n_mels"],
            norm_args=[0, 1, "imagewise"], residual_layers=hp["residual_layers"], kernel_size=hp["kernel_size"],
            dilation_base=hp["dilation_base"], dilation_bound=hp["dilation_bound"],
            spec_args=dict(sample_rate=16000, n_fft=hp["n_fft"], hop_length=hp["hop_length"], n_mels=hp["n_mels"], f_min=0,
                           f_max=8000, normalized=True), timesteps=hp["timesteps"], training={"mode": "x_0"},
            sampling={"type": sampler, "w": w})
        m.load_state_dict(p)
        return m

    x, wav, z = T(g["x"]), T(g["wav"]), T(g["z"])
    t = torch.tensor(5).repeat(x.shape[0])
    m = build("cfdg_ddpm_x0", 0.5)
    x0_u, spec_u = m(x, torch.zeros_like(wav), t, sampling=True)
    assert spec_u.dim() == 2 and torch.equal(spec_u.cpu(), T(g["spec_u"]))
    assert maxdiff(x0_u.cpu(), T(g["x0_u"])) <= ATOL_FWD
    out, _ = m.reverse_diffusion(x, wav, 5, noise=z)
    assert maxdiff(out.cpu(), T(g["cfdg_t5"])) <= ATOL_STEP
    m = build("generation_ddpm_x0", 0.0)
    out, _ = m.reverse_diffusion(x, wav, 5, noise=z)
    assert maxdiff(out.cpu(), T(g["generation_t5"])) <= ATOL_STEP
    # the parameter can be re-loaded: a second commit rebuilds the hoisted tensors
    p2 = dict(p)
    p2["trainable_parameters"] = torch.full_like(p["trainable_parameters"], -1.0)     # == condition 'fixed'
    m.load_state_dict(p2)
    hp_f = dict(hp)
    hp_f["condition"] = "fixed"
    sch = R.schedule(hp["beta_start"], hp["beta_end"], hp["timesteps"])
    with torch.no_grad():
        ref = R.reverse_step(p, hp_f, sch, "generation_ddpm_x0", x, None, 5, z, 0.0)
    out, _ = m.reverse_diffusion(x, wav, 5, noise=z)
    assert maxdiff(out.cpu(), ref) <= ATOL_STEP


def test_cosine_beta_schedule_steps_vs_oracle(golden_dir):
    """beta_schedule='cosine' (model/unet.py:558-567; betas pinned by tests/golden/beta_schedules.npz): the
    engine only sees coefficient tables, so the same kernels run another schedule - three reverse steps
    against the oracle fed with the reference's betas."""
    from diffroll_amd import ClassifierFreeDiffRoll
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=64, residual_layers=3, kernel_size=9, timesteps=50)
    p = R.synthetic_params(hp, seed=21)
    m = ClassifierFreeDiffRoll(
        residual_channels=64, unconditional=False, condition="fixed", n_mels=hp["n_mels"], norm_args=[0, 1, "imagewise"],
        residual_layers=3, kernel_size=9, dilation_base=hp["dilation_base"], dilation_bound=hp["dilation_bound"],
        spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=hp["n_mels"], f_min=0, f_max=8000,
                           normalized=True),
        timesteps=50, training={"mode": "x_0"}, sampling={"type": "cfdg_ddpm_x0", "w": 0.5}, beta_schedule="cosine")
    m.load_state_dict(p)
    betas = T(np.load(os.path.join(golden_dir, "beta_schedules.npz"))["cosine_50"])
    assert torch.equal(m.betas, betas)
    sch = R.schedule(0.0, 0.0, 50, betas=betas)
    torch.manual_seed(4)
    B, Tn = 2, 60
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    z = torch.randn(3, B, 1, Tn, 88)
    ref, out = x, x
    with torch.no_grad():
        spec = R.frontend(wav, hp, Tn)
        for i, t in enumerate((30, 29, 28)):
            ref = R.reverse_step(p, hp, sch, "cfdg_ddpm_x0", ref, spec, t, z[i], 0.5)
    for i, t in enumerate((30, 29, 28)):
        out, _ = m.reverse_diffusion(out, wav, t, noise=z[i])
    assert maxdiff(out.cpu(), ref) <= ATOL_STEP, maxdiff(out.cpu(), ref)


def test_q_sample_extract_x0_bit_exact(golden_dir):
    """diffroll_amd.q_sample / extract_x0 (dr_q_sample / dr_extract_x0) against the reference's free functions'
    outputs (task/diffusion.py:31-64): same operation order, one rounding per operation -> bit-exact; also
    against the oracle on a larger ragged case."""
    import diffroll_amd as D
    g = np.load(os.path.join(golden_dir, "qsample.npz"))
    dev = torch.device("cuda", 0)
    xt = D.q_sample(T(g["x0"]).to(dev), T(g["t"]), T(g["sac"]), T(g["s1m"]), noise=T(g["noise"]).to(dev))
    assert xt.shape == tuple(g["xt"].shape) and torch.equal(xt.cpu(), T(g["xt"]))
    x0b = D.extract_x0(T(g["xt"]).to(dev), T(g["eps"]).to(dev), T(g["t"]), T(g["sac"]), T(g["s1m"]))
    assert torch.equal(x0b.cpu(), T(g["x0_back"]))
    torch.manual_seed(9)
    sch = R.schedule(1e-4, 0.02, 50)
    x0, nz = torch.rand(7, 1, 333, 88), torch.randn(7, 1, 333, 88)
    t = torch.randint(0, 50, (7,))
    ref = R.q_sample(x0, t, sch["sqrt_alphas_cumprod"], sch["sqrt_one_minus_alphas_cumprod"], nz)
    out = D.q_sample(x0.to(dev), t, sch["sqrt_alphas_cumprod"], sch["sqrt_one_minus_alphas_cumprod"], noise=nz.to(dev))
    assert torch.equal(out.cpu(), ref)
    with pytest.raises(TypeError):
        D.q_sample(x0.to(dev), t, sch["sqrt_alphas_cumprod"], sch["sqrt_one_minus_alphas_cumprod"])


def test_roll_longer_than_spectrogram_is_trimmed(full_model):
    """trim_spec_roll (model/diffwave.py:30-39): T_roll > L // hop + 1 -> outputs have T' = L // hop + 1 frames."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=64, residual_layers=2, kernel_size=3, timesteps=4)
    p = R.synthetic_params(hp, seed=5)
    m = make_model(hp, p, sampler="ddpm_x0")
    torch.manual_seed(0)
    wav = 0.1 * torch.randn(2, 10 * 512)          # spectrogram has 11 frames
    x = torch.randn(2, 1, 20, 88)
    t = torch.tensor(1).repeat(2)
    with torch.no_grad():
        ref, ref_spec = R.forward(p, hp, x, wav, t)
    out, spec = m(x, wav, t)
    assert out.shape == ref.shape == (2, 1, 11, 88) and spec.shape == ref_spec.shape
    assert maxdiff(out.cpu(), ref) <= ATOL_FWD


def test_flexible_width_tiles_vs_oracle(monkeypatch):
    """Kernel flavours are chosen per launch geometry (16x16-MFMA 96 / 160-frame blocks, 32x32-MFMA 64 / 128,
    the direct-operand 1x1 at 64 .. 160 frames, split-K): force each one and hold it to the oracle on shapes
    that exercise ragged tails and every dilation."""
    import subprocess, sys, textwrap
    # the tune.* options are process-wide: run each forced variant in a child process
    code = textwrap.dedent("""
        import sys, torch, numpy as np
        torch.set_num_threads(min(16, torch.get_num_threads()))
        sys.path.insert(0, %r)
        from tools import tuning_env; tuning_env.install()
        from oracle import diffroll_ref as R
        from tests.testlib import make_model
        hp = dict(R.DEFAULT_HP); hp.update(residual_channels=128, residual_layers=4, kernel_size=9, timesteps=6)
        p = R.synthetic_params(hp, seed=77)
        m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
        sch = R.schedule(hp["beta_start"], hp["beta_end"], 6)
        g = torch.Generator().manual_seed(5)
        worst = 0.0
        import hashlib
        digest = hashlib.sha1()
        for B, Tn in ((2, 200), (1, 333), (3, 97)):
            wav = 0.1 * torch.randn(B, Tn * 512, generator=g); x = torch.randn(B, 1, Tn, 88, generator=g)
            z = torch.randn(B, 1, Tn, 88, generator=g); t = torch.tensor(2).repeat(B)
            with torch.no_grad():
                ref, _ = R.forward(p, hp, x, wav, t)
                ref_step = R.reverse_step(p, hp, sch, "cfdg_ddpm_x0", x, R.frontend(wav, hp, Tn), 2, z, 0.5)
            out, _ = m(x, wav, t); step, _ = m.reverse_diffusion(x, wav, 2, noise=z)
            worst = max(worst, float((out.cpu() - ref).abs().max()), float((step.cpu() - ref_step).abs().max()))
            digest.update(out.cpu().numpy().tobytes()); digest.update(step.cpu().numpy().tobytes())
        print("HASH", digest.hexdigest())
        print("WORST", worst)
    """ % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import tuning_env
    variants = [{"tune__tile": t} for t in (1603, 1605, 3203, 3205, 3202, 3201)]
    # the 1x1 kernel flavours: direct-operand pw_kernel at every block width, the LDS-staged kernel, no split-K
    variants += [{"tune__pw_nw": n} for n in (2, 3, 4, 5)] + [{"tune__pw": 0}, {"tune__ksplit_max": 1}]
    for var in variants:
        env = tuning_env.env_with(**var)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (var, r.stderr[-2000:])
        worst = float(r.stdout.strip().split("WORST")[-1])
        assert worst <= ATOL_FWD, (var, worst)
    # the 32x32-MFMA conv flavours (64 / 96 / 128 / 160-frame blocks) all accumulate in the same 32-channel blocks: with K
    # splitting and the fused stack out of the way they produce the same bits
    if tuning_env.forced("blocked_accumulation", 2) != 2:
        return              # (blocked_accumulation = 1: 128-frame blocks keep one chain, 96 / 160 fall back to the 16x16 kernels)
    hashes = {}
    for t in (3201, 3202, 3203, 3205):
        env = tuning_env.env_with(tune__tile=t, tune__ksplit_max=1, fused_stack=0)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (t, r.stderr[-2000:])
        hashes[t] = r.stdout.split("HASH")[-1].split()[0]
    assert hashes[3201] == hashes[3202] == hashes[3203] == hashes[3205], hashes


# --------------------------------------------------------------------------------------------
# round 5: the rewritten memory-bound kernels (multi-block min-max, bit-mask note scan, ticketed frame counts, float4
# q_sample) against plain numpy / torch at sizes that exercise every path of theirs
# --------------------------------------------------------------------------------------------
def _note_end_numpy(roll, thr):
    """note_end[b, t, p] = end (exclusive) of the run of frames > thr that STARTS at t, else 0."""
    on = roll > thr
    B, Tn, P = on.shape
    out = np.zeros((B, Tn, P), np.int32)
    for b in range(B):
        for p in range(P):
            col = on[b, :, p]
            t = 0
            while t < Tn:
                if col[t]:
                    e = t
                    while e < Tn and col[e]:
                        e += 1
                    out[b, t, p] = e
                    t = e
                else:
                    t += 1
    return out


@pytest.mark.parametrize("B,Tn", [(3, 1), (2, 31), (2, 32), (2, 33), (5, 125), (2, 640), (1, 2049), (1, 12001)])
def test_note_scan_bitmask_and_column_forms_vs_numpy(full_model, B, Tn):
    """dr_note_runs: the one-workgroup-per-clip bit-mask scan (T <= 12000) and the column walk behind it (longer rolls)
    against a plain run-length scan: word boundaries, a run that ends at T, all-on / all-off columns."""
    hp, p, m = full_model
    rng = np.random.default_rng(B * 100000 + Tn)
    base = rng.random((B, Tn // 5 + 1, 88)) < 0.25
    roll = np.repeat(base, 5, axis=1)[:, :Tn].astype(np.float32) * rng.uniform(0.51, 1.5, (B, Tn, 88)).astype(np.float32)
    roll[:, :, 0] = 0.9                      # a note as long as the clip
    roll[:, :, 1] = 0.1                      # silence
    roll[:, -1, 2] = 0.9                     # a note that starts on the last frame
    got = m.engine.note_runs(torch.from_numpy(roll), 0.5).cpu().numpy()
    assert np.array_equal(got, _note_end_numpy(roll, 0.5))


@pytest.mark.parametrize("n", [1, 3, 4, 8191, 8192, 176000, 2 * 1000 * 1000 + 3])
def test_frame_counts_ticketed_blocks_vs_numpy(full_model, n):
    """dr_frame_counts: 1 .. 256 blocks, float4 body + scalar tail, repeated calls (the ticket word re-arms itself)."""
    hp, p, m = full_model
    g = torch.Generator().manual_seed(n)
    pred = torch.rand(n, generator=g)
    label = (torch.rand(n, generator=g) > 0.8).float()
    pn, ln = pred.numpy() > 0.5, label.numpy() > 0.5
    want = (int((pn & ln).sum()), int((pn & ~ln).sum()), int((~pn & ln).sum()))
    dev = m.engine.device
    pd, ld = pred.to(dev), label.to(dev)
    for _ in range(3):
        assert m.engine.frame_counts(pd, ld, 0.5) == want
    if n > 8:       # an unaligned view: the scalar path
        pn, ln = pn[1:], ln[1:]
        want = (int((pn & ln).sum()), int((pn & ~ln).sum()), int((~pn & ln).sum()))
        assert m.engine.frame_counts(pd[1:], ld[1:], 0.5) == want


@pytest.mark.parametrize("B,L", [(1, 64000), (2, 63999), (3, 327680), (2, 5 * 327680)])
def test_multi_block_min_max_normalisation_vs_oracle(full_model, B, L):
    """The per-clip min / max over 1 .. 32 workgroups (119 KB .. 3 MB of log-mel per clip), twice (tickets re-arm),
    then a smaller batch in the same buffers (the scratch split moves)."""
    hp, p, m = full_model
    g = torch.Generator().manual_seed(L + B)
    wav = 0.1 * torch.randn(B, L, generator=g)
    Tn = L // 512
    with torch.no_grad():
        ref = R.frontend(wav, hp, Tn)
    for _ in range(2):
        spec = m.engine.frontend(wav, Tn).cpu()
        assert maxdiff(spec, ref) <= ATOL_SPEC
    spec1 = m.engine.frontend(wav[:1], Tn).cpu()
    assert maxdiff(spec1, ref[:1]) <= ATOL_SPEC


def test_q_sample_vector_and_scalar_paths_bit_exact():
    """dr_q_sample / dr_extract_x0: float4 path (per-sample size a multiple of 4, aligned) and the scalar path (odd sizes,
    unaligned views) against the torch expressions of task/diffusion.py:31-64, bit for bit."""
    from diffroll_amd import q_sample, extract_x0
    from diffroll_amd.schedule import make_schedule
    sch = make_schedule(1e-4, 0.02, 200)
    sac, s1m = sch["sqrt_alphas_cumprod"], sch["sqrt_one_minus_alphas_cumprod"]
    g = torch.Generator().manual_seed(4)
    for shape in ((4, 1, 125, 88), (3, 1, 7, 3), (2, 1, 640, 88)):
        x0 = torch.rand(shape, generator=g)
        z = torch.randn(shape, generator=g)
        t = torch.randint(0, 200, (shape[0],), generator=g)
        a = sac[t].reshape(-1, 1, 1, 1)
        c = s1m[t].reshape(-1, 1, 1, 1)
        xt = q_sample(x0.cuda(), t, sac, s1m, z.cuda()).cpu()
        assert torch.equal(xt, a * x0 + c * z)
        back = extract_x0(xt.cuda(), z.cuda(), t, sac, s1m).cpu()
        assert torch.equal(back, (xt - c * z) / a)
