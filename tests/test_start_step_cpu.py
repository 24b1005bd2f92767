"""Options "start_step" / "start_noise" (include/diffroll_amd.h) without a GPU: the strength -> step rule, the header and the
public names, the facade's conversation with a stand-in engine (init xor x_T, trimming, start_noise held for the call only,
the drivers' refusal of a batch without a roll to start from), the CLI's keys and exits, sharding over two gloo ranks, and
the identity the restatement of tests/chain_ref.py must have itself: a chain resumed from a row of the whole chain's
trajectory ends in the whole chain's roll."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from testlib import free_port

import chain_ref as CR
from facade_fakes import HOP, L1, L2, MELS, RecordingEngine, clip, eq, facade, sample_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. check_start
def test_strength_to_step_table():
    from diffroll_amd.schedule import check_start, respaced_steps
    for n in (2, 20, 200):
        visited = respaced_steps(200, n)
        assert len(visited) == n
        for s in (0.001, 0.05, 0.1, 0.25, 0.3, 0.5, 0.75, 0.9, 0.999, 1.0):
            k = min(n, max(1, int(math.floor(s * n + 0.5))))
            want = -1 if k == n else visited[n - k]
            assert check_start(None, s, visited) == want, (n, s)
    v20 = respaced_steps(200, 20)
    assert check_start(None, 0.5, v20) == v20[10] == 94 and check_start(None, 0.05, v20) == 0 and check_start(None, 1, v20) == -1
    assert check_start(None, 0.01, v20) == 0                       # at least one step runs
    assert check_start(None, 0.5, respaced_steps(200, 2)) == 0 and check_start(None, 0.8, respaced_steps(200, 2)) == -1
    assert check_start(None, 0.5, respaced_steps(200, 0)) == 99    # 100 of the 200 steps: t = 99 .. 0


def test_check_start_values():
    from diffroll_amd.schedule import check_start, respaced_steps
    v20 = respaced_steps(200, 20)
    assert check_start(None, None, v20) == -1
    for t in v20:
        assert check_start(t, None, v20) == t
    with pytest.raises(ValueError, match="mutually exclusive"):
        check_start(94, 0.5, v20)
    for bad in (0, 0.0, -0.1, 1.5, "0.5", True, [0.5]):
        with pytest.raises(ValueError, match="strength"):
            check_start(None, bad, v20)
    for bad in (-1, 200, 94.0, "94", True):
        with pytest.raises(ValueError, match="start_step"):
            check_start(bad, None, v20)
    with pytest.raises(ValueError, match="start_step .*63 and 52"):
        check_start(57, None, v20)


# ---------------------------------------------------------------------------------------------- 2. header, names, null handle
def test_options_are_public_and_documented():
    from diffroll_amd import _cabi
    assert _cabi.DR_ABI_VERSION == 11
    assert "start_step" in _cabi.PUBLIC_OPTIONS and "start_noise" in _cabi.PUBLIC_OPTIONS
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", text).group(1)) == 11
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    assert re.search(r'"start_step"\s+\[-1\]', doc) and re.search(r'"start_noise"\s+\[0\]', doc)
    flat = re.sub(r"\s*\n \*\s*", " ", doc[doc.index('"start_step"'):])          # the two entries as running text
    for word in ("t <= t_s", "DR_EINVAL", "on either side", "captured chain's key", '"sampling_steps"', '"window_overlap"', '"draws"',
                 '"guidance_t_min"', '"solver_order"', "both precisions", "sharding", "INTEGRATION.md 3c",
                 "x = (A * x0) + (Sm * z)", "timesteps + t_s", "row 0 of d_noise", "dr_sample_checked", "dr_step ignores"):
        assert word in flat, word
    try:
        lib = _cabi.load_library()
    except RuntimeError:
        pytest.skip("library not built")
    assert lib.dr_set_option(None, b"start_step", 3) == _cabi.DR_EINVAL           # a null handle, never a crash
    assert lib.dr_set_option(None, b"start_noise", 1) == _cabi.DR_EINVAL


# ---------------------------------------------------------------------------------------------- 3. the facade
class StartEngine(RecordingEngine):
    """The stand-in of tests/test_facade_cpu.py, recording the two options among those in force at sample()."""

    def options(self):
        return dict(super().options(), start_step=self.start_step, start_noise=self.start_noise)


def start_facade(sampler="cfdg_ddpm_x0", timesteps=6, sampling=None, **kw):
    m, _ = facade(sampler, timesteps, sampling, **kw)
    eng = StartEngine(timesteps)
    m._engine, m._dirty = eng, False
    return m, eng


def call(sampler, x, z, seed=0, first=0, start_step=-1, start_noise=0, **options):
    c = sample_call(sampler, x, z, seed, first, **options)
    return c[:-1] + (dict(c[-1], start_step=start_step, start_noise=start_noise),)


def test_facade_init_xor_x_T_trimming_and_holding():
    m, eng = start_facade(sampling={"start_step": 3})
    assert m.start_step() == 3 and m.start_configured() == "start_step"
    wav, x, _, nz = clip(2, 125, frames=99)                  # 100 spectrogram frames: rolls and noise are trimmed
    init = torch.rand(2, 1, 125, 88)
    roll, spec = m.sample(None, wav, noise=nz, seed=2, init=init)
    z = nz[:, :, 0, :100].contiguous()
    assert eng.talk() == [("set_option", "start_step", 3), ("frontend", eq(wav), 125, None, None),
                          ("set_option", "start_noise", 1),
                          call("cfdg_ddpm_x0", init[:, 0, :100].contiguous(), z, 2, start_step=3, start_noise=1),
                          ("set_option", "start_noise", 0)]
    assert torch.equal(roll, init[:, :, :100]) and spec.shape == (2, MELS, 100) and eng.start_noise == 0
    # resume: x_T is x at the start step, and start_noise is never touched
    m.sample(x, wav, noise=nz)
    assert not any(c[0].startswith("set_") for c in eng.calls)
    assert eng.talk() == [call("cfdg_ddpm_x0", x[:, 0, :100].contiguous(), z, start_step=3)]
    # restored also when the chain raises
    eng.fail = True
    with pytest.raises(RuntimeError, match="sample failed"):
        m.sample(None, wav, init=init)
    assert eng.start_noise == 0 and eng.talk()[-1] == ("set_option", "start_noise", 0)
    eng.fail = False
    for bad in (dict(x_T=x, init=init), dict(x_T=None)):
        with pytest.raises(ValueError, match="either x_T"):
            m.sample(bad["x_T"], wav, init=bad.get("init"))
    with pytest.raises(ValueError, match="init holds 3 rolls: not a whole number of draws = 2"):
        m.sample(None, wav, init=torch.rand(3, 1, 125, 88), draws=2)
    assert eng.talk() == []
    # strength: read at every use; off while a single-step method of the reference runs
    m.hparams.sampling.start_step, m.hparams.sampling.strength = None, 0.5
    assert m.start_step() == 2 and m.start_configured() == "strength"
    m.sample(None, wav, init=init)
    assert ("set_option", "start_step", 2) in eng.talk()
    m.cfdg_ddpm_x0(x, wav, 4, torch.zeros(2, 1, 100, 88))
    got = eng.talk()
    assert got[0] == ("set_option", "start_step", -1) and got[1][0] == "step" and got[1][4] == 4
    m.hparams.sampling.start_step = 3
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.sample(None, wav, init=init)
    with pytest.raises(ValueError, match="strength"):
        start_facade(sampling={"strength": 1.5})
    with pytest.raises(ValueError, match="start_step"):
        start_facade(sampling={"steps": 3, "start_step": 4})           # 3 of 6 steps visit 5, 3, 0
    # without a start configured, init is diffused to the chain's first step
    m, eng = start_facade()
    m.sample(None, wav, init=init)
    assert eng.talk() == [("frontend", eq(wav), 125, None, None), ("set_option", "start_noise", 1),
                          call("cfdg_ddpm_x0", init[:, 0, :100].contiguous(), None, start_noise=1), ("set_option", "start_noise", 0)]


def test_facade_trajectory_and_drivers():
    m, eng = start_facade(sampling={"steps": 4, "start_step": 3})       # 4 of 6 steps: t = 5, 3, 2, 0
    assert m.visited_steps() == [5, 3, 2, 0]
    wav, x, _, nz = clip(2, 125)
    traj, _ = m.sample_trajectory(x, wav, noise=nz)
    assert [c[4] for c in eng.talk() if c[0] == "step"] == [3, 2, 0] and traj.shape == (3, 2, 1, 125, 88)
    # the drivers take the roll to start from out of the batch, and refuse a batch without one, naming the key
    init = torch.rand(2, 1, 125, 88)
    roll = m.predict_step((x, wav, init), batch_idx=4)
    assert eng.talk() == [("set_option", "start_noise", 1), call("cfdg_ddpm_x0", init[:, 0], None, 4, start_step=3, start_noise=1),
                          ("set_option", "start_noise", 0)]
    assert torch.equal(roll, init)
    with pytest.raises(ValueError, match=r"hparams\.sampling\.start_step"):
        m.predict_step((x, wav), batch_idx=4)
    batch = {"frame": torch.zeros(2, 125, 88), "audio": wav, "x_T": x}
    with pytest.raises(ValueError, match=r"hparams\.sampling\.start_step"):
        m.sampling(batch, batch_idx=6)
    with pytest.raises(ValueError, match=r"hparams\.sampling\.start_step"):
        m.test_step(batch, batch_idx=6)
    assert eng.talk() == []
    roll, spec = m.sampling(dict(batch, init=init), batch_idx=6)
    assert eng.talk()[1] == call("cfdg_ddpm_x0", init[:, 0], None, 6, start_step=3, start_noise=1)
    assert torch.equal(roll, init) and spec.shape == (2, MELS, 125)
    m.hparams.sampling.start_step, m.hparams.sampling.strength = None, 1.0      # the whole chain, still FROM a roll
    with pytest.raises(ValueError, match=r"hparams\.sampling\.strength"):
        m.predict_step((x, wav))
    # draws: the one roll per clip starts every draw
    m.hparams.sampling.draws = 2
    m.predict_step((x, wav, init), batch_idx=1)
    got = [c for c in eng.talk() if c[0] == "sample"]
    assert got == [call("cfdg_ddpm_x0", init.repeat(2, 1, 1, 1)[:, 0], None, 1, start_noise=1, draws=2)]


def test_facade_long_form_init():
    from diffroll_amd import longform
    m, eng = start_facade(timesteps=4, sampling={"strength": 0.5})
    g = torch.Generator().manual_seed(5)
    wav = torch.randn(L2, generator=g)
    plan = longform.plan_windows(L2, HOP, overlap=32)
    init = torch.rand(1, 1, plan.T_out, 88, generator=g)
    canvas = torch.zeros(1, 1, plan.T_c, 88)
    canvas[:, :, :plan.T_out] = init
    roll = m.sample_long(wav, overlap=32, seed=3, recording=2, init=init)
    got = eng.talk()
    sample = [c for c in got if c[0] == "sample"]
    xw = longform.gather_windows(canvas.reshape(plan.T_c, 88), plan)
    assert sample == [call("cfdg_ddpm_x0", xw, None, 3, 2, start_step=1, start_noise=1, window_overlap=32)]
    assert got[-1][0] == "set_option" and eng.start_noise == 0 and eng.window_overlap == 0
    assert roll.shape == (1, 1, plan.T_out, 88) and torch.equal(roll, init)      # the stand-in's chain is the identity
    m.sample_long(wav, overlap=32, init=roll)                                    # feeding a returned roll back works
    # two recordings, two draws: a single roll per recording is shared by the draws
    wav1 = torch.randn(L1, generator=g)
    p1 = longform.plan_windows(L1, HOP, overlap=32)
    init1 = torch.rand(1, 1, p1.T_out, 88, generator=g)
    eng.talk()
    rolls = m.sample_long_batch([wav1, wav], overlap=32, draws=2, init=[init1, init])
    sample = [c for c in eng.talk() if c[0] == "sample"]
    assert len(sample) == 1 and sample[0][-1]["start_noise"] == 1 and sample[0][-1]["draws"] == 2
    assert [tuple(r.shape) for r in rolls] == [(2, 1, p1.T_out, 88), (2, 1, plan.T_out, 88)]
    assert torch.equal(rolls[0][0], init1[0]) and torch.equal(rolls[0][1], init1[0]) and torch.equal(rolls[1][1], init[0])
    for bad, match in ((dict(init=init, x_T=canvas), "either x_T"), (dict(init=init[:, :, :-1]), "init must be one roll"),
                       (dict(init=torch.rand(3, 1, plan.T_out, 88)), "init must be one roll")):
        with pytest.raises(ValueError, match=match):
            m.sample_long(wav, overlap=32, **bad)


# ---------------------------------------------------------------------------------------------- 4. the CLI
LONG = ["task=transcription", "dataset=Custom", "dataset.args.max_segment_samples=null"]


def test_cli_keys_and_exits(tmp_path):
    from diffroll_amd import cli
    cfg = cli.build_config(LONG + ["task.sampling.steps=20", "task.sampling.strength=0.5", "task.sampling.init_dir=rolls"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 0.5, "steps": 20, "strength": 0.5, "init_dir": "rolls"}
    cfg = cli.build_config(LONG + ["task.sampling.start_step=77", "task.sampling.init_dir=rolls", "task.recordings_per_chain=3",
                                   "task.sampling.draws=2"])
    assert cfg["task"]["sampling"]["start_step"] == 77
    assert "strength" not in cli.build_config(["task=transcription"])["task"]["sampling"]
    for bad, key in (("task.sampling.strength=0", "strength"), ("task.sampling.strength=1.5", "strength"),
                     ("task.sampling.start_step=200", "start_step"), ("task.sampling.start_step=-1", "start_step")):
        with pytest.raises(SystemExit, match=rf"task\.sampling\.{key}"):
            cli.build_config(LONG + [bad, "task.sampling.init_dir=rolls"])
    with pytest.raises(SystemExit, match=r"task\.sampling\.start_step.*63 and 52"):
        cli.build_config(LONG + ["task.sampling.steps=20", "task.sampling.start_step=57", "task.sampling.init_dir=rolls"])
    with pytest.raises(SystemExit, match=r"task\.sampling\.strength.*mutually exclusive"):
        cli.build_config(LONG + ["task.sampling.strength=0.5", "task.sampling.start_step=77", "task.sampling.init_dir=rolls"])
    with pytest.raises(SystemExit, match=r"task\.sampling\.strength.*init_dir"):
        cli.build_config(LONG + ["task.sampling.strength=0.5"])
    with pytest.raises(SystemExit, match=r"task\.sampling\.init_dir needs"):
        cli.build_config(LONG + ["task.sampling.init_dir=rolls"])
    # everywhere but the long-form path: refused, naming the key
    for argv in (["task=transcription"], ["task=generation"], ["task=transcription", "dataset=Custom"]):
        with pytest.raises(SystemExit, match=r"task\.sampling\.strength.*max_segment_samples=null"):
            cli.build_config(argv + ["task.sampling.strength=0.5", "task.sampling.init_dir=rolls"])


class LongModel:
    """What transcribe_long_form asks of the model, recorded."""

    def __init__(self):
        self.calls = []

    def sample_long(self, wav, overlap=160, seed=0, recording=0, draws=1, init=None):
        self.calls.append(("sample_long", tuple(wav.shape), seed, recording, draws, None if init is None else init.clone()))
        return torch.zeros(draws, 1, -(-wav.shape[0] // 512), 88)

    def sample_long_batch(self, wavs, overlap=160, seed=0, first_recording=0, draws=1, init=None):
        self.calls.append(("sample_long_batch", len(wavs), seed, first_recording, draws, None if init is None else [r.clone() for r in init]))
        return [torch.zeros(draws, 1, -(-w.shape[0] // 512), 88) for w in wavs]

    def export_midi(self, roll, raw, clean_prefix=None):
        for prefix in (raw, clean_prefix):
            open(prefix + "0.mid", "wb").close()


def test_cli_reads_the_rolls_it_writes(tmp_path):
    from scipy.io import wavfile
    from diffroll_amd import cli
    wav_dir, init_dir, out = tmp_path / "audio", tmp_path / "first", tmp_path / "second"
    for d in (wav_dir, init_dir, out):
        d.mkdir()
    rng = np.random.default_rng(0)
    lengths = {"a": 700 * 512 - 100, "b": 300 * 512 + 5}
    for stem, L in lengths.items():
        wavfile.write(str(wav_dir / f"{stem}.wav"), 16000, (0.1 * rng.standard_normal(L)).astype(np.float32))
    argv = LONG + [f"dataset.args.audio_path={wav_dir}", "dataset.args.audio_ext=wav", f"output_dir={out}", "seed=3",
                   "task.sampling.steps=20", "task.sampling.strength=0.5", f"task.sampling.init_dir={init_dir}"]
    cfg = cli.build_config(argv)
    with pytest.raises(SystemExit, match=r"task\.sampling\.init_dir.*roll_a\.npy does not exist"):
        cli.transcribe_long_form(cfg, LongModel(), 0, 1)
    rolls = {stem: rng.random((1, 1, -(-L // 512), 88)).astype(np.float32) for stem, L in lengths.items()}
    np.save(str(init_dir / "roll_a.npy"), rolls["a"])
    np.save(str(init_dir / "roll_b.npy"), rolls["b"][:, :, :-1])
    with pytest.raises(SystemExit, match=r"task\.sampling\.init_dir.*roll_b\.npy has shape"):
        cli.transcribe_long_form(cfg, LongModel(), 0, 1)
    np.save(str(init_dir / "roll_b.npy"), rolls["b"])
    m = LongModel()
    written = cli.transcribe_long_form(cfg, m, 0, 1)
    assert [os.path.basename(p) for p in written] == ["roll_a.npy", "roll_b.npy"]
    assert [(c[0], c[2], c[3]) for c in m.calls] == [("sample_long", 3, 0), ("sample_long", 4, 1)]
    assert all(np.array_equal(c[5].numpy(), rolls[s]) for c, s in zip(m.calls, "ab"))
    # several recordings per chain and draws: one roll per recording, shared by the draws
    cfg = cli.build_config(argv + ["task.recordings_per_chain=2", "task.sampling.draws=2"])
    m = LongModel()
    cli.transcribe_long_form(cfg, m, 0, 1)
    assert [(c[0], c[1], c[4]) for c in m.calls] == [("sample_long_batch", 2, 2)]
    assert all(np.array_equal(r.numpy(), rolls[s]) for r, s in zip(m.calls[0][5], "ab"))
    # what was written can be read back as the next run's init
    assert np.load(str(out / "roll_a.npy")).shape == rolls["a"].shape


# ---------------------------------------------------------------------------------------------- 5. sharding
class ShardModel:
    """sample() as a per-row function of (roll, which keyword carried it, global row key)."""

    class engine:
        device = torch.device("cpu")

    def output_frames(self, T, waveform_samples):
        return T

    def sample(self, x_T, waveform=None, noise=None, seed=0, first_sample=0, draws=1, draw_stride=0, init=None):
        assert (x_T is None) != (init is None)
        src = init if x_T is None else x_T
        n = src.shape[0] // draws
        out = src.clone() * (0.25 if x_T is None else 0.5) + waveform.mean(dim=1).repeat(draws).view(-1, 1, 1, 1)
        for b in range(src.shape[0]):
            key = first_sample + b % n + (b // n) * (draw_stride or n)
            out[b] += torch.randn(out[b].shape, generator=torch.Generator().manual_seed(seed * 1000003 + key))
        return out, None


def _shard_worker(rank, world, port, B, draws, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from diffroll_amd.distributed import sample_sharded
    torch.manual_seed(0)
    init, wav = torch.rand(draws * B, 1, 6, 88), torch.randn(B, 64)
    full = sample_sharded(ShardModel(), None, wav, seed=5, draws=draws, init=init)
    if rank == 0:
        ret.put(full)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("B,draws", [(5, 1), (3, 2)])
def test_init_is_sharded_like_x_T(B, draws):
    from diffroll_amd.distributed import sample_shard, sample_sharded
    torch.manual_seed(0)
    init, wav = torch.rand(draws * B, 1, 6, 88), torch.randn(B, 64)
    single = sample_sharded(ShardModel(), None, wav, seed=5, draws=draws, init=init)         # no process group: world = 1
    assert torch.equal(single, ShardModel().sample(None, wav, seed=5, draws=draws, init=init)[0])
    assert not torch.equal(single, sample_sharded(ShardModel(), init, wav, seed=5, draws=draws))
    with pytest.raises(ValueError, match="either x_T or init"):
        sample_shard(ShardModel(), init, wav, None, 5, 0, 1, draws, init)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, B, draws, q)) for r in range(2)]
    for p in procs:
        p.start()
    full = q.get(timeout=120)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert torch.equal(full, single)


# ---------------------------------------------------------------------------------------------- 6. the restatement itself
def tiny():
    from oracle import diffroll_ref as R
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=16, residual_layers=2, kernel_size=3, timesteps=12)
    p = R.synthetic_params(hp, seed=3)
    g = torch.Generator().manual_seed(4)
    B, T = 2, 8
    x = torch.randn(B, 1, T, 88, generator=g)
    spec = torch.rand(B, int(hp["n_mels"]), T, generator=g)
    noise = torch.randn(12, B, 1, T, 88, generator=g)
    return hp, p, x, spec, noise


@pytest.mark.parametrize("order", [0, 1, 2])
def test_the_restatement_resumes_its_own_trajectory(order):
    hp, p, x, spec, noise = tiny()
    n = 6
    steps = CR.visited(12, n)
    whole = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, n, w=0.5, trajectory=True, order=order)
    assert torch.equal(whole, CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, spec, noise, n, start=CR.start_of(12, n, -1), w=0.5, trajectory=True,
                                             order=order))
    for i in (0, 2, n - 2):
        t_s = steps[i + 1]
        got = CR.sample_chain(p, hp, "cfdg_ddpm_x0", whole[i], spec, noise, n, start=t_s, w=0.5, order=order)
        rows = CR.chain_rows(hp, "cfdg_ddpm_x0", n, order=order, start=t_s)
        assert list(rows) == steps[i + 1:]
        if order < 2:
            assert torch.equal(got, whole[-1]), (order, i)
        else:
            assert rows[t_s][3] == 0                              # the first started row is first order ...
            second = CR.solver_rows(hp, n, 2)[t_s][3] != 0               # ... where the whole chain's row is second order
            assert torch.equal(got, whole[-1]) != second, (i, t_s)
    assert any(CR.solver_rows(hp, n, 2)[steps[i + 1]][3] != 0 for i in (0, 2, n - 2))


def test_the_restatements_diffusion():
    hp, p, x, spec, noise = tiny()
    x0 = torch.rand(2, 1, 8, 88)
    tab = CR.committed(hp)
    z = CR.diffusion_noise(7, 3, 12, 2, 8, 5)
    assert z.shape == (2, 1, 8, 88) and abs(float(z.std()) - 1) < 0.1
    from oracle import philox
    assert np.array_equal(z.numpy().reshape(2, -1), philox.step_noise(7, 3, 2, 8 * 88, 12 + 5))
    assert not np.array_equal(z.numpy().reshape(2, -1), philox.step_noise(7, 3, 2, 8 * 88, 5))
    got = CR.diffuse(hp, x0, 5, z)
    assert torch.equal(got, torch.tensor(tab[0, 5, 2]) * x0 + torch.tensor(tab[0, 5, 3]) * z)
    # windows: one canvas draw per recording, so shared frames carry the same z
    from diffroll_amd import longform
    plan = longform.plan_windows(40, None, T=16, overlap=4)
    zw = CR.window_noise(7, 3, 12, plan, 5)
    assert zw.shape == (plan.n, 1, 16, 88)
    for b in range(plan.n - 1):
        assert torch.equal(zw[b, 0, plan.stride:], zw[b + 1, 0, :plan.overlap])
    t_s = CR.visited(12, 6)[2]
    z = CR.diffusion_noise(7, 3, 12, 2, 8, t_s)
    a = CR.refine_chain(p, hp, "cfdg_ddpm_x0", x0, spec, noise, 6, t_s, z, w=0.5)
    b = CR.sample_chain(p, hp, "cfdg_ddpm_x0", CR.diffuse(hp, x0, t_s, z), spec, noise, 6, start=t_s, w=0.5)
    assert torch.equal(a, b)
