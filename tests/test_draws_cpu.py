"""Several draws per clip (options "draws" / "draw_stride", diffroll_amd/ensemble.py) without a GPU: the draw-major layout
and the aggregates against explicit numpy, the Philox key of a row against a table, hparams.sampling.draws and the CLI's
task.sampling.draws, and the sharded path's regrouping on two gloo ranks with a stand-in model."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def test_aggregate_against_numpy_and_the_draw_major_layout():
    from diffroll_amd.ensemble import aggregate, split_draws
    D, n, T = 4, 3, 7
    g = torch.Generator().manual_seed(12)
    rolls = torch.rand(D * n, 1, T, 88, generator=g)
    mean, votes, std = aggregate(rolls, D, threshold=0.4)
    a = rolls.numpy().astype(np.float64)
    for c in range(n):
        rows = np.stack([a[d * n + c] for d in range(D)])          # row b = draw b // n of clip b % n
        np.testing.assert_allclose(mean[c].numpy(), rows.mean(0), rtol=0, atol=1e-6)
        np.testing.assert_allclose(std[c].numpy(), rows.std(0), rtol=0, atol=1e-6)
        assert np.array_equal(votes[c].numpy(), (rows > 0.4).mean(0).astype(np.float32))
    assert mean.dtype == votes.dtype == std.dtype == torch.float32 and mean.shape == (n, 1, T, 88)
    assert set(np.unique(votes.numpy())) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    # a clip-major reading of the same tensor gives other numbers: the layout is pinned
    wrong = rolls.reshape(n, D, 1, T, 88).mean(1)
    assert not torch.allclose(wrong, mean)
    assert torch.equal(split_draws(rolls, D)[2, 1], rolls[2 * n + 1])
    # one draw: the roll itself, no spread; half precision is aggregated in fp32
    m1, v1, s1 = aggregate(rolls, 1)
    assert torch.equal(m1, rolls) and float(s1.abs().max()) == 0.0 and torch.equal(v1, (rolls > 0.5).float())
    assert aggregate(rolls.half(), D)[0].dtype == torch.float32
    for bad in (5, 0, -1, 2.0, True):
        with pytest.raises(ValueError):
            aggregate(rolls, bad)


def test_row_keys_against_a_table():
    """first_sample + (b % n) + (b / n) * G, G = 0 meaning n (include/diffroll_amd.h, option "draw_stride")."""
    from diffroll_amd.ensemble import draw_key
    # n = 2 clips, D = 3 draws, first_sample = 10
    assert [draw_key(10, b, 2) for b in range(6)] == [10, 11, 12, 13, 14, 15]                # G = 0: first_sample + b
    assert [draw_key(10, b, 2, 7) for b in range(6)] == [10, 11, 17, 18, 24, 25]
    assert [draw_key(0, b, 3, 100) for b in range(9)] == [0, 1, 2, 100, 101, 102, 200, 201, 202]
    # a sharded run (G = the global clip count B): rank shards [lo, hi) with first_sample = lo give draw d of global clip c
    # the key c + d * B on any world size
    B, D = 5, 3
    for world in (1, 2, 3, 5):
        from diffroll_amd.distributed import shard_bounds
        keys = {}
        for r in range(world):
            lo, hi = shard_bounds(B, r, world)
            for b in range(D * (hi - lo)):
                keys[(b // (hi - lo), lo + b % (hi - lo))] = draw_key(lo, b, hi - lo, B)
        assert keys == {(d, c): c + d * B for d in range(D) for c in range(B)}, world


def _model(**kw):
    from diffroll_amd import ClassifierFreeDiffRoll
    base = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=229, norm_args=[0, 1, "imagewise"],
                residual_layers=2, kernel_size=3, dilation_base=2, dilation_bound=4,
                spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000,
                               center=True, normalized=True, pad_mode="reflect"),
                timesteps=200)
    base.update(kw)
    return ClassifierFreeDiffRoll(**base)


def test_facade_hparams_sampling_draws():
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5})
    assert "draws" not in m.hparams.sampling and m.draws() == 1
    assert _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "draws": None}).draws() == 1
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "draws": 8})
    assert m.hparams.sampling.draws == 8 and m.draws() == 8
    m.hparams.sampling.draws = 2                       # read at every use, like the other hparams.sampling keys
    assert m.draws() == 2
    for bad in (0, -2, 1.5, "4", True):
        with pytest.raises(ValueError):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "draws": bad})


def test_cli_parses_and_validates_sampling_draws():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription"])
    assert "draws" not in cfg["task"]["sampling"]
    cfg = cli.build_config(["task=transcription", "task.sampling.draws=8"])
    assert cfg["task"]["sampling"]["draws"] == 8
    assert cli.build_config(["task=transcription", "task.sampling.draws=null"])["task"]["sampling"]["draws"] is None
    for bad in ("0", "-1", "2.5", "many", "true"):
        with pytest.raises(SystemExit, match="task.sampling.draws"):
            cli.build_config(["task=transcription", f"task.sampling.draws={bad}"])


def test_the_options_are_public_and_documented():
    import re
    from diffroll_amd import _cabi
    assert "draws" in _cabi.PUBLIC_OPTIONS and "draw_stride" in _cabi.PUBLIC_OPTIONS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "diffroll_amd.h")).read()
    block = re.search(r"/\*(?:(?!\*/).)*\*/\s*int dr_set_option", header, re.S).group(0)
    assert '"draws"' in block and '"draw_stride"' in block
    assert _cabi.DR_ABI_VERSION == 11


# ------------------------------------------------------------------------------------------------ sharding
class FakeEngine:
    device = torch.device("cpu")


class FakeModel:
    """sample() mimics the contract of ClassifierFreeDiffRoll.sample with draws: row b is draw b // n of clip b % n, reads
    the waveform of clip b % n, and its noise is injected or derived from (seed, the row's key)."""
    engine = FakeEngine()

    def output_frames(self, T, waveform_samples):
        return T

    def sample(self, x_T, waveform=None, noise=None, seed=0, first_sample=0, use_graph=True, draws=1, draw_stride=0):
        from diffroll_amd.ensemble import draw_key
        B = x_T.shape[0]
        n = B // draws
        assert waveform is None or waveform.shape[0] == n
        out = x_T.clone() * 0.5
        for b in range(B):
            if waveform is not None:
                out[b] += waveform[b % n].mean()
            if noise is not None:
                out[b] += noise[:, b].sum(0)
            else:
                g = torch.Generator().manual_seed(seed * 1000003 + draw_key(first_sample, b, n, draw_stride))
                out[b] += torch.randn(out[b].shape, generator=g)
        return out, None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inputs(B, D, use_noise):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(D * B, 1, 6, 88, generator=g)
    wav = torch.randn(B, 64, generator=g)
    noise = torch.randn(4, D * B, 1, 6, 88, generator=g) if use_noise else None
    return x, wav, noise


def _worker(rank, world, port, B, D, use_noise, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from diffroll_amd.distributed import sample_sharded
    x, wav, noise = _inputs(B, D, use_noise)
    full = sample_sharded(FakeModel(), x, wav, noise, seed=5, draws=D)
    if rank == 0:
        ret.put(full)
    dist.barrier()
    dist.destroy_process_group()


def _expected(B, D, use_noise):
    """Every (draw, global clip) on its own: draw-major over the GLOBAL batch, keys c + d * B."""
    x, wav, noise = _inputs(B, D, use_noise)
    rows = []
    for d in range(D):
        for c in range(B):
            b = d * B + c
            r = x[b] * 0.5 + wav[c].mean()
            if noise is not None:
                r = r + noise[:, b].sum(0)
            else:
                r = r + torch.randn(r.shape, generator=torch.Generator().manual_seed(5 * 1000003 + c + d * B))
            rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("B,D,use_noise", [(5, 3, False), (4, 2, True)])
def test_sharded_draws_on_two_gloo_ranks_are_regrouped_draw_major(B, D, use_noise):
    from diffroll_amd.distributed import clip_major, draw_major, sample_sharded, sample_sharded_sequential
    want = _expected(B, D, use_noise)
    x, wav, noise = _inputs(B, D, use_noise)
    single = sample_sharded(FakeModel(), x, wav, noise, seed=5, draws=D)          # no process group: world = 1
    assert torch.equal(single, want)
    for G in (2, 3, 8):                                                           # empty shards included
        assert torch.equal(sample_sharded_sequential(FakeModel(), x, wav, noise, seed=5, world_size=G, draws=D), want), G
    assert torch.equal(draw_major(clip_major(x, D), D), x)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, B, D, use_noise, q)) for r in range(2)]
    for p in procs:
        p.start()
    full = q.get(timeout=120)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert full.shape == (D * B, 1, 6, 88) and torch.equal(full, want)
