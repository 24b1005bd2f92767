"""Respaced sampling (option "sampling_steps", include/diffroll_amd.h) without a GPU: the visited-step rule, the derived
coefficient rows, the facade's hparams.sampling.steps and the CLI's task.sampling.steps."""
import numpy as np
import pytest

from oracle import diffroll_ref as R

import chain_ref as CR


@pytest.mark.parametrize("S", [2, 3, 8, 50, 199, 200, 1000])
def test_visited_steps_rule(S):
    from diffroll_amd.schedule import respaced_steps
    assert respaced_steps(S, 0) == respaced_steps(S, S) == list(range(S - 1, -1, -1))
    assert respaced_steps(S, 2) == [S - 1, 0]
    for n in range(2, min(S, 60) + 1):
        st = respaced_steps(S, n)
        assert st == CR.visited(S, n)
        assert len(st) == n and st[0] == S - 1 and st[-1] == 0
        assert all(a > b for a, b in zip(st, st[1:])), (S, n, st)
        # linspace(0, S - 1, n) rounded half up
        want = [int(np.floor(i * (S - 1) / (n - 1) + 0.5 + 1e-9)) for i in range(n - 1, -1, -1)]
        assert st == want, (S, n)


def test_visited_steps_at_the_shipping_schedule():
    from diffroll_amd.schedule import respaced_steps
    assert respaced_steps(200, 50)[:4] == [199, 195, 191, 187] and respaced_steps(200, 50)[-3:] == [8, 4, 0]
    assert respaced_steps(200, 20)[:3] == [199, 189, 178]
    assert respaced_steps(200, 100)[:3] == [199, 197, 195]
    for bad in (1, -1, 201, 2.5, True, "50"):
        with pytest.raises(ValueError):
            respaced_steps(200, bad)


def test_derived_rows_at_stride_one_restate_the_committed_rows():
    """Sanity check of the row formulas (stride-1 rows are never derived: the committed ones are used).  Columns that are
    schedule scalars are copied exactly; the others agree to the rounding of the fp32 square roots they are derived from -
    a few ulp where they are well conditioned, and up to 4.3e-4 relative (2.6e-6 absolute) near t = 1, where
    1 - (A / Ap)^2 = beta_t cancels."""
    hp = dict(R.DEFAULT_HP)
    tab = CR.committed(hp)
    S = int(hp["timesteps"])
    exact = [(f, k) for f in range(5) for k in range(5)
             if not ((f in (0, 4) and k in (1, 4)) or (f == 1 and k == 1) or (f == 2 and k in (0, 1, 3)))]
    for t in range(1, S):
        d = CR.derived_rows(tab[0, t, 2], tab[0, t - 1, 2], tab[0, t, 3], tab[0, t - 1, 3]).astype(np.float64)
        c = tab[:, t, :].astype(np.float64)
        for f, k in exact:
            assert d[f, k] == c[f, k], (t, f, k)
        err = np.abs(d - c)
        assert err.max() <= 4e-6, (t, err.max())
        assert (err <= 1e-3 * np.abs(c) + 1e-30).all(), t
        if t >= 20:          # away from the cancellation
            assert (err <= 8e-5 * np.abs(c) + 1e-30).all(), t
    assert d[2, 0] == pytest.approx(c[2, 0], rel=2.0 ** -22)


def test_respaced_rows_keep_committed_rows_where_the_stride_is_one():
    hp = dict(R.DEFAULT_HP)
    tab = CR.committed(hp)
    for n in (2, 20, 50, 100, 150, 200):
        st = CR.visited(200, n)
        rows = CR.rows_for(tab, st)
        for i, t in enumerate(st):
            if t == 0 or st[i + 1] == t - 1:
                assert np.array_equal(rows[t], tab[:, t, :])
            else:
                assert not np.array_equal(rows[t], tab[:, t, :])
            assert np.isfinite(rows[t]).all() and (rows[t] >= 0).all()


def _model(**kw):
    from diffroll_amd import ClassifierFreeDiffRoll
    base = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=229, norm_args=[0, 1, "imagewise"],
                residual_layers=2, kernel_size=3, dilation_base=2, dilation_bound=4,
                spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000,
                               center=True, normalized=True, pad_mode="reflect"),
                timesteps=200)
    base.update(kw)
    return ClassifierFreeDiffRoll(**base)


def test_facade_hparams_sampling_steps():
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5})
    assert "steps" not in m.hparams.sampling and m.sampling_steps() == 0
    assert m.visited_steps() == list(range(199, -1, -1))
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "steps": None})
    assert m.sampling_steps() == 0
    m = _model(sampling={"type": "ddim", "steps": 50})
    assert m.hparams.sampling.steps == 50 and m.sampling_steps() == 50
    assert m.visited_steps() == CR.visited(200, 50)
    m.hparams.sampling.steps = 20                     # read at every use, like the other hparams.sampling keys
    assert m.visited_steps() == CR.visited(200, 20)
    assert _model(sampling={"type": "ddim", "steps": 200}).visited_steps() == list(range(199, -1, -1))
    for bad in (1, 201, -3, 2.0, "50"):
        with pytest.raises(ValueError):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "steps": bad})


def test_load_from_checkpoint_sampling_steps_override(golden_dir):
    import os
    from diffroll_amd import ClassifierFreeDiffRoll
    path = os.path.join(golden_dir, "trained_small.ckpt")
    m = ClassifierFreeDiffRoll.load_from_checkpoint(path)
    assert m.hparams.sampling.get("steps") is None and m.sampling_steps() == 0      # the reference's configs: every step
    m = ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "steps": 50})
    assert m.hparams.sampling.type == "cfdg_ddpm_x0" and m.hparams.sampling.steps == 50 and m.sampling_steps() == 50
    with pytest.raises(ValueError):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "steps": 1})


def test_cli_validates_sampling_steps():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "task.sampling.steps=50"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 0.5, "steps": 50}
    assert cli.steps_label(cfg) == "50 of 200 steps"
    assert cli.build_config(["task=generation"])["task"]["sampling"].get("steps") is None
    for ok in ("0", "null", "2", "200"):
        cli.build_config(["task=transcription", f"task.sampling.steps={ok}"])
    cfg = cli.build_config(["task=transcription", "task.timesteps=40", "task.sampling.steps=40"])
    assert cli.steps_label(cfg) == "40 steps"
    # with the long-form path (and any gpus=N: the option travels in the model's hparams)
    cfg = cli.build_config(["task=transcription", "dataset=Custom", "dataset.args.max_segment_samples=null",
                            "task.sampling.steps=20", "gpus=2"])
    assert cfg["task"]["sampling"]["steps"] == 20 and cli.is_long_form(cfg)
    for bad in ("1", "201", "-5", "2.5", "true", "fifty"):
        with pytest.raises(SystemExit):
            cli.build_config(["task=transcription", f"task.sampling.steps={bad}"])
    with pytest.raises(SystemExit):
        cli.build_config(["task=transcription", "task.timesteps=40", "task.sampling.steps=50"])
