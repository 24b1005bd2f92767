"""The identities the restatement of tests/chain_ref.py must have itself, bit for bit: the whole chain is the chain started
at its first visited step; a chain resumed from a row of the whole chain's trajectory ends in the whole chain's roll -
except under solver order 2 where the resumed step had a history to drop; a deterministic solver row reads no noise; and
the noise is the same roll as a tensor or as a dict."""
import functools

import numpy as np
import pytest
import torch

import chain_ref as CR

S, N, B, T = 200, 20, 2, 40
SAMPLER, W, INTERVAL = "cfdg_ddpm_x0", 0.5, (60, 140)
SOLVERS = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)]                 # (order, solver_noise); order 0 draws its own noise


@functools.lru_cache(maxsize=None)
def tiny():
    from oracle import diffroll_ref as R
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=16, residual_layers=2, kernel_size=3, timesteps=S)
    p = R.synthetic_params(hp, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 1, T, 88, generator=g)
    spec = torch.rand(B, int(hp["n_mels"]), T, generator=g)
    noise = torch.randn(S, B, 1, T, 88, generator=g)
    return hp, p, x, spec, noise


@functools.lru_cache(maxsize=None)
def whole(order, solver_noise):
    """The whole chain's trajectory (N, B, 1, T, 88): computed once per solver, never written to."""
    hp, p, x, spec, noise = tiny()
    return CR.sample_chain(p, hp, SAMPLER, x, spec, noise, N, w=W, interval=INTERVAL, trajectory=True, order=order,
                           solver_noise=solver_noise)


def chain(x, noise=None, **kw):
    hp, p, _, spec, z = tiny()
    return CR.sample_chain(p, hp, SAMPLER, x, spec, z if noise is None else noise, N, w=W, interval=INTERVAL, **kw)


@pytest.mark.parametrize("order,solver_noise", SOLVERS)
def test_the_whole_chain_is_the_chain_started_at_its_first_step(order, solver_noise):
    hp, _, x, _, _ = tiny()
    first = CR.visited(S, N)[0]
    assert first == S - 1 == CR.start_of(S, N, -1)
    got = chain(x, trajectory=True, order=order, solver_noise=solver_noise, start=first)
    assert torch.equal(got, whole(order, solver_noise))
    for a, b in zip(CR.chain_rows(hp, SAMPLER, N, order, solver_noise).items(),
                    CR.chain_rows(hp, SAMPLER, N, order, solver_noise, start=first).items()):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("order,solver_noise", SOLVERS)
def test_a_resumed_chain_ends_in_the_whole_chains_roll(order, solver_noise):
    hp = tiny()[0]
    steps = CR.visited(S, N)
    traj = whole(order, solver_noise)
    rows = CR.chain_rows(hp, SAMPLER, N, order, solver_noise)
    differs = []
    for i in (0, N // 2, N - 2):
        t_s = steps[i + 1]
        started = CR.chain_rows(hp, SAMPLER, N, order, solver_noise, start=t_s)
        assert list(started) == steps[i + 1:]
        got = chain(traj[i], order=order, solver_noise=solver_noise, start=t_s)
        if order and rows[t_s][3] != 0:                          # the resumed step had a history: it is dropped
            assert order == 2 and started[t_s][3] == 0
            assert np.array_equal(np.delete(started[t_s], 3), np.delete(rows[t_s], 3))
            assert not torch.equal(got, traj[-1]), (order, i)
            differs.append(i)
        else:
            assert np.array_equal(started[t_s], rows[t_s])
            assert torch.equal(got, traj[-1]), (order, i)
        assert all(np.array_equal(started[t], rows[t]) for t in steps[i + 2:])
    assert differs == ([0, N // 2] if order == 2 else [])         # the c = 0 rule shows mid-chain, and only under order 2


def test_a_deterministic_solver_row_reads_no_noise():
    g = torch.Generator().manual_seed(5)
    x, y, p, z = (torch.randn(3, 7, generator=g) for _ in range(4))
    for row in ([0.9, 0.2, 0.7, 0.4, 0.0], [0.9, 0.2, 0.7, 0.0, 0.0]):
        row = np.asarray(row, dtype=np.float32)
        for t in (7, 0):
            assert torch.equal(CR.solver_update(t, row, x, y, p), CR.solver_update(t, row, x, y, p, z))
            assert torch.equal(CR.solver_update(t, row, x, y, p), CR.solver_update(t, row, x, y, p, torch.full_like(z, float("nan"))))
    row = np.asarray([0.9, 0.2, 0.7, 0.4, 0.3], dtype=np.float32)
    assert not torch.equal(CR.solver_update(7, row, x, y, p, z), CR.solver_update(7, row, x, y, p, -z))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", [0, 2, 4, 20])
def test_deterministic_solver_rows_have_no_noise_column(n, order):
    hp = tiny()[0]
    det, sto = CR.solver_rows(hp, n, order, noise=0), CR.solver_rows(hp, n, order, noise=1)
    assert list(det) == list(sto) == CR.visited(S, n)
    for t in det:
        assert det[t].dtype == np.float32 and det[t][4] == 0 and (sto[t][4] != 0) == (t > 0)
        assert det[t][3] == sto[t][3] and det[t][2] == sto[t][2]                     # one c, one A


@pytest.mark.parametrize("order,solver_noise", [(0, 0), (1, 1), (2, 1)])
def test_noise_as_a_dict_is_noise_as_a_tensor(order, solver_noise):
    _, _, x, _, noise = tiny()
    as_dict = {t: noise[t] for t in CR.visited(S, N) if t > 0}
    assert torch.equal(chain(x, as_dict, order=order, solver_noise=solver_noise), whole(order, solver_noise)[-1])
    # ... from a start on it holds the started chain's steps only, and it is read
    steps = CR.visited(S, N)[N - 3:]
    x_s = whole(order, solver_noise)[N - 4]
    tail = {t: noise[t] for t in steps if t > 0}
    assert len(tail) == 2
    started = chain(x_s, order=order, solver_noise=solver_noise, start=steps[0])
    assert torch.equal(chain(x_s, tail, order=order, solver_noise=solver_noise, start=steps[0]), started)
    other = {t: -z for t, z in tail.items()}
    assert not torch.equal(chain(x_s, other, order=order, solver_noise=solver_noise, start=steps[0]), started)
