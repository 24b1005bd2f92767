"""Precision "bf16" (DR_PRECISION_BF16, include/diffroll_amd.h) on the GPU: one bf16 MFMA per K step in the two hot
contractions, operands rounded once to nearest even, fp32 accumulation.

A deep bf16 network is not held element-wise to a restatement (tests/test_bf16_cpu.py says why, and shows that the bands
used here discriminate): with e = got - float64 network and e_ref the error of the fp32-accumulated restatement
(tests/bf16_ref.py), 0.5 rms(e_ref) <= rms(e) <= 1.15 rms(e_ref) and max|e| <= 2 max|e_ref|.  The lower bound proves that
the mode is engaged (the exact path lies four orders of magnitude below), the upper ones refuse truncation (2.3 - 3.2 x
in rms) and anything worse.  That is true of the network, not of one contraction: SINGLE layers of the mode are held element
by element in tests/test_gpu_layer_probe.py, which sees the one-element faults these bands let through
(tests/test_layer_probe_cpu.py).  What IS held bit for bit here: fused against per-phase launches, captured against plain chains,
run against run, shared window frames, and the other precisions after a visit to this one."""
import json
import os
import subprocess
import sys

import pytest
import torch

import bf16_ref as Q
import chain_ref
from oracle import diffroll_ref as R
from testlib import make_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _log(line):
    print(line)
    log = os.environ.get("DR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("geometry", Q.GEOMETRIES, ids=lambda g: "C%d-L%d-k%d-B%d-T%d" % g)
def test_one_evaluation_lies_in_the_restatements_error_band(geometry):
    C, layers, k, B, T = geometry
    hp, p, x, wav, t = Q.case_inputs(geometry)
    with torch.no_grad():
        spec = R.frontend(wav, hp, T)
    refs = {}
    for uncond in (False, True):
        sp = torch.full_like(spec, -1.0) if uncond else spec
        refs[uncond] = Q.errors(p, hp, x, sp, t)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16")
    eng = m.engine
    for fused in (2, 0):
        eng.set_option("fused_stack", fused)
        for uncond in (False, True):
            ref64, e = refs[uncond]
            got, _ = m(x, wav, t, sampling=uncond)
            mode = eng.launch_state()["mode"]
            # (the fused flavour needs a channel count that is a multiple of 128: elsewhere the per-phase bf16 kernels run)
            assert mode == ("fused_stack" if fused and C % 128 == 0 else "per_phase"), (geometry, fused, mode)
            err = got.cpu().double() - ref64
            r, mx = Q.rms(err), float(err.abs().max())
            r_ref, m_ref = e["f32"]
            _log(f"bf16_band[C={C},L={layers},k={k},B={B},T={T},{mode},uncond={int(uncond)}] rms {r:.3e} ref {r_ref:.3e} ratio {r / r_ref:.3f} "
                 f"max {mx:.3e} ref {m_ref:.3e} ratio {mx / m_ref:.3f}")
            assert torch.isfinite(got).all()
            assert 0.5 * r_ref <= r <= 1.15 * r_ref, (geometry, fused, uncond, r, r_ref)
            assert mx <= 2.0 * m_ref, (geometry, fused, uncond, mx, m_ref)


@pytest.mark.parametrize("ni", ["1", "2", "2b"])
def test_fused_stack_is_bit_identical_to_per_phase_launches(ni):
    """tests/bf16_cases.py for one block flavour ("2b": 128-frame blocks with blocked accumulation), the per-phase kernels
    pinned to the flavours the fused kernel is built from."""
    from tools import tuning_env
    blocked = "b" in ni
    ni = int(ni[0])
    env = tuning_env.env_with(tune__ksplit_max=1, tune__tile=3200 + ni, tune__pw_nw=2 * ni, tune__stack_fl=ni,
                              blocked_accumulation=2 if blocked else 1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_cases.py"), str(ni)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BF16_CASES ")][-1]
    recs = json.loads(line[len("BF16_CASES "):])
    assert len(recs) >= 5
    for rec in recs:
        assert rec["finite"] and rec["per_phase_mode"] == "per_phase", rec
        for run in rec["runs"]:
            assert run["timed_out"] == 0 and run["launches"] >= 1, rec
            assert run["kernel"].startswith(f"stack_kernel<{ni}>") and ", bf16, " in run["kernel"], rec
            assert run["mode"] == "fused_stack", rec                  # (the tail kernel is fp32 only)
            assert run["equal"], rec
            if run.get("chain"):
                assert run["tail_launches"] == 0, rec


def _chain_case(sampler):
    hp, p, x, wav, _ = Q.case_inputs(Q.CHAIN_GEOMETRY, timesteps=Q.CHAIN_STEPS)
    B, T = Q.CHAIN_GEOMETRY[3:]
    nz = torch.randn(Q.CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        spec = None if sampler == "generation_ddpm_x0" else R.frontend(wav, hp, T)
    return hp, p, x, wav, spec, nz


@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "generation_ddpm_x0"])
def test_chains(sampler):
    """An 8-step chain: the rms distance of the bf16 roll from the oracle's fp32 chain lies within 0.5 .. 1.5 x that of the
    restated bf16 chain (the two restatements stay within 0.8 .. 1.25 of each other: tests/test_bf16_cpu.py); the
    captured graph and plain launches, and two runs, give the same bits."""
    hp, p, x, wav, spec, nz = _chain_case(sampler)
    ref = chain_ref.sample_chain(p, hp, sampler, x, spec, nz, 0, w=0.5)
    d_ref = Q.rms(Q.sample_chain(Q.rne, None, p, hp, sampler, x, spec, nz, 0, w=0.5) - ref)
    m = make_model(hp, p, sampler=sampler, w=0.5, precision="bf16")
    wv = None if sampler == "generation_ddpm_x0" else wav
    got = m.sample(x, wv, noise=nz)[0]
    d = Q.rms(got.cpu() - ref)
    _log(f"bf16_chain[{sampler},{Q.CHAIN_STEPS} steps] rms distance from the fp32 chain {d:.3e} restated {d_ref:.3e} ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (sampler, d, d_ref)
    assert torch.equal(m.sample(x, wv, noise=nz)[0], got)                          # run against run
    assert torch.equal(m.sample(x, wv, noise=nz, use_graph=False)[0], got)         # captured against plain launches
    m.engine.set_option("fused_stack", 0)
    pp = m.sample(x, wv, noise=nz)[0]
    assert torch.equal(m.sample(x, wv, noise=nz, use_graph=False)[0], pp)
    # Philox noise drawn on the device: the same composition as under bf16x3
    a = m.sample(x, wv, seed=3)[0]
    assert torch.equal(m.sample(x, wv, seed=3)[0], a) and not torch.equal(m.sample(x, wv, seed=4)[0], a)


def test_windows_leave_shared_frames_bit_identical():
    """Long-form windows (32-frame windows overlapping by 16) under the mode: a frame two windows share holds the same bits
    in both after the chain."""
    from diffroll_amd import longform
    hp, p, _, _, _ = Q.case_inputs(Q.CHAIN_GEOMETRY, timesteps=4)
    HOP = 512
    L = 100 * HOP - 100
    plan = longform.plan_windows(L, HOP, T=32, overlap=16)
    assert plan.n >= 3
    g = torch.Generator().manual_seed(77)
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    noise = torch.randn(4, 1, 1, plan.T_c, 88, generator=g)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16")
    batch = longform.BatchPlan(plans=[plan], first=[0], marks=[], n=plan.n)
    for fused in (1, 0):
        m.engine.set_option("fused_stack", fused)
        win = m._sample_windows(batch, [wav], [x_T], [noise], 1, 0, 0, True, True).cpu()
        assert torch.isfinite(win).all()
        for b in range(plan.n - 1):
            assert torch.equal(win[b, plan.stride:], win[b + 1, :plan.overlap]), (fused, b)
    # ... and next to the exact path it is this mode's roll, not that one's
    mf = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    exact = mf._sample_windows(batch, [wav], [x_T], [noise], 1, 0, 0, True, True).cpu()
    d = Q.rms(win - exact)
    assert 1e-5 < d < 1e-2, d


def test_no_residue_between_precisions():
    """f32 -> bf16 -> bf16x3 -> f32 on ONE engine: the last roll is the first bit for bit, the bf16x3 roll in the middle that
    of a fresh engine; selecting one reduced precision never needs the other's packing."""
    hp, p, x, wav, spec, nz = _chain_case("cfdg_ddpm_x0")
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    first = m.sample(x, wav, noise=nz)[0].clone()
    m.precision = "bf16"
    low = m.sample(x, wav, noise=nz)[0].clone()
    m.precision = "bf16x3"
    split = m.sample(x, wav, noise=nz)[0].clone()
    m.precision = "f32"
    assert torch.equal(m.sample(x, wav, noise=nz)[0], first)
    fresh = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16x3")
    assert torch.equal(fresh.sample(x, wav, noise=nz)[0], split)
    assert float((split - first).abs().max()) <= 1e-5 < Q.rms(low - first)
    # an unknown mode is still refused, and the engine stays where it was
    from diffroll_amd import _cabi
    eng = m.engine
    assert eng.lib.dr_set_precision(eng.h, 3) == _cabi.DR_EINVAL
    assert torch.equal(m.sample(x, wav, noise=nz)[0], first)
