"""Precision "f16" (DR_PRECISION_F16, include/diffroll_amd.h) on the GPU: one v_mfma_f32_32x32x16_f16 per K step in the two
hot contractions, operands rounded once to IEEE binary16 (nearest even, subnormals kept), fp32 accumulation.

As under bf16 the network is not held element-wise to a restatement (tests/test_f16_cpu.py says why, and shows that the
bands used here discriminate): with e = got - float64 network and e_ref the error of the fp32-accumulated restatement
(tests/f16_ref.py), 0.5 rms(e_ref) <= rms(e) <= 1.15 rms(e_ref) and max|e| <= 2 max|e_ref|.  The lower bound proves that
the mode is engaged (the exact path lies three orders of magnitude below); the upper ones refuse rounding toward zero
(2.5 - 3.6 x in rms), bf16 (7.4 - 8.5 x) and - on the subnormal-weight case - an MFMA that flushes subnormal operands
(several hundred x).  That is true of the network, not of one contraction: SINGLE layers of the mode are held element by
element in tests/test_gpu_layer_probe.py, which sees the one-element faults these bands let through
(tests/test_layer_probe_cpu.py).  What IS held bit for bit here: fused against per-phase launches, captured against plain chains, run
against run, shared window frames, and the other precisions after a visit to this one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chain_ref
import f16_ref as H
from oracle import diffroll_ref as R
from testlib import ckpt_path, load_trained, make_model, trained_noise

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _log(line):
    print(line)
    log = os.environ.get("DR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def _band(tag, inputs, geometry, unconds):
    """One evaluation of `inputs` under f16, fused (where C % 128 == 0) and per-phase, in the restatement's band."""
    C, layers, k, B, T = geometry
    hp, p, x, wav, t = inputs
    with torch.no_grad():
        spec = R.frontend(wav, hp, T)
    refs = {}
    for uncond in unconds:
        sp = torch.full_like(spec, -1.0) if uncond else spec
        refs[uncond] = H.errors(p, hp, x, sp, t)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="f16")
    eng = m.engine
    for fused in (2, 0):
        eng.set_option("fused_stack", fused)
        for uncond in unconds:
            ref64, e = refs[uncond]
            got, _ = m(x, wav, t, sampling=uncond)
            mode = eng.launch_state()["mode"]
            # (the fused flavour needs a channel count that is a multiple of 128: elsewhere the per-phase f16 kernels run)
            assert mode == ("fused_stack" if fused and C % 128 == 0 else "per_phase"), (geometry, fused, mode)
            err = got.cpu().double() - ref64
            r, mx = H.rms(err), float(err.abs().max())
            r_ref, m_ref = e["f32"]
            _log(f"{tag}[C={C},L={layers},k={k},B={B},T={T},{mode},uncond={int(uncond)}] rms {r:.3e} ref {r_ref:.3e} ratio {r / r_ref:.3f} "
                 f"max {mx:.3e} ref {m_ref:.3e} ratio {mx / m_ref:.3f}")
            assert torch.isfinite(got).all()
            assert 0.5 * r_ref <= r <= 1.15 * r_ref, (geometry, fused, uncond, r, r_ref)
            assert mx <= 2.0 * m_ref, (geometry, fused, uncond, mx, m_ref)


@pytest.mark.parametrize("geometry", H.GEOMETRIES, ids=lambda g: "C%d-L%d-k%d-B%d-T%d" % g)
def test_one_evaluation_lies_in_the_restatements_error_band(geometry):
    _band("f16_band", H.case_inputs(geometry), geometry, (False, True))


@pytest.mark.parametrize("geometry", H.SUBNORMAL_GEOMETRIES, ids=lambda g: "C%d-L%d-k%d-B%d-T%d" % g)
def test_subnormal_weights_are_kept(geometry):
    """38 % of the output projections' weights are binary16 subnormals (tests/f16_ref.py: subnormal_inputs): the result lies
    in the band of the IEEE restatement, which a packing, a conversion or an MFMA that flushes them misses by a factor of
    several hundred (tests/test_f16_cpu.py)."""
    _band("f16_subnormal", H.subnormal_inputs(geometry), geometry, (False,))


@pytest.mark.parametrize("ni", ["1", "2", "2b"])
def test_fused_stack_is_bit_identical_to_per_phase_launches(ni):
    """tests/f16_cases.py for one block flavour ("2b": 128-frame blocks with blocked accumulation), the per-phase kernels
    pinned to the flavours the fused kernel is built from."""
    from tools import tuning_env
    blocked = "b" in ni
    ni = int(ni[0])
    env = tuning_env.env_with(tune__ksplit_max=1, tune__tile=3200 + ni, tune__pw_nw=2 * ni, tune__stack_fl=ni,
                              blocked_accumulation=2 if blocked else 1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "f16_cases.py"), str(ni)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("F16_CASES ")][-1]
    recs = json.loads(line[len("F16_CASES "):])
    assert len(recs) >= 5
    for rec in recs:
        assert rec["finite"] and rec["per_phase_mode"] == "per_phase", rec
        for run in rec["runs"]:
            assert run["timed_out"] == 0 and run["launches"] >= 1, rec
            assert run["kernel"].startswith(f"stack_kernel<{ni}>") and ", f16, " in run["kernel"], rec
            assert (", blocked accumulation" in run["kernel"]) == (blocked or ni == 1), rec
            assert run["mode"] == "fused_stack", rec                  # (the tail kernel is fp32 only)
            assert run["equal"], rec
            if run.get("chain"):
                assert run["tail_launches"] == 0, rec


def _chain_case(sampler):
    hp, p, x, wav, _ = H.case_inputs(H.CHAIN_GEOMETRY, timesteps=H.CHAIN_STEPS)
    B, T = H.CHAIN_GEOMETRY[3:]
    nz = torch.randn(H.CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        spec = None if sampler == "generation_ddpm_x0" else R.frontend(wav, hp, T)
    return hp, p, x, wav, spec, nz


@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "generation_ddpm_x0"])
def test_chains(sampler):
    """An 8-step chain: the rms distance of the f16 roll from the oracle's fp32 chain lies within 0.5 .. 1.5 x that of the
    restated f16 chain (the two restatements stay within 0.8 .. 1.25 of each other: tests/test_f16_cpu.py); the captured
    graph and plain launches, and two runs, give the same bits."""
    hp, p, x, wav, spec, nz = _chain_case(sampler)
    ref = chain_ref.sample_chain(p, hp, sampler, x, spec, nz, 0, w=0.5)
    d_ref = H.rms(H.sample_chain(H.rne, None, p, hp, sampler, x, spec, nz, 0, w=0.5) - ref)
    m = make_model(hp, p, sampler=sampler, w=0.5, precision="f16")
    wv = None if sampler == "generation_ddpm_x0" else wav
    got = m.sample(x, wv, noise=nz)[0]
    d = H.rms(got.cpu() - ref)
    _log(f"f16_chain[{sampler},{H.CHAIN_STEPS} steps] rms distance from the fp32 chain {d:.3e} restated {d_ref:.3e} ratio {d / d_ref:.3f}")
    assert 0.5 * d_ref <= d <= 1.5 * d_ref, (sampler, d, d_ref)
    assert torch.equal(m.sample(x, wv, noise=nz)[0], got)                          # run against run
    assert torch.equal(m.sample(x, wv, noise=nz, use_graph=False)[0], got)         # captured against plain launches
    m.engine.set_option("fused_stack", 0)
    pp = m.sample(x, wv, noise=nz)[0]
    assert torch.equal(m.sample(x, wv, noise=nz, use_graph=False)[0], pp)
    # Philox noise drawn on the device: the same composition as under the other precisions
    a = m.sample(x, wv, seed=3)[0]
    assert torch.equal(m.sample(x, wv, seed=3)[0], a) and not torch.equal(m.sample(x, wv, seed=4)[0], a)


def test_windows_leave_shared_frames_bit_identical():
    """Long-form windows (32-frame windows overlapping by 16) under the mode: a frame two windows share holds the same bits
    in both after the chain; next to the exact path the roll is this mode's (rms 1e-6 .. 1e-3: a tenth of bf16's band)."""
    from diffroll_amd import longform
    hp, p, _, _, _ = H.case_inputs(H.CHAIN_GEOMETRY, timesteps=4)
    HOP = 512
    L = 100 * HOP - 100
    plan = longform.plan_windows(L, HOP, T=32, overlap=16)
    assert plan.n >= 3
    g = torch.Generator().manual_seed(77)
    wav = 0.1 * torch.randn(L, generator=g)
    x_T = torch.randn(1, 1, plan.T_c, 88, generator=g)
    noise = torch.randn(4, 1, 1, plan.T_c, 88, generator=g)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="f16")
    batch = longform.BatchPlan(plans=[plan], first=[0], marks=[], n=plan.n)
    for fused in (1, 0):
        m.engine.set_option("fused_stack", fused)
        win = m._sample_windows(batch, [wav], [x_T], [noise], 1, 0, 0, True, True).cpu()
        assert torch.isfinite(win).all()
        for b in range(plan.n - 1):
            assert torch.equal(win[b, plan.stride:], win[b + 1, :plan.overlap]), (fused, b)
    mf = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    exact = mf._sample_windows(batch, [wav], [x_T], [noise], 1, 0, 0, True, True).cpu()
    d = H.rms(win - exact)
    _log(f"f16_windows[32-frame windows, overlap 16, 4 steps] rms distance from the exact path's roll {d:.3e}")
    assert 1e-6 < d < 1e-3, d


def test_no_residue_between_precisions():
    """f32 -> f16 -> bf16 -> bf16x3 -> f32 on ONE engine: the last roll is the first bit for bit, the bf16 and bf16x3 rolls
    in the middle those of fresh engines (f16 and bf16 share the 16-bit activation buffers; each mode has its own packing);
    f16 is closer to the exact roll than bf16; unknown modes - the reserved 3 among them - are refused and change nothing."""
    hp, p, x, wav, spec, nz = _chain_case("cfdg_ddpm_x0")
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    first = m.sample(x, wav, noise=nz)[0].clone()
    rolls = {}
    for mode in ("f16", "bf16", "bf16x3"):
        m.precision = mode
        rolls[mode] = m.sample(x, wav, noise=nz)[0].clone()
    m.precision = "f32"
    assert torch.equal(m.sample(x, wav, noise=nz)[0], first)
    for mode in ("bf16", "bf16x3"):
        fresh = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision=mode)
        assert torch.equal(fresh.sample(x, wav, noise=nz)[0], rolls[mode]), mode
    d16, db = H.rms(rolls["f16"] - first), H.rms(rolls["bf16"] - first)
    _log(f"f16_residue[8 steps] rms distance from the f32 roll: f16 {d16:.3e} bf16 {db:.3e}")
    assert 0 < d16 < db, (d16, db)
    from diffroll_amd import _cabi
    eng = m.engine
    for bad in (3, 5, -1):
        assert eng.lib.dr_set_precision(eng.h, bad) == _cabi.DR_EINVAL, bad
    assert torch.equal(m.sample(x, wav, noise=nz)[0], first)


def test_trained_checkpoint_transcription(golden_dir):
    """tests/golden/trained_small.ckpt under f16 (after tests/test_trained_golden.py's first GPU test): the frame counts are
    the reference's, the thresholded roll is the f32 engine's, and the roll is no further from the f32 engine's than bf16's
    is - a relation between two measured distances, not a number."""
    from diffroll_amd import ClassifierFreeDiffRoll
    g = load_trained(golden_dir)
    x_T, noise = trained_noise(g)
    wav, label = torch.from_numpy(g["wav"]), torch.from_numpy(g["label"])
    rolls = {}
    for precision in ("f32", "bf16", "f16"):
        m = ClassifierFreeDiffRoll.load_from_checkpoint(ckpt_path(golden_dir), precision=precision)
        rolls[precision] = m.sample(x_T, wav, noise=noise)[0].cpu()
    thr = float(g["frame_threshold"])
    assert torch.equal(rolls["f16"] > thr, rolls["f32"] > thr)                        # identical thresholded roll
    assert np.array_equal(rolls["f16"].numpy() > thr, g["cfdg_roll"] > thr)
    out = m.test_step({"frame": label, "audio": wav, "x_T": x_T, "noise": noise}, 1)           # (m: the f16 model)
    assert (out["tp"], out["fp"], out["fn"]) == (int(g["tp"]), int(g["fp"]), int(g["fn"]))
    d16 = float((rolls["f16"] - rolls["f32"]).abs().max())
    db = float((rolls["bf16"] - rolls["f32"]).abs().max())
    _log(f"f16_trained[trained_small.ckpt, 200 steps] max distance from the f32 roll: f16 {d16:.3e} bf16 {db:.3e}")
    assert d16 <= db, (d16, db)
