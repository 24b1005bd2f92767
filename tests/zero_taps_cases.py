"""Child process of tests/test_gpu_zero_taps.py: the lab option "zero_taps" (csrc/zero_taps.h: fp32 128-frame conv blocks issue
no MFMAs for an edge tap whose window of the block's first / last 32-frame tile is all zero padding) on and off, with the
per-phase kernels pinned by the parent (DR_TEST_TUNE, tools/tuning_env.py) to the flavours the fused 128-frame kernel is built
from - 32x32 MFMA conv tiles of four frame tiles, no split-K, the four-tile 1x1 - and the fused kernel to that flavour.  Every
network has four layers, so that layer 3 is a d = 8 layer: the only dilation at which k = 9 has such a tap.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import probe_ref as P  # noqa: E402
from oracle import diffroll_ref as R  # noqa: E402
from testlib import make_model  # noqa: E402
from tools import tuning_env  # noqa: E402

tuning_env.install()        # the parent pins the kernel flavours of this process (DR_TEST_TUNE)

# (k, T) of the per-phase cases: C = 64, 4 layers, B = 2, a 3-step guided chain
PER_PHASE = [
    (9, 125),       # both edges: tap 0 of tile 0 and tap 8 of tile 3
    (9, 128),       # the last tile is full: tap 8 reads [128, 160)
    (9, 97),        # one valid frame in tile 3
    (9, 96),        # tile 3 holds no frame
    (9, 60),        # tiles 2 and 3 hold no frame
    (9, 250),       # two frame tiles per clip: the leading edge in the first alone, the trailing edge in the second alone
    (15, 125),      # four all-padding taps per edge: the kernel leaves out one
    (3, 125),       # control: the outer taps sit at -+8 frames, nothing is left out
]
FUSED = (512, 4, 9, 16, 125, "cfdg_ddpm_x0")
STEPS = 3


def on_off(eng, fn):
    """fn() under zero_taps = 1 and = 0 (the engine is left at its default, 1)."""
    eng.set_option("zero_taps", 1)
    on = fn()
    eng.set_option("zero_taps", 0)
    off = fn()
    eng.set_option("zero_taps", 1)
    return on, off


def per_phase(k, Tn):
    C, layers, B = 64, 4, 2
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=C, residual_layers=layers, kernel_size=k, timesteps=STEPS)
    p = R.synthetic_params(hp, seed=C + k)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    g = torch.Generator().manual_seed(B * 1000 + Tn)
    wav = 0.1 * torch.randn(B, Tn * 512, generator=g)
    x = torch.randn(B, 1, Tn, 88, generator=g)
    nz = torch.randn(STEPS, B, 1, Tn, 88, generator=g)
    m.engine.set_option("fused_stack", 0)
    on, off = on_off(m.engine, lambda: m.sample(x, wav, noise=nz)[0])
    mode = m.engine.launch_state()["mode"]
    with torch.no_grad():
        want = R.sample_chain(p, hp, "cfdg_ddpm_x0", x, wav, nz, w=0.5)
    rec = {"case": [k, Tn], "mode": mode, "roll_equal": bool(torch.equal(on, off)),
           "on_vs_oracle": float((on.cpu() - want).abs().max()), "off_vs_oracle": float((off.cpu() - want).abs().max())}
    del m
    # layer 3's gated activation g, every channel, frame and clip, through tests/probe_ref.py's probe network (the layers
    # around it pass their input through; the read-out is exact)
    case = (C, layers, k, 2, 4, 3, B, Tn)
    hpp, _, xp, wavp, t = P.inputs(case)
    net = P.network(case, "conv")
    mp = make_model(hpp, net)
    got = {}
    for zt in (1, 0):
        def run(params):
            mp.load_state_dict(params)
            mp.engine.set_option("fused_stack", 0)
            mp.engine.set_option("zero_taps", zt)
            return mp(xp, wavp, t)[0]
        got[zt] = P.read(run, case, net)
    mp.engine.set_option("zero_taps", 1)
    rec["g_equal"] = bool(torch.equal(got[1], got[0]))
    rec["g_finite_nonzero"] = bool(torch.isfinite(got[1]).all()) and bool((got[1] != 0).any())
    del mp
    return rec


def fused():
    C, layers, k, B, Tn, sampler = FUSED
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=C, residual_layers=layers, kernel_size=k, timesteps=6)
    p = R.synthetic_params(hp, seed=C + k)
    m = make_model(hp, p, sampler=sampler, w=0.5)
    g = torch.Generator().manual_seed(B * 1000 + Tn)
    wav = 0.1 * torch.randn(B, Tn * 512, generator=g)
    x = torch.randn(B, 1, Tn, 88, generator=g)
    z = torch.randn(B, 1, Tn, 88, generator=g)
    eng = m.engine
    eng.set_option("fused_stack", 0)
    ref_on, ref_off = on_off(eng, lambda: m.reverse_diffusion(x, wav, 3, noise=z)[0])
    rec = {"case": list(FUSED), "per_phase_equal": bool(torch.equal(ref_on, ref_off)), "runs": []}
    for xcd in (1, 0):
        eng.set_option("fused_stack", 2)
        eng.set_option("fused_stack_xcd", xcd)
        eng.stack_status()
        n0 = eng.stack_launches
        eng.profile_enable(True)
        on, off = on_off(eng, lambda: m.reverse_diffusion(x, wav, 3, noise=z)[0])
        _, _, _, kname = eng.profile_read_ex()
        eng.profile_enable(False)
        flag, _ = eng.stack_status()
        rec["runs"].append({"xcd": xcd, "timed_out": flag, "launches": eng.stack_launches - n0, "kernel": kname.split(" ")[0],
                            "on_equals_per_phase": bool(torch.equal(on, ref_on)), "off_equals_per_phase": bool(torch.equal(off, ref_off)),
                            "on_equals_off": bool(torch.equal(on, off))})
    eng.set_option("fused_stack_xcd", 1)
    st = eng.launch_state()
    rec["fallbacks"], rec["yields"] = st["fallbacks"], st["yields"]
    sch = R.schedule(hp["beta_start"], hp["beta_end"], hp["timesteps"])
    with torch.no_grad():
        want = R.reverse_step(p, hp, sch, sampler, x, R.frontend(wav, hp, Tn), 3, z, 0.5)
    rec["vs_oracle"] = float((ref_on.cpu() - want).abs().max())
    return rec


def main():
    torch.cuda.set_device(torch.device("cuda", 0))
    out = {"per_phase": [per_phase(k, Tn) for k, Tn in PER_PHASE], "fused": fused()}
    print("ZERO_TAPS_CASES " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
