"""Child process of tests/test_gpu_f16.py: tests/bf16_cases.py's cases - every case of one block flavour of the fused
residual stack, the per-phase kernels pinned by the tune.* options the parent passes in DR_TEST_TUNE to the flavours the
fused kernel is built from - in precision "f16" (stack_kernel<FL, .., PREC = 4>): one reverse step under both block-to-XCD
mappings and a whole captured chain, fused against per-phase bit for bit.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bf16_cases import CASES  # noqa: E402  (its import installs the parent's tune.* options: tuning_env.install())
from oracle import diffroll_ref as R  # noqa: E402
from testlib import make_model  # noqa: E402


def main():
    ni = int(sys.argv[1])
    torch.cuda.set_device(torch.device("cuda", 0))
    out = []
    for (C, layers, k, B, Tn, sampler) in CASES[ni]:
        hp = dict(R.DEFAULT_HP)
        hp.update(residual_channels=C, residual_layers=layers, kernel_size=k, timesteps=6)
        p = R.synthetic_params(hp, seed=C + k)
        m = make_model(hp, p, sampler=sampler, w=0.5, precision="f16")
        g = torch.Generator().manual_seed(B * 1000 + Tn)
        wav = 0.1 * torch.randn(B, max(Tn * 512, 2048), generator=g)
        x = torch.randn(B, 1, Tn, 88, generator=g)
        z = torch.randn(B, 1, Tn, 88, generator=g)
        nz = torch.randn(hp["timesteps"], B, 1, Tn, 88, generator=g)
        eng = m.engine
        eng.set_option("fused_stack", 0)
        ref = m.reverse_diffusion(x, wav, 3, noise=z)[0]
        per_phase_mode = eng.launch_state()["mode"]
        chain_ref = m.sample(x, wav, noise=nz)[0]
        rec = {"case": [C, layers, k, B, Tn, sampler], "per_phase_mode": per_phase_mode, "finite": bool(torch.isfinite(ref).all()), "runs": []}
        for xcd in (1, 0):
            eng.set_option("fused_stack", 2)
            eng.set_option("fused_stack_xcd", xcd)
            eng.stack_status()
            n0 = eng.stack_launches
            eng.profile_enable(True)
            got = m.reverse_diffusion(x, wav, 3, noise=z)[0]
            _, _, _, kname = eng.profile_read_ex()
            eng.profile_enable(False)
            flag, _ = eng.stack_status()
            rec["runs"].append({"xcd": xcd, "timed_out": flag, "launches": eng.stack_launches - n0, "kernel": kname,
                                "mode": eng.launch_state()["mode"], "equal": bool(torch.equal(got, ref)),
                                "maxdiff": float((got - ref).abs().max())})
        eng.set_option("fused_stack_xcd", 1)
        t0 = eng.tail_launches
        got = m.sample(x, wav, noise=nz)[0]
        flag, _ = eng.stack_status()
        rec["runs"].append({"xcd": 1, "chain": True, "timed_out": flag, "launches": 1, "tail_launches": eng.tail_launches - t0,
                            "kernel": rec["runs"][0]["kernel"], "mode": eng.launch_state()["mode"],
                            "equal": bool(torch.equal(got, chain_ref)), "maxdiff": float((got - chain_ref).abs().max())})
        out.append(rec)
        del m
    print("F16_CASES " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
