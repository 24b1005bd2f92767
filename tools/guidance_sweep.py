"""Guidance interval (options "guidance_t_min" / "guidance_t_max", hparams.sampling.guidance_interval): chain time against
the share of guided steps.

    python tools/guidance_sweep.py [--reps 5] [--warmup 1] [--out profiles/guidance_interval_sweep.txt]

At config 2's geometry (16 clips of 125 frames) and config 6's (4 clips of 640 frames), k = 9, 15 layers, C = 512,
cfdg_ddpm_x0 w = 0.5, 200 steps, Philox noise, synthetic weights: the captured chain (Engine.sample, check=True: host clock
around a call that returns synchronised) for intervals centred in the chain that guide 100 %, 60 %, 40 %, 20 % of the steps,
and 0 % (w = 0: the empty interval).  The cells alternate rep by rep after `warmup` untimed rounds; each timed call is
preceded by an untimed one of the same interval, which captures (the engine keeps one captured chain), so the timed call
replays.  A timed region in which the engine yielded or healed is dropped, not listed.  Next to the times: the launch mode
of a guided and of an unguided step (dr_launch_state after a dr_step of each kind), and the expectation from the code -
guided steps x (per-step time of the 100 % row) + unguided steps x (per-step time of the 0 % row) - with each mixed row's
residual against it.  One JSON line per cell on stdout, the table into --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

HOP, S, W = 512, 200, 0.5
GEOMETRIES = {"config 2": (16, 125), "config 6": (4, 640)}
SHARES = (100, 60, 40, 20, 0)


def interval_for(share):
    """(lo, hi) guiding share % of the S steps, centred; None for 0 % (run with w = 0)."""
    n = S * share // 100
    if n == 0:
        return None
    lo = (S - n) // 2
    return lo, lo + n - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_interval_sweep.txt"))
    args = ap.parse_args()
    from oracle import diffroll_ref as R
    from diffroll_amd import ClassifierFreeDiffRoll

    lines = [f"guidance interval sweep: cfdg_ddpm_x0 w = {W}, {S} steps, C = 512, L = 15, k = 9, captured chain, Philox noise;",
             f"median [min .. max] ms of {args.reps} timed chains per cell after {args.warmup} warm-up round(s), cells alternating;",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    for name, (B, T) in GEOMETRIES.items():
        hp = dict(R.DEFAULT_HP)
        hp.update(residual_channels=512, residual_layers=15, kernel_size=9, timesteps=S)
        m = ClassifierFreeDiffRoll(
            residual_channels=512, unconditional=False, condition="fixed", n_mels=hp["n_mels"], norm_args=[0, 1, "imagewise"],
            residual_layers=15, kernel_size=9, dilation_base=2, dilation_bound=4,
            spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=HOP, n_mels=hp["n_mels"], f_min=0, f_max=8000, center=True,
                           normalized=True, pad_mode="reflect"),
            timesteps=S, sampling={"type": "cfdg_ddpm_x0", "w": W})
        m.load_state_dict(R.synthetic_params(hp, seed=3))
        eng = m.engine
        g = torch.Generator().manual_seed(1)
        eng.frontend(0.1 * torch.randn(B, T * HOP, generator=g), T, return_spec=False)
        x = torch.randn(B, T, 88, generator=g).to(eng.device)

        def run(share):
            iv = interval_for(share)
            eng.set_guidance_interval(*(iv or (0, -1)))
            eng.sample("cfdg_ddpm_x0", x.clone(), None, W if iv else 0.0, 7, 0, True, True)

        def step_mode(guided):
            eng.set_guidance_interval(0, -1)
            eng.step("cfdg_ddpm_x0", x.clone(), None, 100, W if guided else 0.0)
            eng.finish()
            return eng.launch_state()["mode"]

        modes = (step_mode(True), step_mode(False))
        runs = {s: [] for s in SHARES}
        for rep in range(args.warmup + args.reps):
            for s in SHARES:
                run(s)                                  # captures (untimed)
                before = eng.launch_state()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(s)
                ms = 1e3 * (time.perf_counter() - t0)
                after = eng.launch_state()
                clean = after["yields"] == before["yields"] and after["fallbacks"] == before["fallbacks"]
                if rep >= args.warmup and clean:
                    runs[s].append(ms)
        eng.set_guidance_interval(0, -1)
        med = {s: statistics.median(v) for s, v in runs.items() if v}
        lines.append(f"{name}: B = {B} clips x T = {T} frames; a guided step launches {modes[0]}, an unguided step {modes[1]}")
        if 100 in med and 0 in med:
            per_g, per_u = med[100] / S, med[0] / S
            lines.append(f"  per step: guided {per_g:.3f} ms (100 % row), unguided {per_u:.3f} ms (0 % row)")
        lines.append("  guided steps | interval   | ms per chain [min .. max]      | network evaluations | expected ms | residual")
        for s in SHARES:
            if s not in med:
                lines.append(f"  {s:3d} %        | (every timed region saw a yield or a heal: no line)")
                continue
            iv, n = interval_for(s), S * s // 100
            exp = n * per_g + (S - n) * per_u if 100 in med and 0 in med else float("nan")
            rec = dict(geometry=name, B=B, T=T, share=s, interval=iv, ms=med[s], ms_min=min(runs[s]), ms_max=max(runs[s]),
                       kept=len(runs[s]), evaluations=B * (S + n), expected_ms=exp, modes=modes)
            print(json.dumps(rec))
            lines.append(f"  {s:3d} % ({n:3d})  | {str(list(iv)) if iv else 'w = 0':10s} | {med[s]:8.1f} [{min(runs[s]):8.1f} .. {max(runs[s]):8.1f}] "
                         f"| {B * (S + n):6d}              | {exp:8.1f}    | {med[s] - exp:+7.1f} ({100 * (med[s] - exp) / exp:+.1f} %)")
        lines.append("")
        del m, eng
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
