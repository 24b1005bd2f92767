"""Start sweep (options "start_step" / "start_noise", hparams.sampling.strength, sample(init=...)): what refining a given
roll with the last part of the chain does, by strength.

    python tools/start_sweep.py [--strengths 0.1,0.2,...,1.0] [--flip 0.05] [--steps 0] [--chains 5] [--warmup 2]

On tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy) with its fixture's clips, for every strength s: the
frame-level TP / FP / FN against the label of (a) the proxy's own whole-chain roll refined - diffused to the start step of
strength s and denoised by the remaining steps - and (b) a copy of that roll with a fixed fraction of its cells flipped
(x -> 1 - x on a seeded mask) refined the same way; and ms per captured chain against the whole chain of the same build
(strength 1.0 is the whole chain plus the diffusion node).  The unrefined inputs are scored too.  The proxy task is too easy
for its counts to be a quality measure: this is a record of behaviour, not a claim.  One JSON line per strength, then a table.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--strengths", default="0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9,1.0", help="comma-separated s in (0, 1]")
    ap.add_argument("--flip", type=float, default=0.05, help="fraction of cells flipped in the damaged copy")
    ap.add_argument("--steps", type=int, default=0, help="n of a respaced chain (0: every step)")
    ap.add_argument("--chains", type=int, default=5, help="timed chains per cell")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from diffroll_amd import ClassifierFreeDiffRoll
    torch.cuda.set_device(0)
    golden = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(golden, "trained_small.npz"))
    B, Tn, _ = z["label"].shape
    x_T = torch.randn(B, 1, Tn, 88, generator=torch.Generator().manual_seed(int(z["noise_seed"])))      # the fixture's x_T
    wav, label = torch.from_numpy(z["wav"]), torch.from_numpy(z["label"])
    thr = float(z["frame_threshold"])
    m = ClassifierFreeDiffRoll.load_from_checkpoint(os.path.join(golden, "trained_small.ckpt"),
                                                    sampling={"type": "cfdg_ddpm_x0", "w": float(z["w"])},
                                                    device=torch.device("cuda", 0))
    m.hparams.sampling.steps = args.steps or None
    eng = m.engine

    def timed(fn):
        for _ in range(args.warmup):
            fn(True)
        before = eng.launch_state()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.chains):
            fn(False)
        t1.record()
        eng.finish()
        after = eng.launch_state()
        return t0.elapsed_time(t1) / args.chains, after["fallbacks"] == before["fallbacks"] and after["yields"] == before["yields"]

    own, _ = m.sample(x_T, wav, seed=1)                               # the proxy's own whole-chain roll
    whole_ms, whole_clean = timed(lambda check: m.sample(x_T, wav, seed=1, check=check))
    lab = label[:, :own.shape[2]].to(own.device).float()
    mask = torch.rand(own.shape, generator=torch.Generator().manual_seed(7)).to(own.device) < args.flip
    damaged = torch.where(mask, 1.0 - own, own)

    def counts(roll):
        return eng.frame_counts(roll[:, 0], lab, thr)

    print(json.dumps(dict(input="own", counts=counts(own), whole_chain_ms=whole_ms, clean=whole_clean)))
    print(json.dumps(dict(input="damaged", flipped=int(mask.sum()), counts=counts(damaged))))
    rows = []
    for s in [float(v) for v in args.strengths.split(",")]:
        m.hparams.sampling.strength = s
        start = m.start_step()
        steps = m.visited_steps()
        k = len(steps) if start < 0 else len(steps) - steps.index(start)
        a, _ = m.sample(None, wav, seed=2, init=own.cpu())
        b, _ = m.sample(None, wav, seed=2, init=damaged.cpu())
        ms, clean = timed(lambda check: m.sample(None, wav, seed=2, init=own, check=check))
        rec = dict(strength=s, start_step=start, steps_run=k, own=counts(a), damaged=counts(b), ms_per_chain=ms,
                   vs_whole_chain=ms / whole_ms, clean=clean and whole_clean)
        rows.append(rec)
        print(json.dumps(rec))
    print(f"\nwhole chain: {whole_ms:.2f} ms; own roll TP/FP/FN {counts(own)}; damaged copy ({args.flip:.0%} flipped) {counts(damaged)}")
    print("strength | start step | steps run | refined own TP/FP/FN | refined damaged TP/FP/FN | ms / chain | x whole chain")
    for r in rows:
        print(f"{r['strength']:8.2f} | {r['start_step']:10d} | {r['steps_run']:9d} | {'/'.join(map(str, r['own']))} | "
              f"{'/'.join(map(str, r['damaged']))} | {r['ms_per_chain']:9.2f} | {r['vs_whole_chain']:.3f}"
              f"{'' if r['clean'] else ' (fallback / yield!)'}")


if __name__ == "__main__":
    main()
