"""Solver sweep (option "solver_order", hparams.sampling.solver_order): what the second-order multistep update changes
at a given number of steps.

    python tools/solver_sweep.py [--steps 10,20,50] [--noise 0,1] [--chains 5] [--warmup 2]

On tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy) with its fixture's clips and x_T, for every n and
for orders 1 and 2: ms per captured chain, max and mean |roll_n - roll_200| against the 200-step order-1 chain from the same
x_T, and the frame-level TP / FP / FN of the thresholded roll.  The chains are deterministic and share one ODE solution, so
the distance to the 200-step chain is a discretisation error that needs no dataset; it is not a quality measure, and the
proxy task is too easy for its counts to be one.  One JSON line per (n, order), then a table.

--noise 0,1 adds the stochastic cells (option "solver_noise", hparams.sampling.solver_noise = 1) at every n < 200: ms per
captured chain and its ratio to the deterministic chain of the same n and order, the TP / FP / FN of one draw and of the mean
of 8 draws (draws = 8, one chain), and the per-cell spread of those draws (ensemble.aggregate: the standard deviation over the
draws of each roll cell, averaged over the cells).  A stochastic chain has no common ODE solution: no distance to the
200-step chain is printed for it.  A cell whose launch state shows a fallback or a yield prints no time.
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
    ap.add_argument("--steps", default="10,20,50", help="comma-separated n")
    ap.add_argument("--noise", default="0", help="comma-separated values of solver_noise (0: the deterministic cells, 1: the stochastic ones)")
    ap.add_argument("--chains", type=int, default=5, help="timed chains per cell")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from diffroll_amd import ClassifierFreeDiffRoll
    torch.cuda.set_device(0)
    golden = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(golden, "trained_small.npz"))
    hp = json.loads(str(z["hp"]))
    S, (B, Tn, _) = int(hp["timesteps"]), z["label"].shape
    x_T = torch.randn(B, 1, Tn, 88, generator=torch.Generator().manual_seed(int(z["noise_seed"])))      # the fixture's x_T
    wav, label = torch.from_numpy(z["wav"]), torch.from_numpy(z["label"])
    thr = float(z["frame_threshold"])
    m = ClassifierFreeDiffRoll.load_from_checkpoint(os.path.join(golden, "trained_small.ckpt"),
                                                    sampling={"type": "cfdg_ddpm_x0", "w": float(z["w"])},
                                                    device=torch.device("cuda", 0))

    def run(n, order, noise=0):
        m.hparams.sampling.steps, m.hparams.sampling.solver_order, m.hparams.sampling.solver_noise = n, order, noise
        roll, _ = m.sample(x_T, wav)                               # capture + instantiate, and the roll that is scored
        for _ in range(args.warmup):
            m.sample(x_T, wav)
        eng = m.engine
        before = eng.launch_state()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.chains):
            m.sample(x_T, wav, check=False)
        t1.record()
        eng.finish()
        after = eng.launch_state()
        clean = after["fallbacks"] == before["fallbacks"] and after["yields"] == before["yields"]
        return roll, t0.elapsed_time(t1) / args.chains, after["mode"], clean

    noises = sorted({int(v) for v in args.noise.split(",")})
    if not set(noises) <= {0, 1}:
        ap.error("--noise takes 0 and / or 1")
    base, base_ms, _, _ = run(S, 1)
    lab = label[:, :base.shape[2]].to(base.device) > 0.5
    rows = []
    if 0 in noises:
        for n in [S] + [int(v) for v in args.steps.split(",")]:
            for order in (1, 2):
                roll, ms, mode, clean = (base, base_ms, None, True) if (n, order) == (S, 1) else run(n, order)
                d = (roll - base).abs()
                tp, fp, fn = m.engine.frame_counts(roll[:, 0], lab.float(), thr)
                rec = dict(steps=n, order=order, ms_per_chain=ms if clean else None, max_abs_vs_200=float(d.max()),
                           mean_abs_vs_200=float(d.mean()), tp=tp, fp=fp, fn=fn, mode=mode, clean=clean)
                rows.append(rec)
                print(json.dumps(rec))
        print("\nn | order | ms / chain | max |roll - roll_200| | mean | proxy TP/FP/FN")
        for r in rows:
            print(f"{r['steps']:4d} | {r['order']} | {ms_text(r['ms_per_chain'])} | {r['max_abs_vs_200']:.3e} | {r['mean_abs_vs_200']:.3e} | "
                  f"{r['tp']}/{r['fp']}/{r['fn']}")
    if 1 not in noises:
        return
    # the stochastic cells: the draws of a clip start from the clip's x_T and differ through the noise alone
    from diffroll_amd import ensemble
    D, srows = 8, []
    for n in [int(v) for v in args.steps.split(",")]:
        for order in (1, 2):
            # deterministic and stochastic chains timed in turn, three rounds each: the ratio is of the two medians
            ms_d, ms_s, clean = [], [], True
            for _ in range(3):
                for noise, acc in ((0, ms_d), (1, ms_s)):
                    roll, ms, mode, ok = run(n, order, noise)
                    acc.append(ms)
                    clean = clean and ok
            tp, fp, fn = m.engine.frame_counts(roll[:, 0], lab.float(), thr)      # (the last round's stochastic roll)
            draws, _ = m.sample(x_T.repeat(D, 1, 1, 1), wav, draws=D)
            mean, _, spread = ensemble.aggregate(draws, D, thr)
            mtp, mfp, mfn = m.engine.frame_counts(mean[:, 0].contiguous(), lab.float(), thr)
            ms, det = float(np.median(ms_s)), float(np.median(ms_d))
            rec = dict(steps=n, order=order, solver_noise=1, ms_per_chain=ms if clean else None,
                       ms_per_deterministic_chain=det if clean else None, ratio_to_deterministic=(ms / det) if clean else None,
                       tp=tp, fp=fp, fn=fn, mean8_tp=mtp, mean8_fp=mfp, mean8_fn=mfn, spread=float(spread.mean()), mode=mode, clean=clean)
            srows.append(rec)
            print(json.dumps(rec))
    print("\nstochastic (solver_noise = 1)\nn | order | ms / chain | x deterministic | one draw TP/FP/FN | mean of 8 TP/FP/FN | spread")
    for r in srows:
        ratio = "    -" if r["ratio_to_deterministic"] is None else f"{r['ratio_to_deterministic']:5.3f}"
        print(f"{r['steps']:4d} | {r['order']} | {ms_text(r['ms_per_chain'])} | {ratio} | {r['tp']}/{r['fp']}/{r['fn']} | "
              f"{r['mean8_tp']}/{r['mean8_fp']}/{r['mean8_fn']} | {r['spread']:.3e}")


def ms_text(ms):
    """A cell whose chains met a fallback or a yield has no time."""
    return "        -" if ms is None else f"{ms:9.2f}"


if __name__ == "__main__":
    main()
