"""Clip sweep (option "x0_clip", hparams.sampling.x0_clip): what clamping the x0 prediction to the roll's range changes, and
what it costs, by guidance weight and chain length.

    python tools/clip_sweep.py [--w 0.5,2,5] [--steps 200,20] [--chains 50] [--warmup 3] [--rounds 3]

On tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy) with its fixture's clips and x_T, cfdg_ddpm_x0, for
every w and n and for x0_clip off and on: the frame-level TP / FP / FN of the thresholded roll against the held-out labels,
max |roll_clipped - roll_unclipped| from the same x_T and seed, how many roll cells cross the threshold between the two,
and the share of the unclipped roll outside [0, 1].  Time: ms per captured chain from device events around --chains x
(200 / n) chains (every window holds the same number of steps) after --warmup; the unclipped and the clipped chain of a cell
are timed in turn, --rounds rounds each, and the ratio is of the two medians; the spread of the unclipped chain's own
rounds (max / min) stands beside it, since a ratio inside that spread is no difference.  A cell whose launch state shows a
fallback or a yield prints no time.  One JSON line per (w, n), then a table.  The proxy's task is easy and its geometry a
toy one dominated by launches: a record of behaviour, not a quality or a speed claim.
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
    ap.add_argument("--w", default="0.5,2,5", help="comma-separated guidance weights")
    ap.add_argument("--steps", default="200,20", help="comma-separated n")
    ap.add_argument("--chains", type=int, default=50, help="timed chains per round at n = 200 (x 200 / n at a shorter chain)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from diffroll_amd import ClassifierFreeDiffRoll
    if not torch.cuda.is_available():
        raise SystemExit("clip_sweep measures on the GPU: no ROCm device visible")
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

    def run(w, n, clip):
        chains = max(1, args.chains * S // n)
        m.hparams.sampling.w, m.hparams.sampling.steps, m.hparams.sampling.x0_clip = w, n, clip
        roll, _ = m.sample(x_T, wav)                               # capture + instantiate, and the roll that is scored
        for _ in range(args.warmup):
            m.sample(x_T, wav)
        eng = m.engine
        before = eng.launch_state()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(chains):
            m.sample(x_T, wav, check=False)
        t1.record()
        eng.finish()
        after = eng.launch_state()
        clean = after["fallbacks"] == before["fallbacks"] and after["yields"] == before["yields"]
        return roll, t0.elapsed_time(t1) / chains, after["mode"], clean

    rows = []
    for w in [float(v) for v in args.w.split(",")]:
        for n in [int(v) for v in args.steps.split(",")]:
            ms = {0: [], 1: []}
            rolls, clean, mode = {}, True, None
            for _ in range(args.rounds):
                for clip in (0, 1):
                    rolls[clip], t, mode, ok = run(w, n, clip)
                    ms[clip].append(t)
                    clean = clean and ok
            lab = label[:, :rolls[0].shape[2]].to(rolls[0].device).float()
            counts = {clip: m.engine.frame_counts(rolls[clip][:, 0], lab, thr) for clip in (0, 1)}
            off, on = float(np.median(ms[0])), float(np.median(ms[1]))
            rec = dict(w=w, steps=n,
                       off=dict(zip(("tp", "fp", "fn"), counts[0])), on=dict(zip(("tp", "fp", "fn"), counts[1])),
                       max_abs_roll_difference=float((rolls[1] - rolls[0]).abs().max()),
                       cells_across_threshold=int(((rolls[1] > thr) != (rolls[0] > thr)).sum()),
                       unclipped_share_below_0=float((rolls[0] < 0).float().mean()),
                       unclipped_share_above_1=float((rolls[0] > 1).float().mean()),
                       ms_per_chain_off=off if clean else None, ms_per_chain_on=on if clean else None,
                       ratio_on_to_off=(on / off) if clean else None,
                       off_rounds_max_over_min=(max(ms[0]) / min(ms[0])) if clean else None, mode=mode, clean=clean)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    print("\nw | n | off TP/FP/FN | on TP/FP/FN | max |on - off| | cells across thr | off <0 / >1 | ms off | ms on | on / off | off max / min")
    for r in rows:
        ratio = "    -" if r["ratio_on_to_off"] is None else f"{r['ratio_on_to_off']:5.3f}"
        spread = "    -" if r["off_rounds_max_over_min"] is None else f"{r['off_rounds_max_over_min']:5.3f}"
        print(f"{r['w']:3g} | {r['steps']:4d} | {r['off']['tp']}/{r['off']['fp']}/{r['off']['fn']} | {r['on']['tp']}/{r['on']['fp']}/{r['on']['fn']} | "
              f"{r['max_abs_roll_difference']:.3e} | {r['cells_across_threshold']} | {r['unclipped_share_below_0']:.3f} / {r['unclipped_share_above_1']:.3f} | "
              f"{ms_text(r['ms_per_chain_off'])} | {ms_text(r['ms_per_chain_on'])} | {ratio} | {spread}")
    same = all(r["off"] == r["on"] for r in rows)
    print("\nthe proxy's counts " + ("do not depend on the option in any cell" if same else "depend on the option in at least one cell"))


def ms_text(ms):
    """A cell whose chains met a fallback or a yield has no time."""
    return "        -" if ms is None else f"{ms:9.2f}"


if __name__ == "__main__":
    main()
