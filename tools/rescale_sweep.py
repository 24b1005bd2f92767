"""Rescale sweep (option "cfg_rescale", hparams.sampling.cfg_rescale): what the guidance rescale changes on the trained proxy,
alone and beside the clamp and the thresholding, and what its launches cost on the geometry that fuses.

    python tools/rescale_sweep.py [--w 0.5,2,5] [--steps 200,20] [--phi 0.7] [--chains 3] [--warmup 1] [--rounds 2] [--forms a,b,c,d]

Part 1, on tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy) with its fixture's clips and x_T,
cfdg_ddpm_x0, for every w and n and for the chain alone, with x0_clip and with x0_clip + x0_threshold 0.995: the frame-level
TP / FP / FN against the held-out labels at phi = 0 and at --phi, and max |roll_phi - roll_0| from the same x_T and seed.  A
record of behaviour, not a quality claim.  The proxy's geometry does not fuse; no time is taken there.

Part 2, on the geometry that fuses - bench.py's config 2 (C = 512, 15 layers, 16 guided clips x 125 frames, random-init
weights, 200 steps, w = 3): ms per captured chain from device events around --chains chains after --warmup, of
    (a) the plain chain (the option off: the tail kernel), (b) cfg_rescale --phi, (c) x0_clip, (d) x0_clip + x0_threshold 0.995,
timed in turn from this one process, --rounds runs per cell; medians, and each cell's own spread over its runs (max / min),
since a ratio inside that spread is no difference.  --forms a times the option-off chain alone: run from a checkout of the
parent commit it gives the parent's time for the same cell.  A chain whose launch state shows a fallback or a yield prints
no time.  JSON lines, then tables.
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

COMPANIONS = {"alone": dict(x0_clip=None, x0_threshold=None), "clip": dict(x0_clip=1, x0_threshold=None),
              "clip+threshold": dict(x0_clip=1, x0_threshold=0.995)}


def proxy_part(args):
    from diffroll_amd import ClassifierFreeDiffRoll
    golden = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(golden, "trained_small.npz"))
    B, Tn, _ = z["label"].shape
    x_T = torch.randn(B, 1, Tn, 88, generator=torch.Generator().manual_seed(int(z["noise_seed"])))      # the fixture's x_T
    wav, label = torch.from_numpy(z["wav"]), torch.from_numpy(z["label"])
    thr = float(z["frame_threshold"])
    m = ClassifierFreeDiffRoll.load_from_checkpoint(os.path.join(golden, "trained_small.ckpt"),
                                                    sampling={"type": "cfdg_ddpm_x0", "w": float(z["w"])}, device=torch.device("cuda", 0))
    rows = []
    for w in [float(v) for v in args.w.split(",")]:
        for n in [int(v) for v in args.steps.split(",")]:
            for name, keys in COMPANIONS.items():
                rolls = {}
                for phi in (None, args.phi):
                    m.hparams.sampling.w, m.hparams.sampling.steps, m.hparams.sampling.cfg_rescale = w, n, phi
                    m.hparams.sampling.x0_clip, m.hparams.sampling.x0_threshold = keys["x0_clip"], keys["x0_threshold"]
                    rolls[phi], _ = m.sample(x_T, wav)
                lab = label[:, :rolls[None].shape[2]].to(rolls[None].device).float()
                counts = {phi: m.engine.frame_counts(rolls[phi][:, 0], lab, thr) for phi in rolls}
                rec = dict(part="proxy", w=w, steps=n, companions=name, phi=args.phi, off=dict(zip(("tp", "fp", "fn"), counts[None])),
                           rescaled=dict(zip(("tp", "fp", "fn"), counts[args.phi])),
                           max_abs_roll_difference=float((rolls[args.phi] - rolls[None]).abs().max()),
                           cells_across_threshold=int(((rolls[args.phi] > thr) != (rolls[None] > thr)).sum()))
                rows.append(rec)
                print(json.dumps(rec), flush=True)
    print(f"\nw | n | with | phi 0 TP/FP/FN | phi {args.phi} TP/FP/FN | max |roll_phi - roll_0| | cells across thr")
    for r in rows:
        c, t = r["off"], r["rescaled"]
        print(f"{r['w']:3g} | {r['steps']:4d} | {r['companions']} | {c['tp']}/{c['fp']}/{c['fn']} | {t['tp']}/{t['fp']}/{t['fn']} | "
              f"{r['max_abs_roll_difference']:.3e} | {r['cells_across_threshold']}")
    same = all(r["off"] == r["rescaled"] for r in rows)
    print("\nthe proxy's counts " + ("do not depend on the option in any cell" if same else "depend on the option in at least one cell"))


def fused_part(args):
    import bench
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[2]
    m = bench.build_model(dev, w=3.0)
    B, T = cfg["B"], cfg["L"] // bench.HP["hop_length"]
    g = torch.Generator().manual_seed(0)
    wav = 0.1 * torch.randn(B, cfg["L"], generator=g)
    x_T = torch.randn(B, 1, T, 88, generator=g)
    eng = m.engine
    every = {"a": dict(phi=None, x0_clip=None, x0_threshold=None), "b": dict(phi=args.phi, x0_clip=None, x0_threshold=None),
             "c": dict(phi=None, x0_clip=1, x0_threshold=None), "d": dict(phi=None, x0_clip=1, x0_threshold=0.995)}
    forms = {f: every[f] for f in args.forms.split(",")}

    def run(form):
        keys = forms[form]
        m.hparams.sampling.cfg_rescale, m.hparams.sampling.x0_clip, m.hparams.sampling.x0_threshold = keys["phi"], keys["x0_clip"], keys["x0_threshold"]
        for _ in range(1 + args.warmup):                           # capture + instantiate, then warm
            m.sample(x_T, wav, seed=1)
        before = eng.launch_state()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.chains):
            m.sample(x_T, wav, seed=1, check=False)
        t1.record()
        eng.finish()
        after = eng.launch_state()
        clean = after["fallbacks"] == before["fallbacks"] and after["yields"] == before["yields"]
        return t0.elapsed_time(t1) / args.chains, after["mode"], clean

    ms = {f: [] for f in forms}
    mode, clean = {}, {f: True for f in forms}
    for _ in range(args.rounds):
        for f in forms:
            t, mode[f], ok = run(f)
            ms[f].append(t)
            clean[f] = clean[f] and ok
    med = {f: float(np.median(ms[f])) for f in forms}
    rec = dict(part="fused", geometry="config 2: C = 512, 15 layers, B = 16 x T = 125, cfdg_ddpm_x0, w = 3, 200 steps", phi=args.phi,
               ms_per_chain={f: (med[f] if clean[f] else None) for f in forms}, runs_ms=ms,
               runs_max_over_min={f: max(ms[f]) / min(ms[f]) for f in forms}, mode=mode, clean=clean)
    if "a" in forms:
        rec["over_a"] = {f: med[f] / med["a"] for f in forms}
        rec["per_step_us_over_a"] = {f: (med[f] - med["a"]) * 1e3 / 200 for f in forms}
    print(json.dumps(rec), flush=True)
    names = {"a": "(a) option off, tail kernel", "b": f"(b) cfg_rescale {args.phi}", "c": "(c) x0_clip", "d": "(d) x0_clip + x0_threshold 0.995"}
    print("\nform | ms per chain | max / min over its runs | mode")
    for f in forms:
        t = "        -" if not clean[f] else f"{med[f]:9.2f}"
        print(f"{names[f]} | {t} | {rec['runs_max_over_min'][f]:5.3f} | {mode[f]}")
    if "a" in forms and len(forms) > 1:
        print("\n" + ", ".join(f"({f}) / (a) = {rec['over_a'][f]:.4f} ({rec['per_step_us_over_a'][f]:+.1f} us per step)" for f in forms if f != "a"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--w", default="0.5,2,5", help="comma-separated guidance weights (part 1)")
    ap.add_argument("--steps", default="200,20", help="comma-separated n (part 1)")
    ap.add_argument("--phi", type=float, default=0.7, help="the factor, hparams.sampling.cfg_rescale")
    ap.add_argument("--chains", type=int, default=3, help="timed chains per run (part 2)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2, help="runs per cell (part 2)")
    ap.add_argument("--forms", default="a,b,c,d", help="the cells of part 2")
    ap.add_argument("--part", default="both", choices=("both", "proxy", "fused"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rescale_sweep measures on the GPU: no ROCm device visible")
    torch.cuda.set_device(0)
    if args.part in ("both", "proxy"):
        proxy_part(args)
    if args.part in ("both", "fused"):
        fused_part(args)


if __name__ == "__main__":
    main()
