"""Momentum sweep (option "cfg_momentum", hparams.sampling.cfg_momentum): what the momentum of adaptive projected guidance
changes on the trained proxy, and what its state costs on the geometry that fuses.

    python tools/momentum_sweep.py [--w 3] [--steps 200,20] [--chains 3] [--warmup 1] [--rounds 2] [--forms a,b,c,d]

The cells, in both parts:
    (a) the plain chain (the options off: the tail kernel), (b) cfg_project 1.0 + cfg_norm 0.05 - the projected chain without
    momentum, (c) the same with cfg_momentum -0.5, (d) with cfg_momentum -0.75.

Part 1, on tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy) with its fixture's clips and x_T,
cfdg_ddpm_x0, for every w and n: the frame-level TP / FP / FN of every cell against the held-out labels, and
max |roll - roll_b| from the same x_T and seed.  A record of behaviour on an easy task, not a quality claim.  The proxy's
geometry does not fuse; no time is taken there.

Part 2, on the geometry that fuses - bench.py's config 2 (C = 512, 15 layers, 16 guided clips x 125 frames, random-init
weights, 200 steps, w = 3): ms per captured chain from device events around --chains chains after --warmup, the cells timed
in turn from this one process, --rounds runs per cell; medians, and each cell's own spread over its runs (max / min), since
a ratio inside that spread is no difference.  The momentum's cost is reported against (b), the projected chain of the same
build, and against (a).  A chain whose launch state shows a fallback or a yield prints no time.  JSON lines, then tables.
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

CELLS = {"a": dict(cfg_project=None, cfg_norm=None, cfg_momentum=None), "b": dict(cfg_project=1.0, cfg_norm=0.05, cfg_momentum=None),
         "c": dict(cfg_project=1.0, cfg_norm=0.05, cfg_momentum=-0.5), "d": dict(cfg_project=1.0, cfg_norm=0.05, cfg_momentum=-0.75)}
NAMES = {"a": "(a) options off, tail kernel", "b": "(b) cfg_project 1.0 + cfg_norm 0.05", "c": "(c) (b) + cfg_momentum -0.5",
         "d": "(d) (b) + cfg_momentum -0.75"}


def put(m, cell):
    for key in ("cfg_momentum", "cfg_project", "cfg_norm"):      # (the momentum off first: it is refused without a partner)
        setattr(m.hparams.sampling, key, None)
    for key, value in CELLS[cell].items():
        setattr(m.hparams.sampling, key, value)


def proxy_part(args, forms):
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
            m.hparams.sampling.w, m.hparams.sampling.steps = w, n
            rolls = {}
            for f in forms:
                put(m, f)
                rolls[f], _ = m.sample(x_T, wav)
            first = rolls[forms[0]]
            lab = label[:, :first.shape[2]].to(first.device).float()
            rec = dict(part="proxy", w=w, steps=n,
                       counts={f: dict(zip(("tp", "fp", "fn"), m.engine.frame_counts(rolls[f][:, 0], lab, thr))) for f in forms},
                       max_abs_roll_difference_from_b={f: float((rolls[f] - rolls["b"]).abs().max()) for f in forms if "b" in rolls})
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    print("\nw | n | " + " | ".join(f"{NAMES[f]} TP/FP/FN" for f in forms))
    for r in rows:
        print(f"{r['w']:3g} | {r['steps']:4d} | " + " | ".join("{tp}/{fp}/{fn}".format(**r["counts"][f]) for f in forms))


def fused_part(args, forms):
    import bench
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[2]
    m = bench.build_model(dev, w=3.0)
    B, T = cfg["B"], cfg["L"] // bench.HP["hop_length"]
    g = torch.Generator().manual_seed(0)
    wav = 0.1 * torch.randn(B, cfg["L"], generator=g)
    x_T = torch.randn(B, 1, T, 88, generator=g)
    eng = m.engine

    def run(form):
        put(m, form)
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
    rec = dict(part="fused", geometry="config 2: C = 512, 15 layers, B = 16 x T = 125, cfdg_ddpm_x0, w = 3, 200 steps",
               ms_per_chain={f: (med[f] if clean[f] else None) for f in forms}, runs_ms=ms,
               runs_max_over_min={f: max(ms[f]) / min(ms[f]) for f in forms}, mode=mode, clean=clean)
    for base in ("a", "b"):
        if base in forms:
            rec["over_" + base] = {f: med[f] / med[base] for f in forms}
            rec["per_step_us_over_" + base] = {f: (med[f] - med[base]) * 1e3 / 200 for f in forms}
    print(json.dumps(rec), flush=True)
    print("\nform | ms per chain | max / min over its runs | mode")
    for f in forms:
        t = "        -" if not clean[f] else f"{med[f]:9.2f}"
        print(f"{NAMES[f]} | {t} | {rec['runs_max_over_min'][f]:5.3f} | {mode[f]}")
    for base in ("a", "b"):
        if base in forms and len(forms) > 1:
            print("\n" + ", ".join(f"({f}) / ({base}) = {rec['over_' + base][f]:.4f} ({rec['per_step_us_over_' + base][f]:+.1f} us per step)"
                                   for f in forms if f != base))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--w", default="3", help="comma-separated guidance weights (part 1)")
    ap.add_argument("--steps", default="200,20", help="comma-separated n (part 1)")
    ap.add_argument("--chains", type=int, default=3, help="timed chains per run (part 2)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2, help="runs per cell (part 2)")
    ap.add_argument("--forms", default="a,b,c,d", help="the cells")
    ap.add_argument("--part", default="both", choices=("both", "proxy", "fused"))
    args = ap.parse_args()
    forms = args.forms.split(",")
    if any(f not in CELLS for f in forms):
        raise SystemExit(f"--forms takes cells of {sorted(CELLS)}, got {args.forms!r}")
    if not torch.cuda.is_available():
        raise SystemExit("momentum_sweep measures on the GPU: no ROCm device visible")
    torch.cuda.set_device(0)
    if args.part in ("both", "proxy"):
        proxy_part(args, forms)
    if args.part in ("both", "fused"):
        fused_part(args, forms)


if __name__ == "__main__":
    main()
