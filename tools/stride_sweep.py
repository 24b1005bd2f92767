"""Guidance-stride sweep (option "guidance_stride", hparams.sampling.guidance_stride): what reusing the guidance update saves on
the geometries that matter, and what it changes on the trained proxy.

    python tools/stride_sweep.py [--strides 0,2,3,4] [--chains 3] [--warmup 1] [--rounds 2] [--out profiles/stride_sweep.txt]

Part 1, timing, cfdg_ddpm_x0, w = 3, 200 steps, random-init weights (bench.py's model), at two geometries: bench.py's config 2
(16 guided clips of 125 frames) and config 6, the reference's shipping geometry (4 guided clips of 640 frames).  The cells:
every stride of --strides (0 = the option off) and "w0", the chain of conditional evaluations alone (w = 0).  Each cell: ms
per captured chain from device events around --chains chains after --warmup, the cells timed in turn from this one process,
--rounds runs per cell; the median, the cell's own spread over its runs (max / min: a ratio inside that spread is no
difference), the network evaluations of the chain, and the launch mode dr_launch_state reports behind a dr_step at a step that
refreshes, at one that reuses and at a w = 0 step.  A chain whose launch state shows a fallback or a yield prints no time.
Then the step costs: a chain at stride n runs R_n refresh steps and U_n reuse steps, so the times at the two extreme strides
give r (a refresh step under the option: stack launch, head projections, update_stride_kernel) and u (a reuse step); the
stride in between is predicted from them and compared with what it measured.  u is set against the step of the w0 chain and r
against the step of the option-off chain (both end in the tail kernel).

Part 2, on tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy) with its fixture's clips and x_T, for every n
of --proxy-steps: the frame-level TP / FP / FN of every stride against the held-out labels and max |roll - roll_off| from the
same x_T and seed.  A record of behaviour on an easy task, not a quality claim.  No time is taken there.

JSON lines, then tables; the tables also go to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def schedule(visited, n):
    """[(t, refreshes)] of a chain whose every step guides (include/diffroll_amd.h: k % n == 0 or t == 0)."""
    return [(t, n <= 1 or k % n == 0 or t == 0) for k, t in enumerate(visited)]


def timing_part(args, strides, config):
    import bench
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[config]
    m = bench.build_model(dev, w=3.0)
    B, T = cfg["B"], cfg["L"] // bench.HP["hop_length"]
    g = torch.Generator().manual_seed(0)
    wav = 0.1 * torch.randn(B, cfg["L"], generator=g)
    x_T = torch.randn(B, 1, T, 88, generator=g)
    eng = m.engine
    visited = m.visited_steps()
    cells = [str(n) for n in strides] + ["w0"]

    def put(cell):
        m.hparams.sampling.w = 0.0 if cell == "w0" else 3.0
        m.hparams.sampling.guidance_stride = None if cell == "w0" or int(cell) <= 1 else int(cell)

    def run(cell):
        put(cell)
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
        return t0.elapsed_time(t1) / args.chains, after["fallbacks"] == before["fallbacks"] and after["yields"] == before["yields"]

    def modes(cell):
        """dr_launch_state behind a dr_step at the chain's first step (a refresh, or the w0 step) and at its second (a reuse)."""
        put(cell)
        eng = m.engine
        xb = x_T.squeeze(1).to(eng.device).contiguous()
        w = float(m.hparams.sampling.w)
        out = []
        for t in visited[:2]:
            eng.step("cfdg_ddpm_x0", xb, None, t, w=w, seed=1)
            out.append(eng.launch_state()["mode"])
        eng.finish()
        return out

    ms, clean = {c: [] for c in cells}, {c: True for c in cells}
    for _ in range(args.rounds):
        for c in cells:
            t, ok = run(c)
            ms[c].append(t)
            clean[c] = clean[c] and ok
    mode = {c: modes(c) for c in cells}
    med = {c: float(np.median(ms[c])) for c in cells}
    evals = {c: (len(visited) * B if c == "w0" else sum(2 * B if r else B for _, r in schedule(visited, int(c)))) for c in cells}
    rec = dict(part="timing", config=config, geometry=f"C = 512, 15 layers, B = {B} x T = {T}, cfdg_ddpm_x0, w = 3, {len(visited)} steps",
               ms_per_chain={c: (med[c] if clean[c] else None) for c in cells}, runs_ms=ms,
               runs_max_over_min={c: max(ms[c]) / min(ms[c]) for c in cells}, evaluations=evals, mode_first_two_steps=mode, clean=clean)
    print(json.dumps(rec), flush=True)
    say(f"\nconfig {config}: {rec['geometry']}; {args.rounds} runs of {args.chains} captured chains per cell")
    say("cell | ms per chain (median) | runs [ms] | max / min over its runs | evaluations | vs off: time, evaluations | "
        "mode behind step 1 / step 2 (dr_step)")
    off = "0" if "0" in cells else cells[0]
    for c in cells:
        name = "w0 (conditional evaluations alone)" if c == "w0" else ("stride off" if int(c) <= 1 else f"stride {c}")
        what = "unguided / unguided" if c == "w0" else ("guided / guided" if int(c) <= 1 else "refresh / reuse")
        t = "        -" if not clean[c] else f"{med[c]:9.2f}"
        say(f"{name} | {t} | {', '.join(f'{v:.2f}' for v in ms[c])} | {rec['runs_max_over_min'][c]:5.3f} | {evals[c]} | "
            f"{med[c] / med[off]:.4f}, {evals[c] / evals[off]:.4f} | {what}: {mode[c][0]} / {mode[c][1]}")
    on = sorted(int(c) for c in cells if c != "w0" and int(c) > 1)
    if len(on) >= 2 and all(clean[str(n)] for n in on):
        lo, hi = on[0], on[-1]
        count = lambda n: (sum(r for _, r in schedule(visited, n)), sum(not r for _, r in schedule(visited, n)))
        A = np.array([count(lo), count(hi)], dtype=np.float64)
        r, u = np.linalg.solve(A, np.array([med[str(lo)], med[str(hi)]]))
        say(f"step costs from strides {lo} and {hi} (refresh / reuse steps {count(lo)} and {count(hi)}): a refresh step {r * 1e3:.1f} us, "
            f"a reuse step {u * 1e3:.1f} us")
        for n in on[1:-1]:
            R, U = count(n)
            say(f"  stride {n} predicted from them {R * r + U * u:.2f} ms, measured {med[str(n)]:.2f} ms")
        n_steps = len(visited)
        say(f"  a step of the option-off chain (stack launch + tail kernel, 2 B evaluations): {med[off] / n_steps * 1e3:.1f} us; "
            f"refresh step / that = {r / (med[off] / n_steps):.4f}")
        say(f"  a step of the w0 chain (stack launch + tail kernel, B evaluations): {med['w0'] / n_steps * 1e3:.1f} us; "
            f"reuse step / that = {u / (med['w0'] / n_steps):.4f}")
        say(f"  B-evaluation step / 2 B-evaluation step: w0 / off = {med['w0'] / med[off]:.4f}, reuse / refresh = {u / r:.4f} "
            f"(the evaluation ratio is 0.5)")


def proxy_part(args, strides):
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
        for n in [int(v) for v in args.proxy_steps.split(",")]:
            m.hparams.sampling.w, m.hparams.sampling.steps = w, n
            rolls = {}
            for s in strides:
                m.hparams.sampling.guidance_stride = s if s > 1 else None
                rolls[s], _ = m.sample(x_T, wav)
            first = rolls[strides[0]]
            lab = label[:, :first.shape[2]].to(first.device).float()
            rec = dict(part="proxy", w=w, steps=n,
                       counts={s: dict(zip(("tp", "fp", "fn"), m.engine.frame_counts(rolls[s][:, 0], lab, thr))) for s in strides},
                       max_abs_roll_difference_from_off={s: float((rolls[s] - first).abs().max()) for s in strides})
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    say(f"\ntrained proxy (tests/golden/trained_small.ckpt, its fixture's clips, x_T and seed), cfdg_ddpm_x0: TP / FP / FN per stride")
    say("w | n | " + " | ".join("off" if s <= 1 else f"stride {s}" for s in strides) + " | max |roll - roll off| per stride")
    for r in rows:
        say(f"{r['w']:3g} | {r['steps']:4d} | " + " | ".join("{tp}/{fp}/{fn}".format(**r["counts"][s]) for s in strides) + " | " +
            ", ".join(f"{r['max_abs_roll_difference_from_off'][s]:.3e}" for s in strides))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--strides", default="0,2,3,4", help="comma-separated strides (0 = the option off)")
    ap.add_argument("--configs", default="2,6", help="bench.py configurations of part 1")
    ap.add_argument("--chains", type=int, default=3, help="timed chains per run (part 1)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2, help="runs per cell (part 1)")
    ap.add_argument("--w", default="3", help="comma-separated guidance weights (part 2)")
    ap.add_argument("--proxy-steps", default="200,20", help="comma-separated n (part 2)")
    ap.add_argument("--part", default="both", choices=("both", "timing", "proxy"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stride_sweep.txt"))
    args = ap.parse_args()
    strides = [int(v) for v in args.strides.split(",")]
    if any(s < 0 or s > 64 for s in strides):
        raise SystemExit(f"--strides takes values in 0 .. 64, got {args.strides!r}")
    if not torch.cuda.is_available():
        raise SystemExit("stride_sweep measures on the GPU: no ROCm device visible")
    torch.cuda.set_device(0)
    say('Option "guidance_stride": tools/stride_sweep.py on one MI355X (python tools/stride_sweep.py ' + " ".join(sys.argv[1:]) + ")")
    if args.part in ("both", "timing"):
        for config in [int(v) for v in args.configs.split(",")]:
            timing_part(args, strides, config)
    if args.part in ("both", "proxy"):
        proxy_part(args, strides)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
