"""Blend sweep (option "window_blend", sample_long(..., blend=)): what the cross-fade and the hand-over of shared frames cost
against the mean, and what they change on the trained proxy.

    python tools/blend_sweep.py [--modes 0,1,2] [--windows 3] [--chains 3] [--warmup 1] [--rounds 3] [--steps 200] [--no-proxy]

Chain time, at the shipping geometry (k = 9, 15 layers, C = 512, cfdg_ddpm_x0 w = 0.5, --windows 640-frame windows sharing
160 frames, Philox noise): the engine is driven as sample_long drives it, with "window_overlap" held over the whole
measurement so that a mode's chain is captured once per round and replayed; ms per chain from device events around --chains
chains after --warmup, the modes in turn, --rounds rounds.  Per mode the median, and the ratio of a mode's median to mode
0's; the spread of mode 0's own rounds (max / min) stands beside it, since a ratio inside that spread is no difference.
--modes 0 with DR_LIB pointing at a build of the parent commit gives the parent's chain as further repeats of mode 0 (the
option is never set then).  A mode whose launch state shows a fallback or a yield prints no time.

Behaviour, on tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy): its fixture's four 64-frame clips, six
times over, are one recording of 1536 frames - three windows - with the labels tiled alike.  Per mode the frame-level
TP / FP / FN of the thresholded roll, the largest |roll - roll of mode 0| inside the two overlaps and outside them, and the
cells that cross the threshold.  The proxy's task is easy: a record of behaviour, not a quality claim.
One JSON line per measurement, then two tables.
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

HOP, T, O = 512, 640, 160
NAMES = {0: "mean", 1: "linear", 2: "nearest"}


def chain_times(args, modes):
    import bench
    from diffroll_amd import longform
    hp = dict(bench.HP)
    hp.update(kernel_size=9, timesteps=args.steps)
    m = bench.build_model(torch.device("cuda", 0), hp=hp, sampler="cfdg_ddpm_x0")
    eng = m.engine
    g = torch.Generator().manual_seed(0)
    plan = longform.plan_windows((T + (args.windows - 1) * (T - O)) * HOP, HOP, T, O)
    wav = 0.1 * torch.randn((T + (args.windows - 1) * (T - O)) * HOP, generator=g)
    eng.frontend(longform.window_audio(wav, plan, HOP), T)
    x_T = longform.gather_windows(torch.randn(plan.T_c, 88, generator=g), plan).to(eng.device)
    w = float(m.hparams.sampling.w)
    ms = {k: [] for k in modes}
    clean, mode_name = {k: True for k in modes}, {}
    eng.set_option("window_overlap", O)
    try:
        for _ in range(args.rounds):
            for k in modes:
                if eng.window_blend != k:             # (never set for a run of mode 0 alone: a parent build does not know the name)
                    eng.set_option("window_blend", k)
                for _ in range(args.warmup):          # the first one captures
                    eng.sample("cfdg_ddpm_x0", x_T.clone(), None, w, 7, 0, True, True)
                before = eng.launch_state()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                xs = [x_T.clone() for _ in range(args.chains)]
                t0.record()
                for xb in xs:
                    eng.sample("cfdg_ddpm_x0", xb, None, w, 7, 0, True, False)
                t1.record()
                eng.finish()
                after = eng.launch_state()
                clean[k] = clean[k] and after["fallbacks"] == before["fallbacks"] and after["yields"] == before["yields"]
                mode_name[k] = after["mode"]
                ms[k].append(t0.elapsed_time(t1) / args.chains)
    finally:
        if eng.window_blend != 0:
            eng.set_option("window_blend", 0)
        eng.set_option("window_overlap", 0)
    rows = []
    for k in modes:
        rec = dict(measurement="chain_ms", blend=NAMES[k], windows=args.windows, steps=args.steps, launch_mode=mode_name[k],
                   clean=clean[k], ms_rounds=ms[k] if clean[k] else None, ms_median=float(np.median(ms[k])) if clean[k] else None,
                   rounds_max_over_min=(max(ms[k]) / min(ms[k])) if clean[k] else None, lib=os.environ.get("DR_LIB") or "this build")
        if 0 in modes and clean[k] and clean[0]:
            rec["ratio_to_mean"] = float(np.median(ms[k]) / np.median(ms[0]))
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    return rows


def proxy_behaviour(modes):
    from diffroll_amd import ClassifierFreeDiffRoll, longform
    golden = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(golden, "trained_small.npz"))
    thr = float(z["frame_threshold"])
    wav = torch.from_numpy(z["wav"]).reshape(-1).repeat(6)                      # 4 clips x 6 = 1536 frames
    label = torch.from_numpy(z["label"]).reshape(-1, 88).repeat(6, 1)
    m = ClassifierFreeDiffRoll.load_from_checkpoint(os.path.join(golden, "trained_small.ckpt"),
                                                    sampling={"type": "cfdg_ddpm_x0", "w": float(z["w"])},
                                                    device=torch.device("cuda", 0))
    plan = longform.plan_windows(wav.shape[0], HOP, T, O)
    shared = torch.zeros(plan.T_out, dtype=torch.bool)
    for b in range(1, plan.n):
        shared[b * plan.stride:b * plan.stride + O] = True
    rolls, rows = {}, []
    for k in [0] + [k for k in modes if k != 0]:
        roll = m.sample_long(wav, overlap=O, seed=int(z["noise_seed"]), blend=k)
        rolls[k] = roll.cpu()[0, 0]
        lab = label[:plan.T_out].to(roll.device).float()
        tp, fp, fn = m.engine.frame_counts(roll[0], lab[None], thr)
        d = (rolls[k] - rolls[0]).abs()
        rec = dict(measurement="proxy", blend=NAMES[k], windows=plan.n, frames=plan.T_out, tp=int(tp), fp=int(fp), fn=int(fn),
                   max_abs_difference_inside_overlaps=float(d[shared].max()), max_abs_difference_outside_overlaps=float(d[~shared].max()),
                   cells_across_threshold=int(((rolls[k] > thr) != (rolls[0] > thr)).sum()), launch_mode=m.engine.launch_state()["mode"])
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--modes", default="0,1,2", help="comma-separated values of the option")
    ap.add_argument("--windows", type=int, default=3, help="windows of the timed recording (2 or 3)")
    ap.add_argument("--chains", type=int, default=3, help="timed chains per round and mode")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="diffusion steps of the timed chain (200 = shipping)")
    ap.add_argument("--no-proxy", action="store_true", help="chain times only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blend_sweep measures on the GPU: no ROCm device visible")
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    modes = [int(v) for v in args.modes.split(",")]
    times = chain_times(args, modes)
    print(f"\nk = 9, 15 layers, C = 512, cfdg_ddpm_x0, {args.windows} windows, {args.steps} steps, {args.rounds} rounds of {args.chains} chains")
    print("blend | launch mode | ms per chain (median) | rounds max / min | mode / mean")
    for r in times:
        if r["ms_median"] is None:
            print(f"{r['blend']:7s} | {r['launch_mode']} |         - |     - |     -")
        else:
            ratio = f"{r['ratio_to_mean']:5.3f}" if "ratio_to_mean" in r else "    -"
            print(f"{r['blend']:7s} | {r['launch_mode']} | {r['ms_median']:9.2f} | {r['rounds_max_over_min']:5.3f} | {ratio}")
    if args.no_proxy:
        return
    rows = proxy_behaviour(modes)
    print("\nblend | TP/FP/FN | max |roll - mean's| inside overlaps | outside | cells across thr")
    for r in rows:
        print(f"{r['blend']:7s} | {r['tp']}/{r['fp']}/{r['fn']} | {r['max_abs_difference_inside_overlaps']:.3e} | "
              f"{r['max_abs_difference_outside_overlaps']:.3e} | {r['cells_across_threshold']}")


if __name__ == "__main__":
    main()
