"""Several draws per clip in one chain (option "draws", ClassifierFreeDiffRoll.sample(draws=)): what sharing the
conditioning buys.

    python tools/draws_sweep.py [--draws 4] [--steps 200] [--reps 3] [--warmup 1] [--no-quality]

At config 2's geometry (n = 4 clips of 125 frames, D = 4: the 16 rolls of bench.py's headline) and at the shipping
long-form geometry (one recording of 3 windows of 640 frames, D = 4), k = 9, 15 layers, C = 512, cfdg_ddpm_x0 w = 0.5,
Philox noise, three ways to the same D rolls per clip are timed end to end in one process (front-end, chain, for the
long-form cell also the stitch; host clock around a device synchronisation), alternating rep by rep after `warmup`
untimed rounds.  Every timed call replays a captured chain: an untimed call of the same case goes first (the engine keeps
one captured chain, and the cases differ in shape or options), and its capture time is listed apart.  (Case (c) changes
first_sample from chain to chain, which replays the same graph.)  The long-form calls are the exception: sample_long /
sample_long_batch set and restore "window_overlap", which drops the chain, so every one of them captures - once in (a)
and (b), D times in (c); the capture column says how much of each time that is.
    (a) the draws chain: front-end on the n clips, one chain of D * n rolls;
    (b) the same rolls from the waveform tiled D times (all there is without the option);
    (c) D separate chains of the n clips.
(d) the conditioner tensors [L][fe_B][2 Cp / 4][T][4] of (a) and (b) in bytes - the engine's allocation rule, and next to
it the device memory a fresh engine's first front-end call took (every front-end buffer, in the allocator's granules);
(e) the front-end alone for (a) and (b).
Then, on tests/golden/trained_small.ckpt and the held-out clips of trained_small.npz: TP / FP / FN at the frame
threshold of one draw and of the mean of 8 draws (a record of the proxy task, not a quality claim).
One JSON line per cell, then the tables.
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

import numpy as np
import torch

HOP, T_WIN, O = 512, 640, 160


def timed(fn, eng):
    before = eng.launch_state()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    after = eng.launch_state()
    return ms, after["mode"], after["yields"] - before["yields"], after["fallbacks"] - before["fallbacks"]


def summarise(runs):
    ms = [r[0] for r in runs]
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), mode=runs[-1][1],
                yields=sum(r[2] for r in runs), fallbacks=sum(r[3] for r in runs))


def alternate(cases, eng, reps, warmup, prime=False):
    """prime: the engine caches ONE captured chain and the cases differ in shape or options, so alternating them captures
    every time; each timed call is then preceded by an untimed one of the same case (which captures), and the timed call
    replays.  The capture + instantiate seconds of that untimed call (dr_cold_times) are reported next to the times."""
    runs = {name: [] for name, _ in cases}
    capture = {name: [] for name, _ in cases}
    for rep in range(warmup + reps):
        for name, fn in cases:
            if prime:
                fn()
                capture[name].append(eng.cold_times()[3])
            r = timed(fn, eng)
            if rep >= warmup:
                runs[name].append(r)
    out = {name: summarise(v) for name, v in runs.items()}
    if prime:
        for name in out:
            out[name]["capture_ms"] = 1e3 * statistics.median(capture[name])
    return out


def cond_bytes(hp, clips, T):
    Cp = (int(hp["residual_channels"]) + 63) // 64 * 64
    return int(hp["residual_layers"]) * clips * 2 * Cp * T * 4


def frontend_footprint(build, wav, T):
    """Device memory a fresh engine's first front-end call on `wav` takes (all its buffers)."""
    m = build()
    eng = m.engine
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    eng.frontend(wav, T, return_spec=False)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    del m, eng
    return int(free0 - free1)


def clip_cell(m, build, hp, n, D, T, reps, warmup, g):
    eng = m.engine
    wav = 0.1 * torch.randn(n, T * HOP, generator=g)
    tiled = wav.repeat(D, 1)
    x = torch.randn(D * n, 1, T, 88, generator=g)

    def a():
        m.sample(x, wav, seed=7, draws=D)

    def b():
        m.sample(x, tiled, seed=7)

    def c():
        for d in range(D):
            m.sample(x[d * n:(d + 1) * n], wav, seed=7, first_sample=d * n)

    out = dict(cell="clips", n=n, draws=D, T=T)
    out.update(alternate([("a", a), ("b", b), ("c", c)], eng, reps, warmup, prime=True))
    fe = alternate([("a", lambda: eng.frontend(wav, T, return_spec=False)), ("b", lambda: eng.frontend(tiled, T, return_spec=False))],
                   eng, max(reps, 5), warmup)
    m._fe_key = None
    out["frontend_ms"] = {k: v["ms"] for k, v in fe.items()}
    out["cond_bytes"] = dict(a=cond_bytes(hp, n, T), b=cond_bytes(hp, D * n, T))
    out["frontend_device_bytes"] = dict(a=frontend_footprint(build, wav, T), b=frontend_footprint(build, tiled, T))
    return out


def long_cell(m, build, hp, windows, D, reps, warmup, g):
    from diffroll_amd import longform
    eng = m.engine
    L = (T_WIN + (windows - 1) * (T_WIN - O)) * HOP            # exactly `windows` windows
    wav = 0.1 * torch.randn(L, generator=g)
    plan = longform.plan_windows(L, HOP, overlap=O)
    x = torch.randn(D, 1, plan.T_c, 88, generator=g)
    clips = longform.window_audio(wav, plan, HOP)
    tiled = clips.repeat(D, 1)

    def a():
        m.sample_long(wav, overlap=O, seed=7, x_T=x, draws=D)

    def b():
        # without the option: the recording D times in one sample_long_batch chain (its windows' audio D times)
        m.sample_long_batch([wav] * D, overlap=O, seed=7, x_T=[x[d:d + 1] for d in range(D)])

    def c():
        for d in range(D):
            m.sample_long(wav, overlap=O, seed=7, recording=d, x_T=x[d:d + 1])

    out = dict(cell="long-form", n=windows, draws=D, T=T_WIN)
    out.update(alternate([("a", a), ("b", b), ("c", c)], eng, reps, warmup, prime=True))
    fe = alternate([("a", lambda: eng.frontend(clips, T_WIN, return_spec=False)),
                    ("b", lambda: eng.frontend(tiled, T_WIN, return_spec=False))], eng, max(reps, 5), warmup)
    m._fe_key = None
    out["frontend_ms"] = {k: v["ms"] for k, v in fe.items()}
    out["cond_bytes"] = dict(a=cond_bytes(hp, windows, T_WIN), b=cond_bytes(hp, D * windows, T_WIN))
    out["frontend_device_bytes"] = dict(a=frontend_footprint(build, clips, T_WIN), b=frontend_footprint(build, tiled, T_WIN))
    return out


def quality(device, D=8):
    from diffroll_amd import ClassifierFreeDiffRoll
    from diffroll_amd.ensemble import aggregate
    gold = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(gold, "trained_small.npz"))
    m = ClassifierFreeDiffRoll.load_from_checkpoint(os.path.join(gold, "trained_small.ckpt")).to(device)
    wav, label = torch.from_numpy(z["wav"]), torch.from_numpy(z["label"])
    n, Tn, _ = label.shape
    thr = float(m.hparams.frame_threshold)
    x = torch.randn(D * n, 1, Tn, 88, generator=torch.Generator().manual_seed(2024))
    rolls, _ = m.sample(x, wav, seed=1, draws=D)
    lab = label[:, :rolls.shape[2]].to(rolls.device, torch.float32).contiguous()
    out = dict(clips=n, frames=int(rolls.shape[2]), draws=D, threshold=thr, single=[])
    for d in range(D):
        out["single"].append(m.engine.frame_counts(rolls[d * n:(d + 1) * n, 0].contiguous(), lab, thr))
    mean, votes, _ = aggregate(rolls, D, thr)
    out["mean"] = m.engine.frame_counts(mean[:, 0].contiguous(), lab, thr)
    out["vote_majority"] = m.engine.frame_counts(votes[:, 0].contiguous(), lab, 0.5)
    return out


def f1(c):
    tp, fp, fn = c
    return 2 * tp / max(2 * tp + fp + fn, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--draws", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200, help="diffusion steps of the chain (200 = shipping)")
    ap.add_argument("--reps", type=int, default=3, help="timed rounds per cell (each round: cases a, b, c)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-quality", action="store_true", help="skip the TP / FP / FN record on the trained checkpoint")
    args = ap.parse_args()
    import bench
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hp = dict(bench.HP)
    hp.update(kernel_size=9, timesteps=args.steps)

    def build():
        return bench.build_model(device, hp=hp, sampler="cfdg_ddpm_x0")

    m = build()
    g = torch.Generator().manual_seed(0)
    D = args.draws
    cells = [clip_cell(m, build, hp, 4, D, 125, args.reps, args.warmup, g),
             long_cell(m, build, hp, 3, D, args.reps, args.warmup, g)]
    for c in cells:
        print(json.dumps(c), flush=True)
    print(f"\nk = 9, 15 layers, C = 512, cfdg_ddpm_x0 w = 0.5, {args.steps} steps, D = {D}, {args.reps} alternating reps: median (min - max) ms")
    print("cell | n x T | (a) draws chain | mode | (b) tiled waveform | mode | (c) D chains | mode | a / b | a / c | capture ms a/b/c (not in the times) | yields a/b/c | fallbacks a/b/c")
    for c in cells:
        a, b, cc = c["a"], c["b"], c["c"]
        print(f"{c['cell']} | {c['n']} x {c['T']} | {a['ms']:.1f} ({a['ms_min']:.1f} - {a['ms_max']:.1f}) | {a['mode']} | "
              f"{b['ms']:.1f} ({b['ms_min']:.1f} - {b['ms_max']:.1f}) | {b['mode']} | {cc['ms']:.1f} ({cc['ms_min']:.1f} - {cc['ms_max']:.1f}) | "
              f"{cc['mode']} | {a['ms'] / b['ms']:.3f} | {a['ms'] / cc['ms']:.3f} | {a['capture_ms']:.1f}/{b['capture_ms']:.1f}/{cc['capture_ms']:.1f} | "
              f"{a['yields']}/{b['yields']}/{cc['yields']} | "
              f"{a['fallbacks']}/{b['fallbacks']}/{cc['fallbacks']}")
    print("\ncell | conditioner bytes (a) | (b) | a / b | device bytes of a fresh engine's front-end (a) | (b) | front-end ms (a) | (b) | a / b")
    for c in cells:
        cb, fb, fm = c["cond_bytes"], c["frontend_device_bytes"], c["frontend_ms"]
        print(f"{c['cell']} | {cb['a']} | {cb['b']} | {cb['a'] / cb['b']:.3f} | {fb['a']} | {fb['b']} | {fm['a']:.3f} | {fm['b']:.3f} | "
              f"{fm['a'] / fm['b']:.3f}")
    if not args.no_quality:
        q = quality(device)
        print("\n" + json.dumps(q))
        print(f"\ntrained_small.ckpt, {q['clips']} held-out clips x {q['frames']} frames, 200 steps, threshold {q['threshold']}: TP / FP / FN (frame F1)")
        for d, c in enumerate(q["single"]):
            print(f"draw {d}: {c[0]} / {c[1]} / {c[2]} ({f1(c):.4f})")
        print(f"mean of {q['draws']} draws: {q['mean'][0]} / {q['mean'][1]} / {q['mean'][2]} ({f1(q['mean']):.4f})")
        print(f"majority vote of {q['draws']} draws: {q['vote_majority'][0]} / {q['vote_majority'][1]} / {q['vote_majority'][2]} ({f1(q['vote_majority']):.4f})")


if __name__ == "__main__":
    main()
