"""Several recordings in one long-form chain (option "window_break", sample_long_batch): what grouping buys.

    python tools/long_batch_sweep.py [--recordings 1,2,4,8] [--windows 1,2,3] [--steps 200] [--reps 3] [--warmup 1]

For R recordings of n windows each at the shipping geometry (k = 9, 15 layers, C = 512, cfdg_ddpm_x0 w = 0.5, 640-frame
windows overlapping by 160, Philox noise) two cases are timed end to end (front-end, capture, chain, stitch; host clock
around a device synchronisation):
    (a) R consecutive sample_long calls (one chain per recording: what the CLI does by default);
    (b) one sample_long_batch over the same recordings.
The two cases alternate inside one process, rep by rep, after `warmup` untimed rounds; the table gives the median, the
min - max spread of the reps, the launch mode of each case and whether yields / fallbacks moved under the measurement.
One JSON line per cell, then the table.
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

HOP, T, O = 512, 640, 160


def timed(fn, eng):
    before = eng.launch_state()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    after = eng.launch_state()
    return ms, after["mode"], after["yields"] - before["yields"], after["fallbacks"] - before["fallbacks"]


def cell(m, R, n, reps, warmup, g):
    L = (T + (n - 1) * (T - O)) * HOP                      # exactly n windows
    wavs = [0.1 * torch.randn(L, generator=g) for _ in range(R)]
    eng = m.engine

    def solo():
        for i, wv in enumerate(wavs):
            m.sample_long(wv, overlap=O, seed=7, recording=i)

    def batch():
        m.sample_long_batch(wavs, overlap=O, seed=7)

    runs = {"a": [], "b": []}
    for rep in range(warmup + reps):
        for name, fn in (("a", solo), ("b", batch)):
            r = timed(fn, eng)
            if rep >= warmup:
                runs[name].append(r)
    out = dict(recordings=R, windows_each=n)
    for name in ("a", "b"):
        ms = [r[0] for r in runs[name]]
        out[name] = dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), mode=runs[name][-1][1],
                         yields=sum(r[2] for r in runs[name]), fallbacks=sum(r[3] for r in runs[name]))
    out["b_over_a"] = out["b"]["ms"] / out["a"]["ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--recordings", default="1,2,4,8")
    ap.add_argument("--windows", default="1,2,3", help="windows per recording")
    ap.add_argument("--steps", type=int, default=200, help="diffusion steps of the chain (200 = shipping)")
    ap.add_argument("--reps", type=int, default=3, help="timed rounds per cell (each round: case a, then case b)")
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hp = dict(bench.HP)
    hp.update(kernel_size=9, timesteps=args.steps)
    m = bench.build_model(torch.device("cuda", 0), hp=hp, sampler="cfdg_ddpm_x0")
    g = torch.Generator().manual_seed(0)
    cells = []
    for n in (int(v) for v in args.windows.split(",")):
        for R in (int(v) for v in args.recordings.split(",")):
            c = cell(m, R, n, args.reps, args.warmup, g)
            cells.append(c)
            print(json.dumps(c), flush=True)
    print(f"\nk = 9, 15 layers, C = 512, cfdg_ddpm_x0, {args.steps} steps, {args.reps} alternating reps (median, min - max)")
    print("windows each | recordings | (a) R x sample_long ms | mode | (b) sample_long_batch ms | mode | b / a | yields a/b | fallbacks a/b")
    for c in cells:
        a, b = c["a"], c["b"]
        print(f"{c['windows_each']:12d} | {c['recordings']:10d} | {a['ms']:9.1f} ({a['ms_min']:.1f} - {a['ms_max']:.1f}) | {a['mode']} | "
              f"{b['ms']:9.1f} ({b['ms_min']:.1f} - {b['ms_max']:.1f}) | {b['mode']} | {c['b_over_a']:.3f} | "
              f"{a['yields']}/{b['yields']} | {a['fallbacks']}/{b['fallbacks']}")


if __name__ == "__main__":
    main()
