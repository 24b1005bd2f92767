"""Precision sweep (Engine.set_precision: f32 / bf16x3 / bf16 / f16): what each arithmetic of the two hot contractions costs per
chain, what its weight packing costs to build and to hold, and what it changes on the trained proxy.

    python tools/precision_sweep.py [--configs 2,6] [--chains 2] [--warmup 1] [--steps 200] [--no-proxy]

Chain time, per configuration of bench.py (2: 16 guided clips of 125 frames; 6: the shipping geometry, 4 guided clips of
640 frames; k = 9, 15 layers, C = 512, cfdg_ddpm_x0 w = 0.5, Philox noise) and precision: ms per chain from device events
around --chains captured chains after --warmup, TWO runs of every cell in one process, the precisions in turn inside a run
- so a cell's two figures are minutes apart and their ratio is the cell's own run-to-run spread.  A precision is faster
than another only where the ratio of their times lies outside both spreads (f16 is read against bf16 of the same run: the
same MFMA count and operand bytes, so "not told apart" is the expectation).  Beside the times: the launch mode from
dr_launch_state (a cell whose engine fell back or yielded prints no time), the wall time of the set_precision call that
first selected the mode (packing + upload: the first-use cost; 0 for f32, whose packing the commit builds) and the device
bytes that call took (hipMemGetInfo before / after: the mode's weight packings).

Behaviour, on tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy; its fixture's clips, x_T and noise): per
precision the frame-level TP / FP / FN against the fixture's labels (golden: what the reference's own test_step counted),
the largest |roll - f32 roll| and the cells that cross the threshold.  The proxy's task is easy: a record of behaviour, no
quality claim - nothing here says what a reduced precision does to transcription quality with real weights.
One JSON line per measurement, then two tables.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

PRECISIONS = ("f32", "bf16x3", "bf16", "f16")


def chain_times(args, config):
    import bench
    cfg = bench.CONFIGS[config]
    hp = dict(bench.HP)
    hp.update(kernel_size=cfg["k"], timesteps=args.steps)
    dev = torch.device("cuda", 0)
    m = bench.build_model(dev, hp=hp, sampler=cfg["sampler"])
    eng = m.engine
    B, T = cfg["B"], cfg["L"] // hp["hop_length"]
    g = torch.Generator().manual_seed(0)
    wav = 0.1 * torch.randn(B, cfg["L"], generator=g)
    x_T = torch.randn(B, T, 88, generator=g).to(dev)
    eng.frontend(wav, T)
    w = float(m.hparams.sampling.w)
    first_use, packing = {}, {}
    ms = {p: [] for p in PRECISIONS}
    clean, mode = {p: True for p in PRECISIONS}, {}
    for run in range(2):
        for p in PRECISIONS:
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(dev)[0]
            t0 = time.perf_counter()
            eng.set_precision(p)
            torch.cuda.synchronize()
            if run == 0:
                first_use[p] = time.perf_counter() - t0
                packing[p] = free0 - torch.cuda.mem_get_info(dev)[0]
            for _ in range(args.warmup):          # the first one captures
                eng.sample(cfg["sampler"], x_T.clone(), None, w, 7, 0, True, True)
            before = eng.launch_state()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            xs = [x_T.clone() for _ in range(args.chains)]
            e0.record()
            for xb in xs:
                eng.sample(cfg["sampler"], xb, None, w, 7, 0, True, False)
            e1.record()
            eng.finish()
            after = eng.launch_state()
            clean[p] = clean[p] and after["fallbacks"] == before["fallbacks"] and after["yields"] == before["yields"]
            mode[p] = after["mode"]
            ms[p].append(e0.elapsed_time(e1) / args.chains)
    eng.set_precision("f32")
    rows = []
    for p in PRECISIONS:
        ok = clean[p]
        rec = dict(measurement="chain_ms", config=config, clips=B, frames=T, steps=args.steps, precision=p, launch_mode=mode[p], clean=ok,
                   ms_runs=ms[p] if ok else None, ms_best=min(ms[p]) if ok else None,
                   runs_max_over_min=(max(ms[p]) / min(ms[p])) if ok else None,
                   first_use_s=first_use[p], packing_device_bytes=int(packing[p]))
        if ok and clean["bf16x3"]:
            rec["ratio_to_bf16x3"] = min(ms[p]) / min(ms["bf16x3"])
        if ok and clean["bf16"]:
            rec["ratio_to_bf16"] = min(ms[p]) / min(ms["bf16"])
            rec["ratio_to_bf16_per_run"] = [a / b for a, b in zip(ms[p], ms["bf16"])]
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    del m
    return rows


def proxy_behaviour():
    from diffroll_amd import ClassifierFreeDiffRoll
    golden = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(golden, "trained_small.npz"))
    thr = float(z["frame_threshold"])
    wav, label = torch.from_numpy(z["wav"]), torch.from_numpy(z["label"])
    # x_T and the injected z's, regenerated from the stored seed as tests/test_trained_golden.py does (which checks their bits)
    S, (B, Tn, _) = int(json.loads(str(z["hp"]))["timesteps"]), z["label"].shape
    gen = torch.Generator().manual_seed(int(z["noise_seed"]))
    x_T = torch.randn(B, 1, Tn, 88, generator=gen)
    noise = torch.randn(S, B, 1, Tn, 88, generator=gen)
    rolls, rows = {}, []
    for p in PRECISIONS:
        m = ClassifierFreeDiffRoll.load_from_checkpoint(os.path.join(golden, "trained_small.ckpt"), precision=p,
                                                        device=torch.device("cuda", 0))
        roll, _ = m.sample(x_T, wav, noise=noise)
        rolls[p] = roll.cpu()
        out = m.test_step({"frame": label, "audio": wav, "x_T": x_T, "noise": noise}, 1)
        d = (rolls[p] - rolls["f32"]).abs()
        rec = dict(measurement="proxy", precision=p, tp=int(out["tp"]), fp=int(out["fp"]), fn=int(out["fn"]),
                   golden=[int(z["tp"]), int(z["fp"]), int(z["fn"])], max_abs_difference_from_f32=float(d.max()),
                   max_abs_difference_from_reference=float((rolls[p] - torch.from_numpy(z["cfdg_roll"])).abs().max()),
                   cells_across_threshold=int(((rolls[p] > thr) != (rolls["f32"] > thr)).sum()), cells=int(rolls[p].numel()),
                   launch_mode=m.engine.launch_state()["mode"])
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        del m
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="2,6", help="comma-separated bench.py configurations")
    ap.add_argument("--chains", type=int, default=2, help="timed chains per run and cell")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="diffusion steps of the timed chain (200 = shipping)")
    ap.add_argument("--no-proxy", action="store_true", help="chain times only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("precision_sweep measures on the GPU: no ROCm device visible")
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    tables = [chain_times(args, int(c)) for c in args.configs.split(",")]
    print(f"\nk = 9, 15 layers, C = 512, cfdg_ddpm_x0, {args.steps} steps, two runs of {args.chains} chains per cell")
    print("config | clips x frames | precision | launch mode | ms per chain (run 1, run 2) | runs max / min | best / bf16x3's best | "
          "best / bf16's best (run 1, run 2) | first use [s] | packing [MiB]")
    for rows in tables:
        for r in rows:
            if r["ms_runs"] is None:
                print(f"{r['config']} | {r['clips']} x {r['frames']} | {r['precision']:6s} | {r['launch_mode']} | - | - | - | - | "
                      f"{r['first_use_s']:.2f} | {r['packing_device_bytes'] / 2 ** 20:.0f}")
                continue
            ratio = f"{r['ratio_to_bf16x3']:.3f}" if "ratio_to_bf16x3" in r else "-"
            if "ratio_to_bf16" in r:
                ratio += f" | {r['ratio_to_bf16']:.4f} ({r['ratio_to_bf16_per_run'][0]:.4f}, {r['ratio_to_bf16_per_run'][1]:.4f})"
            else:
                ratio += " | -"
            print(f"{r['config']} | {r['clips']} x {r['frames']} | {r['precision']:6s} | {r['launch_mode']} | "
                  f"{r['ms_runs'][0]:.2f}, {r['ms_runs'][1]:.2f} | {r['runs_max_over_min']:.4f} | {ratio} | "
                  f"{r['first_use_s']:.2f} | {r['packing_device_bytes'] / 2 ** 20:.0f}")
    if args.no_proxy:
        return
    rows = proxy_behaviour()
    print("\nprecision | TP/FP/FN (golden " + "/".join(str(v) for v in rows[0]["golden"]) + ") | max |roll - f32 roll| | "
          "max |roll - reference's roll| | cells across thr (of " + str(rows[0]["cells"]) + ")")
    for r in rows:
        print(f"{r['precision']:6s} | {r['tp']}/{r['fp']}/{r['fn']} | {r['max_abs_difference_from_f32']:.3e} | "
              f"{r['max_abs_difference_from_reference']:.3e} | {r['cells_across_threshold']}")


if __name__ == "__main__":
    main()
