"""Respaced sampling sweep (option "sampling_steps", hparams.sampling.steps): what fewer steps buy and cost.

    python tools/steps_sweep.py --config 2 --steps 200,100,50,20 [--chains 5] [--warmup 2]

For each n: ms per captured chain at a bench.py configuration (synthetic k = 9 network, Philox noise), the capture +
instantiate time of its graph, and the frame-level TP / FP / FN and Frame-F1 of the test_step of
tests/golden/trained_small.ckpt (the reference-trained C = 64 proxy, its fixture's clips, x_T and noise) at n steps.
The proxy task is easy: its F1 does not say what fewer steps cost on real weights.  One JSON line per n, then a table.
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


def chain_ms(cfg_id, steps, chains, warmup):
    import bench
    cfg = bench.CONFIGS[cfg_id]
    device = torch.device("cuda", 0)
    hp = dict(bench.HP)
    hp.update(kernel_size=cfg["k"], timesteps=cfg["S"])
    it = None
    Tn = cfg["L"] // hp["hop_length"]
    if cfg["sampler"] == "inpainting_ddpm_x0":
        it = [Tn // 4, Tn // 2]
    m = bench.build_model(device, hp=hp, sampler=cfg["sampler"], inpainting_t=it)
    g = torch.Generator().manual_seed(0)
    wav = 0.1 * torch.randn(cfg["B"], cfg["L"], generator=g)
    x = torch.randn(cfg["B"], 1, Tn, 88, generator=g)
    out = {}
    for n in steps:
        m.hparams.sampling.steps = n
        m.sample(x, wav, seed=0)                                   # capture + instantiate
        capture_s = m.engine.cold_times()[3]
        for i in range(warmup):
            m.sample(x, wav, seed=1 + i)
        eng = m.engine
        before = eng.launch_state()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(chains):
            m.sample(x, wav, seed=100 + i, check=False)
        t1.record()
        eng.finish()
        after = eng.launch_state()
        out[n] = dict(ms_per_chain=t0.elapsed_time(t1) / chains, capture_s=capture_s, mode=after["mode"],
                      clean=after["fallbacks"] == before["fallbacks"] and after["yields"] == before["yields"])
    return out


def proxy_f1(steps):
    from diffroll_amd import ClassifierFreeDiffRoll
    golden = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(golden, "trained_small.npz"))
    hp = json.loads(str(z["hp"]))
    S, (B, Tn, _) = int(hp["timesteps"]), z["label"].shape
    gen = torch.Generator().manual_seed(int(z["noise_seed"]))       # the fixture's draws (tests/test_trained_golden.py)
    x_T = torch.randn(B, 1, Tn, 88, generator=gen)
    noise = torch.randn(S, B, 1, Tn, 88, generator=gen)
    batch = {"frame": torch.from_numpy(z["label"]), "audio": torch.from_numpy(z["wav"]), "x_T": x_T, "noise": noise}
    out = {}
    for n in steps:
        m = ClassifierFreeDiffRoll.load_from_checkpoint(os.path.join(golden, "trained_small.ckpt"),
                                                        sampling={"type": "cfdg_ddpm_x0", "w": float(z["w"]), "steps": n},
                                                        device=torch.device("cuda", 0))
        r = m.test_step(batch, 1)
        out[n] = dict(tp=r["tp"], fp=r["fp"], fn=r["fn"], frame_f1=r["Test/Frame_F1"])
        del m
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", type=int, default=2, help="bench.py configuration (default 2)")
    ap.add_argument("--steps", default="200,100,50,20", help="comma-separated n (200 = the full chain)")
    ap.add_argument("--chains", type=int, default=5, help="timed chains per n")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-proxy", action="store_true", help="skip the trained-proxy F1")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    steps = [int(v) for v in args.steps.split(",")]
    speed = chain_ms(args.config, steps, args.chains, args.warmup)
    f1 = {} if args.no_proxy else proxy_f1(steps)
    base = speed.get(max(steps), {}).get("ms_per_chain")
    for n in steps:
        rec = dict(config=args.config, steps=n, **speed[n], **f1.get(n, {}))
        print(json.dumps(rec))
    print(f"\nconfig {args.config}: n | ms / chain | vs n = {max(steps)} | capture s | mode | proxy TP/FP/FN | Frame-F1")
    for n in steps:
        s, f = speed[n], f1.get(n)
        q = f"{f['tp']}/{f['fp']}/{f['fn']} | {f['frame_f1']:.4f}" if f else "- | -"
        print(f"{n:4d} | {s['ms_per_chain']:9.2f} | {s['ms_per_chain'] / base:6.3f} | {s['capture_s']:.3f} | {s['mode']}"
              f"{'' if s['clean'] else ' (fallback / yield!)'} | {q}")


if __name__ == "__main__":
    main()
