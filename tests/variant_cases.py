"""The forced launch variants of tests/test_gpu_launch_variants.py, as one table - test infrastructure.  A case is a small
network (synthetic parameters of the oracle), a sampler, a batch shape and a precision; each case carries pin sets - tune.*
knobs (csrc/kernels.h: Tuning) held with tuning_pins.pinned - and `claim()` states which kernel variant every launch of the
network takes under a pin set.  tests/test_launch_variants_cpu.py proves the claims on csrc/launch_plan.h without a GPU, so
that a forced knob the planner ignores (one M tile, frame tiles no multiple of 8, K slabs no multiple of 4, ...) fails there
instead of making a twin comparison vacuous; the GPU tests then compare the runs bit for bit and hold one of them to the
oracle.

Groups:
  A  block -> XCD mapping of the per-phase GEMM launches: tune.xcd_n = 1 against 0 (and tune.xcd_model = 0 against the
     traffic model), under every conv / 1x1 tile flavour, with and without split-K
  B  the 1x1 residual / skip GEMM keeps one chain per output: pw_kernel at every width = the LDS-staged kernels at every
     channels-per-hand-over (tune.one_ks), both block widths
  C  pwk_kernel<1> against pwk_kernel<2> (tune.pwk = 2), 1 / 2 / 3 K slabs per wave, ragged frame tiles, the skip half
  D  the tail kernel's first-layer conv on 64- / 96-frame items (tune.tail_t4) = no tail kernel = per-phase launches
  E  every split-K factor of the conv (tune.ksplit_max, tune.ksplit_blocks), fp32 and split-bf16

The networks run with blocked accumulation (the default: every 32x32 conv width contracts in the same 32-channel blocks)."""
import functools
from collections import namedtuple

import torch

from oracle import diffroll_ref as R

DEFAULTS = {"tune.tile": 0, "tune.pw": 1, "tune.pw_nw": 0, "tune.pwk": 1, "tune.ksplit_max": 16, "tune.ksplit_blocks": 0,
            "tune.one_ks": 0, "tune.stack_fl": 0, "tune.tail_t4": 0, "tune.xcd_n": -1, "tune.xcd_model": 1}
W = 0.5                 # guidance weight of the guided cases
STEP_T = 2              # the diffusion step of the single reverse step
N_CUS = 256

# steps: timesteps of the network (group D runs the whole chain)
Case = namedtuple("Case", "group name C L k sampler B T precision steps")
# pins: {option: value}; info: what the set forces, for claim()
PinSet = namedtuple("PinSet", "label pins info")


def pin(**kw):
    return {"tune." + k: v for k, v in kw.items()}


def with_defaults(pins):
    """the form tuning_pins.pinned takes: option -> (value, default)"""
    return {k: (v, DEFAULTS[k]) for k, v in pins.items()}


def case_id(c):
    return c.name


def hp_of(c):
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=c.C, residual_layers=c.L, kernel_size=c.k, timesteps=c.steps)
    return hp


def guided(c):
    return c.sampler.startswith("cfdg")


def max_dil(c):
    return max(R.layer_dilation(hp_of(c), i) for i in range(c.L))


# ------------------------------------------------------------------------------------------------------------- A
A_NET = dict(C=128, L=3, k=9, steps=6)            # dilations 1 / 2 / 4; two 128-row M tiles
CASES_A = [
    Case("A", "A-ddpm-T97", sampler="ddpm_x0", B=8, T=97, precision="f32", **A_NET),          # 1-frame last tile at 96 frames per block
    Case("A", "A-ddpm-T161", sampler="ddpm_x0", B=8, T=161, precision="f32", **A_NET),        # ... at 160
    Case("A", "A-cfdg-T97", sampler="cfdg_ddpm_x0", B=8, T=97, precision="f32", **A_NET),     # the pair's shared first-layer conv
    Case("A", "A-cfdg-T97-bf16x3", sampler="cfdg_ddpm_x0", B=8, T=97, precision="bf16x3", **A_NET),
    # full width, 64 clips: 18.9 MB of conv weights (beyond an XCD's 4 MiB of L2) against 25 - 34 MB of activations - the one
    # case here whose conv launches the two traffic rules map differently (tune.xcd_model = 0: mapping 1; the model: 0)
    Case("A", "A-ddpm-B64-T161-C512", C=512, L=1, k=9, steps=6, sampler="ddpm_x0", B=64, T=161, precision="f32"),
]
A_RULES_DIFFER = "A-ddpm-B64-T161-C512"


def pins_a(c):
    if c.name == A_RULES_DIFFER:
        return [PinSet(f"tile{t}-ks1", pin(tile=t, ksplit_max=1), dict(tile=t, ksplit_max=1)) for t in (3201, 3202)]
    tiles = (3201, 3202) if c.precision != "f32" else (3201, 3202, 3203, 3205, 1603, 1605)
    sets = [PinSet(f"tile{t}-ks{m}", pin(tile=t, ksplit_max=m), dict(tile=t, ksplit_max=m)) for t in tiles for m in (1, 16)]
    if c.precision == "f32":        # (the split-bf16 1x1 has one flavour)
        sets += [PinSet(f"pw_nw{n}", pin(pw_nw=n), dict(pw_nw=n)) for n in (2, 3, 4, 5)]
        sets += [PinSet(f"pw0-tile{t}", pin(pw=0, tile=t), dict(pw=0, tile=t)) for t in (3201, 3202)]
    return sets


# ------------------------------------------------------------------------------------------------------------- B
CASES_B = [c._replace(group="B", name="B" + c.name[1:]) for c in CASES_A if c.precision == "f32" and c.C == 128]
CASES_B.append(Case("B", "B-ddpm-T97-C192", C=192, L=3, k=9, steps=6, sampler="ddpm_x0", B=8, T=97, precision="f32"))   # 6 K slabs


def pins_b(c):
    sets = [PinSet(f"pw_nw{n}", pin(ksplit_max=1, pw_nw=n), dict(pw_nw=n, ksplit_max=1)) for n in (2, 3, 4, 5)]
    for t in (3201, 3202):
        for ks in (1, 2, 4):
            # what the launch takes: the forced value where it divides the K slabs and fits the LDS (128-frame blocks
            # hold 64 channels beside the read-modify-write tile), else the unforced choice - 2 in every such case here
            slabs = c.C // 32
            fits = not (t == 3202 and ks == 4)
            took = ks if slabs % ks == 0 and fits else 2
            sets.append(PinSet(f"pw0-tile{t}-one_ks{ks}", pin(ksplit_max=1, pw=0, tile=t, one_ks=ks),
                               dict(pw=0, tile=t, ksplit_max=1, ks=took)))
    return sets


# ------------------------------------------------------------------------------------------------------------- C
C_SHAPES = [(1, 1), (2, 31), (1, 33), (3, 65), (2, 97)]       # (B, T): one frame, ragged 32- / 64-frame tiles, several tiles
CASES_C = [Case("C", f"C-C{C}-B{B}-T{T}", C=C, L=2, k=3, steps=6, sampler="cfdg_ddpm_x0", B=B, T=T, precision="f32")
           for C in (128, 256, 384) for B, T in C_SHAPES]     # 1 / 2 / 3 K slabs per wave


def pins_c(c):
    return [PinSet(f"pwk{w}", pin(pwk=2, pw_nw=w), dict(pwk=w)) for w in (1, 2)]


# ------------------------------------------------------------------------------------------------------------- D
D_ROWS = [(128, 2, 9, 2, 97, 1), (192, 2, 15, 2, 200, 2), (64, 2, 3, 4, 1, 1), (128, 2, 9, 2, 161, 5)]     # C, L, k, B, T, stack flavour
CASES_D = [Case("D", f"D-C{C}-k{k}-B{B}-T{T}-fl{f}", C=C, L=L, k=k, steps=3, sampler="cfdg_ddpm_x0", B=B, T=T, precision="f32")
           for C, L, k, B, T, f in D_ROWS]
D_FLAVOUR = {c.name: row[5] for c, row in zip(CASES_D, D_ROWS)}


def pins_d(c):
    f = D_FLAVOUR[c.name]
    twin = dict(stack_fl=f, ksplit_max=1, tile=3200 + f, pw_nw=5 if f == 5 else 2 * f)      # as tests/test_gpu_fused.py pins them
    return [PinSet(f"t4-{n}", pin(tail_t4=n, **twin), dict(t4=n, fl=f, tile=3200 + f, pw_nw=twin["pw_nw"], ksplit_max=1)) for n in (1, 3)]


# ------------------------------------------------------------------------------------------------------------- E
E_NET = dict(C=512, L=1, k=9, steps=6, sampler="ddpm_x0", B=1, T=97)      # 8 M tiles x 2 64-frame tiles = 16 tiles, 16 K slabs
CASES_E = [Case("E", "E-f32", precision="f32", **E_NET), Case("E", "E-bf16x3", precision="bf16x3", **E_NET)]


def pins_e(c):
    if c.precision != "f32":
        return [PinSet("ks16", pin(tile=3201, ksplit_max=16), dict(tile=3201, ksplit=16))]
    sets = [PinSet(f"ks{m}", pin(tile=3201, ksplit_max=m), dict(tile=3201, ksplit=m)) for m in (2, 4, 8, 16)]
    return sets + [PinSet("blocks64", pin(tile=3201, ksplit_blocks=64), dict(tile=3201, ksplit=4))]


CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E
PIN_SETS = {"A": pins_a, "B": pins_b, "C": pins_c, "D": pins_d, "E": pins_e}


def pin_sets(c):
    return PIN_SETS[c.group](c)


# ------------------------------------------------------------------------------------------------- what a case reaches
def evaluations(c):
    """The network evaluations a case runs, as run_network sees them: name -> (NB, n_cond, bmod, per-sample steps).
    forward(): B conditional samples; a reverse step: B samples, or under guidance 2 B of B inputs, the first B
    conditional (layer 0's conv is then contracted once per pair: on B samples)."""
    step = (2 * c.B, c.B, c.B, False) if guided(c) else (c.B, c.B, c.B, False)
    if c.group == "D":
        return {"step": step}
    return {"forward": (c.B, c.B, 0, c.group == "C"), "step": step}


LAUNCHES = ("conv0", "conv", "pw", "half")      # layer 0's conv, a later conv at the largest dilation, the 1x1, the last layer's skip half


def claim(c, ps, ev, launch):
    """What launch `launch` of evaluation `ev` takes under pin set `ps`: a dict with any of
         tile   (flavour, n) of launch_plan.h: Tile
         flavour  the flavour alone
         ksplit split-K factor (gemm_kernel launches)
         ks     32-channel slabs per hand-over of an LDS-staged 1x1
         xcd1   the block -> XCD mapping under tune.xcd_n = 1
       and None for "half" where the last layer's 1x1 is one launch over all rows.  Stated from the issue's rules, not read
       off the planner."""
    i = ps.info
    dual = ev == "step" and guided(c)
    conv = launch in ("conv0", "conv")
    mt = c.C // 64 if launch != "half" else c.C // 64 - c.C // 128
    # the skip half is a launch of its own beside pw_kernel / pwk_kernel only: not beside the LDS-staged kernels (tune.pw = 0, the
    # split-bf16 1x1, an under-filled launch with K splitting pinned off)
    nb = evaluations(c)[ev][0]
    under_filled = (c.C // 64) * nb * ((c.T + 63) // 64) <= 128          # cannot fill half the chip even with 64-frame blocks
    staged = c.precision != "f32" or i.get("pw") == 0 or (under_filled and "pw_nw" not in i and i.get("ksplit_max") == 1)
    if launch == "half" and staged:
        return None
    want = {}
    if c.group in ("A", "B", "D", "E") and conv and "tile" in i:
        fl, n = (1 if i["tile"] // 100 == 16 else 0), i["tile"] % 100
        if fl == 1 and launch == "conv0" and dual:
            want["flavour"] = 0              # the pair's shared contraction exists on the 32x32 kernels only
        else:
            want["tile"] = (fl, n)
    if c.group == "A":
        if conv:
            want.setdefault("flavour", want["tile"][0] if "tile" in want else 0)      # (blocked accumulation: never the 16x16 kernels unforced)
            if want.get("tile", (0,))[0] == 0 and "ksplit_max" in i:
                want["ksplit"] = 4 if i["ksplit_max"] == 16 else 1
            want["xcd1"] = 1
        elif "pw_nw" in i:
            want.update(tile=(2, i["pw_nw"]), xcd1=1 if mt > 1 else 0)
        elif "pw" in i:
            want.update(tile=(0, i["tile"] % 100), xcd1=1)
        elif c.precision != "f32":
            want.update(tile=(0, 1), xcd1=1)
        elif under_filled and i["ksplit_max"] == 16:
            want.update(flavour=3, xcd1=0)          # pwk_kernel, which has one mapping
        elif not under_filled:
            want.update(flavour=2, xcd1=1 if mt > 1 else 0)
    elif c.group == "B":
        if conv:
            want.update(flavour=0, ksplit=1)
        elif "pw_nw" in i:
            want["tile"] = (2, i["pw_nw"])
        else:
            want.update(tile=(0, i["tile"] % 100), ks=i["ks"], ksplit=1)
    elif c.group == "C":
        if not conv:
            want["tile"] = (3, i["pwk"])
    elif c.group == "D":
        if conv:
            want["ksplit"] = 1
        else:
            want["tile"] = (2, i["pw_nw"])
    elif c.group == "E":
        if conv:
            want["ksplit"] = i["ksplit"]
    return want


# ------------------------------------------------------------------------------------------------------- inputs, oracle
@functools.lru_cache(maxsize=None)
def params(c):
    return R.synthetic_params(hp_of(c), seed=1000 + c.C + c.k)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(wav, x, z, per-sample steps, chain noise) - shared, never modified"""
    g = torch.Generator().manual_seed(c.B * 1000 + c.T)
    wav = 0.1 * torch.randn(c.B, max(c.T * 512, 2048), generator=g)      # (reflect padding needs more than n_fft / 2 samples)
    x = torch.randn(c.B, 1, c.T, 88, generator=g)
    z = torch.randn(c.B, 1, c.T, 88, generator=g)
    if c.group == "C":
        t = torch.tensor([(5 - 2 * b) % c.steps for b in range(c.B)])    # differing entries: 5, 3, 1
    else:
        t = torch.tensor(STEP_T).repeat(c.B)
    noise = torch.randn(c.steps, c.B, 1, c.T, 88, generator=g)
    return wav, x, z, t, noise


def _kind(c):
    return {"C": "per_sample_steps", "D": "chain"}.get(c.group, "uniform")


@functools.lru_cache(maxsize=None)
def _reference(net, kind):
    c = next(x for x in CASES if x[2:8] + (x.steps,) == net and _kind(x) == kind)
    hp, p = hp_of(c), params(c)
    wav, x, z, t, noise = inputs(c)
    with torch.no_grad():
        if kind == "chain":
            return (R.sample_chain(p, hp, c.sampler, x, wav, noise, w=W),)
        sch = R.schedule(hp["beta_start"], hp["beta_end"], hp["timesteps"])
        fwd, _ = R.forward(p, hp, x, wav, t)
        step = R.reverse_step(p, hp, sch, c.sampler, x, R.frontend(wav, hp, c.T), STEP_T, z, W if guided(c) else 0.0)
    return fwd, step


def reference(c):
    """the oracle's (forward, one reverse step) - group D: (the whole chain,) - computed once per network, shape and kind
    of call (the cases of groups A and B share theirs, whatever the precision), never modified"""
    return _reference(c[2:8] + (c.steps,), _kind(c))
