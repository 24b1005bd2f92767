"""Probe networks: ONE layer of a 16-bit mode read out element by element through the unchanged forward call - test
infrastructure, not collected.

A deep bf16 / f16 network cannot be held element-wise (tests/bf16_ref.py says why); one contraction can: products of two
bf16 or binary16 values are exact in fp32 and the accumulation is fp32, so a layer's output is fixed to fp32 accuracy once
its operands are known exactly.  A probe of layer l of an L-layer network chooses weights that make them known, and that
carry the layer's output unchanged to the network's output:

  exact input    input_projection is one-hot (channel c reads pitch c % 88, bias 0), x_t is drawn from {0 .. 15} / 8, every
                 diffusion_projection has weight 0 and a bias from {-16 .. 15} / 8: x + d is exact in fp32 and representable
                 in bf16 and binary16 whatever the embedding MLP computes.
  pass-through   every layer but l (and the read-out layer of the residual probe) has output_projection = 0: no residual,
                 no skip, so layer l reads x divided l times by fp32(sqrt 2) in IEEE fp32 (diffroll_amd/csrc/device_common.h:
                 div_sqrt2; torch's division is the same operation).
  read-out       L is 1 or 4, so skip / sqrt(L) is exact.  skip_projection holds the rows +e_c and -e_c for up to 88 channels
                 at a time (bias 0), the final output_projection subtracts each pair: pitch i = relu(s_c) - relu(-s_c) = s_c /
                 sqrt(L), one of the two terms being 0.  ceil(C / min(88, C / 2)) forward calls read every channel, frame
                 and clip; the pitches a call does not use must come back as exact zeros.

Three probes (network()):
  "conv"       layer l keeps its random dilated_conv and conditioner_projection; the skip half of its output_projection is the
               identity, the residual half 0.  Read: the layer's (rounded) gated activation G.
  "pointwise"  layer l's output_projection is the random one.  Read: its skip half, W_skip G + b.
  "residual"   layer l keeps the random residual half (its skip half is 0, so that the skip sum holds the read-out alone);
               layer l + 1 passes its rounded input through: the filter rows of its conv are one-hot at (c, centre tap), the
               gate rows have weight 0 and bias 30 (sigmoid = 1 in fp32), its conditioner is 0, its output_projection the
               identity on the skip half.  Read: rnd(tanh(rnd(h_l + d_{l+1}))) - the only way to see the epilogue that writes
               the next layer's rounded input.

The references are float64 statements of the same operands (gate(), check_*); the bounds are those of the formats, of fp32
accumulation, and - for the gate - a delta measured per case on the CPU, between the fp32 and the float64 statement: never
from the engine's output.  faulted() restates bf16_ref.residual_block with one of four faults, for the test that shows
what the probe sees and the network-wide error bands do not.
"""
import collections
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

import bf16_ref as Q
import f16_ref as H
from oracle import diffroll_ref as R

# (C, L, k, dilation_base, dilation_bound, l, B, T): the smallest at which each code path of the 16-bit kernels can go wrong
CASES = [
    (128, 1, 3, 2, 4, 0, 1, 1),        # one frame, halo 1
    (128, 4, 9, 2, 4, 0, 2, 65),       # the second 64-frame tile holds one frame
    (128, 4, 15, 2, 4, 3, 2, 129),     # dilation 8: a halo of 56 frames across tiles, a one-frame last tile
    (128, 4, 3, 3, 4, 3, 1, 70),       # dilation 27, the largest the random sweep reaches in f32
    (384, 4, 9, 2, 4, 1, 3, 63),       # six M tiles, residual and skip halves split between tiles, less than one frame tile
    (96, 4, 9, 2, 4, 2, 2, 40),        # padded channels, Cp != C
    (160, 1, 9, 2, 4, 0, 2, 40),       # padded channels, one layer
    (64, 1, 9, 2, 4, 0, 2, 40),        # Cp % 128 != 0: per-phase only
    (512, 1, 9, 2, 4, 0, 1, 33),       # full width
]
SAMPLING_CASE = CASES[1]               # also read with sampling=True (the unconditional spectrogram rows)
FAULT_CASE = (128, 4, 9, 2, 4, 1, 2, 65)      # the CPU test's faults: layer 1, as in the band geometry (128, 3, 9, 2, 65)
ROUND = {"f32": Q.identity, "bf16": Q.rne, "f16": H.rne}
FORMAT = {"bf16": (7, -126), "f16": (10, -14)}          # stored significand bits, exponent of the smallest normal
U = 2.0 ** -24                                           # fp32 unit roundoff
SQRT2 = torch.tensor(math.sqrt(2.0), dtype=torch.float32)


def case_id(case):
    return "C%d-L%d-k%d-base%d-bound%d-l%d-B%d-T%d" % case


def has_residual_probe(case):
    return case[5] + 1 < case[1]


def step16(mode, v):
    """Spacing of the mode's 16-bit format at |v| (float64; subnormals have the smallest normal's; 0 for "f32")."""
    v = v.double().abs()
    if mode == "f32":
        return torch.zeros_like(v)
    bits, emin = FORMAT[mode]
    e = torch.frexp(v)[1] - 1                                        # 2^e <= |v| < 2^(e + 1)
    e = torch.where(v == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.ldexp(torch.ones_like(v), e - bits)


def representable(mode, v):
    """Every element of the fp32 tensor is a value of the mode's format."""
    return bool((ROUND[mode](v) == v).all())


# ---------------------------------------------------------------------------------------------- the networks
@functools.lru_cache(maxsize=None)
def inputs(case):
    """hp, params (exact input, everything else R.synthetic_params'), x_t, wav, t of a case - shared, not to be changed."""
    C, L, k, base, bound, l, B, T = case
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=C, residual_layers=L, kernel_size=k, dilation_base=base, dilation_bound=bound, timesteps=20)
    p = R.synthetic_params(hp, seed=C + k)
    g = torch.Generator().manual_seed(1000 * k + T + B)
    wav = 0.1 * torch.randn(B, max(T * 512, 2048), generator=g)
    x = torch.randint(0, 16, (B, 1, T, 88), generator=g).float() / 8
    t = torch.tensor(13).repeat(B)
    w = torch.zeros(C, 88, 1)
    w[torch.arange(C), torch.arange(C) % 88, 0] = 1.0
    p["input_projection.weight"], p["input_projection.bias"] = w, torch.zeros(C)
    for i in range(L):
        q = f"residual_layers.{i}.diffusion_projection."
        p[q + "weight"] = torch.zeros(C, 512)
        p[q + "bias"] = torch.randint(-16, 16, (C,), generator=g).float() / 8
    p["skip_projection.bias"], p["output_projection.bias"] = torch.zeros(C), torch.zeros(88)
    return hp, p, x, wav, t


def network(case, probe):
    """The parameters of one probe, without the read-out (read() sets skip_projection and the final output_projection)."""
    C, L, k, _, _, l, _, _ = case
    p = dict(inputs(case)[1])
    skip_identity = torch.cat([torch.zeros(C, C), torch.eye(C)]).unsqueeze(-1)
    for i in range(L):
        if i != l:
            q = f"residual_layers.{i}.output_projection."
            p[q + "weight"], p[q + "bias"] = torch.zeros(2 * C, C, 1), torch.zeros(2 * C)
    q = f"residual_layers.{l}.output_projection."
    if probe == "conv":
        p[q + "weight"], p[q + "bias"] = skip_identity, torch.zeros(2 * C)
    elif probe == "residual":
        assert has_residual_probe(case), case
        p[q + "weight"] = torch.cat([p[q + "weight"][:C], torch.zeros(C, C, 1)])
        p[q + "bias"] = torch.cat([p[q + "bias"][:C], torch.zeros(C)])
        n = f"residual_layers.{l + 1}."
        w = torch.zeros(2 * C, C, k)
        w[C + torch.arange(C), torch.arange(C), (k - 1) // 2] = 1.0
        p[n + "dilated_conv.weight"] = w
        p[n + "dilated_conv.bias"] = torch.cat([torch.full((C,), 30.0), torch.zeros(C)])
        p[n + "conditioner_projection.weight"] = torch.zeros_like(p[n + "conditioner_projection.weight"])
        p[n + "conditioner_projection.bias"] = torch.zeros(2 * C)
        p[n + "output_projection.weight"], p[n + "output_projection.bias"] = skip_identity, torch.zeros(2 * C)
    else:
        assert probe == "pointwise", probe
    return p


def read(run, case, params):
    """The probed tensor (B, C, T): run(params) -> (B, 1, T, 88) is called once per group of channels."""
    C, L, _, _, _, _, B, T = case
    n = min(88, C // 2)
    out = torch.empty(B, C, T)
    for c0 in range(0, C, n):
        m = min(C, c0 + n) - c0
        i = torch.arange(m)
        ws, wo = torch.zeros(C, C, 1), torch.zeros(88, C, 1)
        ws[2 * i, c0 + i, 0], ws[2 * i + 1, c0 + i, 0] = 1.0, -1.0
        wo[i, 2 * i, 0], wo[i, 2 * i + 1, 0] = 1.0, -1.0
        y = run(dict(params, **{"skip_projection.weight": ws, "output_projection.weight": wo})).cpu()
        assert tuple(y.shape) == (B, 1, T, 88), (case, tuple(y.shape))
        assert bool((y[..., m:] == 0).all()), (case, c0, "a pitch that reads no channel is not 0")
        out[:, c0:c0 + m, :] = y[:, 0, :, :m].transpose(1, 2) * math.sqrt(L)
    return out


def cpu_spec(case, uncond=False):
    hp, _, _, wav, _ = inputs(case)
    with torch.no_grad():
        spec = R.frontend(wav, hp, case[7])
    return torch.full_like(spec, -1.0) if uncond else spec


def restated(case, spec, rnd, acc=None, fault=None):
    """run() of the CPU restatement: tests/bf16_ref.py's network (faulted() 's block where a fault is given) on `spec`."""
    hp, _, x, _, t = inputs(case)

    def run(params):
        with (Q.patched(rnd, acc) if fault is None else faulted(rnd, acc, fault)), torch.no_grad():
            return R.denoise(params, hp, x, spec, t)
    return run


# ---------------------------------------------------------------------------------------------- the references
def layer_input(case):
    """x_l, the fp32 input of layer l (B, C, T): the exact input divided l times by fp32(sqrt 2)."""
    C, _, _, _, _, l, _, _ = case
    x = inputs(case)[2][:, 0].transpose(1, 2)[:, torch.arange(C) % 88, :].contiguous()
    for _ in range(l):
        x = x / SQRT2
    return x


def shift(case, i):
    """d_i (1, C, 1): what layer i's diffusion_projection adds."""
    return inputs(case)[1][f"residual_layers.{i}.diffusion_projection.bias"][None, :, None]


def gate(case, mode, spec, dtype):
    """The gated activation of layer l BEFORE its rounding, (B, C, T) in `dtype`: the contraction of the rounded input and
    the rounded conv weights, plus bias, plus the conditioner term of `spec`, then sigmoid * tanh."""
    hp, p, _, _, _ = inputs(case)
    _, _, k, _, _, l, _, _ = case
    rnd, q, dil = ROUND[mode], f"residual_layers.{l}.", R.layer_dilation(hp, l)
    y = rnd(layer_input(case) + shift(case, l))                                    # (the sum is an fp32 one)
    u = F.conv1d(y.to(dtype), rnd(p[q + "dilated_conv.weight"]).to(dtype), p[q + "dilated_conv.bias"].to(dtype),
                 padding=R.conv_padding(k, dil), dilation=dil)
    u = u + F.conv1d(spec.to(dtype), p[q + "conditioner_projection.weight"].to(dtype), p[q + "conditioner_projection.bias"].to(dtype))
    a, b = torch.chunk(u, 2, dim=1)
    return torch.sigmoid(a) * torch.tanh(b)


@functools.lru_cache(maxsize=None)
def delta(case, mode, uncond=False):
    """The fp32 error of the pre-rounding gate, measured on the CPU on the case's own inputs: max |fp32 - float64|."""
    spec = cpu_spec(case, uncond)
    return float((gate(case, mode, spec, torch.float32).double() - gate(case, mode, spec, torch.float64)).abs().max())


# worst: (clip, channel, frame) of the largest err / bound, err and bound: there; max: the largest err anywhere; bad: elements outside
Verdict = collections.namedtuple("Verdict", "ok err bound worst bad max")


def verdict(err, bound):
    i = int((err / bound.clamp(min=1e-300)).argmax())
    B, C, T = err.shape
    worst = (i // (C * T), (i // T) % C, i % T)
    return Verdict(bool((err <= bound).all()) and bool(torch.isfinite(err).all()), float(err[worst]), float(bound[worst]), worst,
                   int((err > bound).sum()), float(err.max()))


def check_conv(case, mode, got, spec, dlt, factor=8.0):
    """|got - g64| <= step16(g64) / 2 + factor * delta: half a step of the one rounding, and the fp32 error of what is
    rounded (8 x the CPU's: ~1 ulp transcendentals where libm has half an ulp, and another accumulation order)."""
    g64 = gate(case, mode, spec, torch.float64)
    return verdict((got.double() - g64).abs(), step16(mode, g64) / 2 + factor * dlt)


def _projection(case, mode, G, rows):
    """float64 W G + b over `rows` of layer l's output_projection with the rounded weights, and sum |w g|."""
    p, l = inputs(case)[1], case[5]
    w = ROUND[mode](p[f"residual_layers.{l}.output_projection.weight"][rows, :, 0]).double()
    b = p[f"residual_layers.{l}.output_projection.bias"][rows].double()
    return torch.einsum("oc,bct->bot", w, G.double()) + b[None, :, None], torch.einsum("oc,bct->bot", w.abs(), G.double().abs())


def check_pointwise(case, mode, got, G):
    """The skip half of layer l's 1x1 on the G the conv probe read (exact 16-bit data: both sides contract the same
    operands): |got - ref| <= (C + 2) 2^-24 sum |w g| + 2^-24 |ref| - fp32 accumulation of C exact products and a bias in
    any order, and the final rounding."""
    C = case[0]
    ref, absum = _projection(case, mode, G, slice(C, 2 * C))
    return verdict((got.double() - ref).abs(), (C + 2) * U * absum + U * ref.abs()), absum


def check_residual(case, mode, got, G):
    """got = rnd(tanh(rnd(h_l + d_{l+1}))) against tanh(v), v = h64 + d, h64 = (x_l + W_res G + b) / fp32(sqrt 2) in float64:
        |got - tanh(v)| <= s + max(s, noise),   s = (step16(v) + step16(got)) / 2.
    s: the two roundings, half a step each, through a slope of at most 1.  The second term is what fp32 noise adds: where it
    is below a half step it moves each rounding by at most one further half step (s again: the bound is then step16(v) +
    step16(got)); where h_l and d cancel, v is small, its step is below the fp32 error of h_l (which is that of a number of
    unit size) and the noise itself comes through - (0, 31, 5) of C128-L4-k9-l0-B2-T65 in f16 on the CPU restatement: |v| =
    2e-4, both steps 2^-23, error 3.3e-7.  noise = the fp32 error of h + d - the accumulation bound of check_pointwise plus
    one rounding each of the sum with x_l, the division and the sum with d - and of the device's tanh = 1 - 2 rcp(2^(c v)
    + 1): the argument's rounding (4 |v| u through 2^x), ~1 ulp each for 2^x and rcp, one rounding each for the sum and the
    fma: (4 |v| + 11) u.  Under "f32" nothing is rounded, s = 0 and the bound is the noise alone.
    Returns the verdict and how many elements lie beyond 2 s, the bound without the noise term."""
    C, l = case[0], case[5]
    res, absum = _projection(case, mode, G, slice(0, C))
    x, d = layer_input(case).double(), shift(case, l + 1).double()
    v = (x + res) / float(SQRT2) + d
    noise = (C + 2) * U * absum + 4 * U * (x.abs() + res.abs() + d.abs()) + (4 * v.abs() + 11) * U
    s = (step16(mode, v) + step16(mode, got)) / 2
    err = (got.double() - torch.tanh(v)).abs()
    return verdict(err, s + torch.maximum(s, noise)), int((err > 2 * s).sum())


# ---------------------------------------------------------------------------------------------- faults
FAULTS = ("input_zero", "taps_swapped", "chunk_missed", "tap_missed")


def fault_at(kind, layer, C, k, B, T):
    """One of the four faults at fixed places of a (B, C, T) layer: clip B - 1, channel 37, the last frame (a one-frame
    tile at T = 65) - except the zeroed input element, which sits mid-clip where every tap reads it.  The element that
    misses a tap is the channel's sigmoid row, the swapped taps are those of its tanh row."""
    return dict(kind=kind, layer=layer, b=B - 1, c=37, t=T // 2 if kind == "input_zero" else T - 1, row=37, swap_row=C + 37,
                taps=(1, 2), tap=(k - 1) // 2 - 1, chunk=slice(32, 64))


def faulted_block(params, i, hp, x, emb, spectrogram, rnd, acc, fault):
    """bf16_ref.residual_block (the same statements in the same order: fault=None is held bit-identical to it) with, in
    layer fault["layer"]:
      input_zero    one element of the rounded input is 0
      taps_swapped  one output row's conv weights of two taps swapped
      chunk_missed  the last frame misses one 32-channel K chunk of one tap, in every output row
      tap_missed    ONE pre-gate element misses one tap - what one lane, one corner of a ragged tile really produces"""
    def conv(inp, w, b, **kw):
        if acc is None:
            return F.conv1d(inp, w, b, **kw)
        return F.conv1d(inp.to(acc), w.to(acc), b.to(acc), **kw).to(inp.dtype)
    f = fault if fault is not None and fault["layer"] == i else None
    p = f"residual_layers.{i}."
    k = int(hp["kernel_size"])
    dil = R.layer_dilation(hp, i)
    d = F.linear(emb, params[p + "diffusion_projection.weight"],
                 params[p + "diffusion_projection.bias"]).unsqueeze(-1)
    y = x + d
    cond = F.conv1d(spectrogram, params[p + "conditioner_projection.weight"],
                    params[p + "conditioner_projection.bias"])
    xin, w = rnd(y), rnd(params[p + "dilated_conv.weight"])
    if f and f["kind"] == "input_zero":
        xin = xin.clone()
        assert float(xin[f["b"], f["c"], f["t"]]) != 0
        xin[f["b"], f["c"], f["t"]] = 0
    if f and f["kind"] == "taps_swapped":
        w = w.clone()
        w[f["swap_row"], :, list(f["taps"])] = w[f["swap_row"], :, list(f["taps"])[::-1]]
    y = conv(xin, w, params[p + "dilated_conv.bias"], padding=R.conv_padding(k, dil), dilation=dil) + cond
    if f and f["kind"] in ("chunk_missed", "tap_missed"):
        T = y.shape[-1]
        t = T - 1 + (f["tap"] - (k - 1) // 2) * dil                       # the frame this tap reads at the last frame
        assert 0 <= t < T
        y = y.clone()
        if f["kind"] == "chunk_missed":
            y[:, :, T - 1] -= torch.einsum("oc,bc->bo", w[:, f["chunk"], f["tap"]], xin[:, f["chunk"], t])
        else:
            assert f["t"] == T - 1
            y[f["b"], f["row"], T - 1] -= w[f["row"], :, f["tap"]] @ xin[f["b"], :, t]
    gate_, filt = torch.chunk(y, 2, dim=1)
    y = torch.sigmoid(gate_) * torch.tanh(filt)
    y = conv(rnd(y), rnd(params[p + "output_projection.weight"]), params[p + "output_projection.bias"])
    residual, skip = torch.chunk(y, 2, dim=1)
    return (x + residual) / math.sqrt(2.0), skip


@contextlib.contextmanager
def faulted(rnd, acc, fault):
    """bf16_ref.patched with the faulted block."""
    saved = R.residual_block
    R.residual_block = lambda params, i, hp, x, emb, spectrogram: faulted_block(params, i, hp, x, emb, spectrogram, rnd, acc, fault)
    try:
        yield
    finally:
        R.residual_block = saved
