"""CPU restatement of precision "bf16" (include/diffroll_amd.h: DR_PRECISION_BF16) - test infrastructure.

It is oracle.diffroll_ref.residual_block with a rounding function applied at the four operands the header names - the
input x + diffusion_projection and the weights of the dilated conv, the gated activation sigmoid * tanh and the weights of
the output projection - and nothing else changed: biases, the conditioner term, the residual stream, the skip sum and
everything outside the residual stack are computed as the oracle computes them, in the dtype of the tensors handed in.
acc=torch.float64 contracts the two rounded operand pairs in float64 and rounds the sum once to that dtype: the
"fp64-accumulated" restatement of the same arithmetic, next to the plain fp32-accumulated one (acc=None).

A deep bf16 network cannot be held element-wise to a restatement (one flipped rounding is a 2^-8 relative change that the
layers amplify); what is stable is the SIZE of its error against the float64 network, which is what errors() returns and
the tests compare.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from oracle import diffroll_ref as R

GEOMETRIES = [
    # (C, layers, k, B, T): the smallest that reach every code path of the one-pass bf16 kernels
    (128, 2, 3, 1, 1),        # one frame, one M-tile pair, halo 1
    (128, 3, 9, 2, 65),       # two 64-frame tiles, the second holding one frame
    (128, 3, 15, 5, 129),     # halo 56 frames across tiles, one-frame last tile
    (384, 2, 9, 3, 125),      # 6 M tiles: the residual and skip halves split between tiles
    (512, 2, 9, 3, 125),      # full width
    (64, 2, 9, 2, 40),        # Cp % 128 != 0: the fused flavour refuses it, the per-phase kernels run
]
# (No case in the trained-weight regime of tests/test_gpu_r3.py - weights scaled x4 / x4 or x16 / x8: there the truncating
# restatement is only 1.2 - 1.96 x the rounding one in rms at every geometry above, so the bands of tests/test_bf16_cpu.py
# do not admit it: saturated gates hide part of the operand error.)
CHAIN_GEOMETRY = (128, 3, 9, 2, 65)
CHAIN_STEPS = 8


def identity(x: torch.Tensor) -> torch.Tensor:
    return x


def rne(x: torch.Tensor) -> torch.Tensor:
    """bf16(x), round to nearest even, in x's dtype (float64 goes through float32 first: both roundings are to nearest
    and the second keeps 8 of the first's 24 bits, so a double-rounding flip needs an exact 16-bit tie pattern)."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def truncate(x: torch.Tensor) -> torch.Tensor:
    """The low 16 bits of the fp32 pattern dropped: what the mode must NOT do."""
    bits = x.to(torch.float32).contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(x.dtype)


def residual_block(params, i, hp, x, emb, spectrogram, rnd=identity, acc=None):
    """oracle.diffroll_ref.residual_block (model/diffwave.py:134-151) with rnd at the four operands; acc: the dtype the two
    contractions of rounded operands accumulate in (None: the tensors' own)."""
    def conv(inp, w, b, **kw):
        if acc is None:
            return F.conv1d(inp, w, b, **kw)
        return F.conv1d(inp.to(acc), w.to(acc), b.to(acc), **kw).to(inp.dtype)
    p = f"residual_layers.{i}."
    k = int(hp["kernel_size"])
    dil = R.layer_dilation(hp, i)
    d = F.linear(emb, params[p + "diffusion_projection.weight"],
                 params[p + "diffusion_projection.bias"]).unsqueeze(-1)
    y = x + d
    cond = F.conv1d(spectrogram, params[p + "conditioner_projection.weight"],
                    params[p + "conditioner_projection.bias"])
    y = conv(rnd(y), rnd(params[p + "dilated_conv.weight"]), params[p + "dilated_conv.bias"],
             padding=R.conv_padding(k, dil), dilation=dil) + cond
    gate, filt = torch.chunk(y, 2, dim=1)
    y = torch.sigmoid(gate) * torch.tanh(filt)
    y = conv(rnd(y), rnd(params[p + "output_projection.weight"]), params[p + "output_projection.bias"])
    residual, skip = torch.chunk(y, 2, dim=1)
    return (x + residual) / math.sqrt(2.0), skip


@contextlib.contextmanager
def patched(rnd, acc=None):
    """For the duration of the block every oracle evaluation (R.denoise - and so tests/chain_ref.py's chain, which calls
    it) runs the restated residual block with this rounding."""
    saved = R.residual_block
    R.residual_block = lambda params, i, hp, x, emb, spectrogram: residual_block(params, i, hp, x, emb, spectrogram, rnd, acc)
    try:
        yield
    finally:
        R.residual_block = saved


def denoise(params, hp, x_t, spectrogram, t, table=None, rnd=identity, acc=None):
    """R.denoise on the restated block; any dtype (params, x_t, spectrogram and table in the same one)."""
    with patched(rnd, acc), torch.no_grad():
        return R.denoise(params, hp, x_t, spectrogram, t, table)


def sample_chain(rnd, acc, *args, **kw):
    """tests/chain_ref.py's sample_chain on the restated block."""
    import chain_ref
    with patched(rnd, acc):
        return chain_ref.sample_chain(*args, **kw)


def cast(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


def denoise_as(params, hp, x, spec, t, dtype, rnd, acc=None):
    """One evaluation with everything in `dtype`, returned as float64."""
    table = R.build_embedding(int(hp["timesteps"])).to(dtype)
    return denoise(cast(params, dtype), hp, x.to(dtype), spec.to(dtype), t, table, rnd, acc).double()


def rms(e: torch.Tensor) -> float:
    return float(e.double().pow(2).mean().sqrt())


def errors(params, hp, x, spec, t, truncating=False):
    """float64 network, and (rms, max) error against it of the fp32-accumulated restatement, the fp64-accumulated one and -
    on request - the truncating fp32 one.  Returns (ref64, {"f32": (rms, max), "f64": ..., "trunc": ...})."""
    ref64 = denoise_as(params, hp, x, spec, t, torch.float64, identity)
    out = {}
    for name, rnd, acc in (("f32", rne, None), ("f64", rne, torch.float64)) + ((("trunc", truncate, None),) if truncating else ()):
        e = denoise_as(params, hp, x, spec, t, torch.float32, rnd, acc) - ref64
        out[name] = (rms(e), float(e.abs().max()))
    return ref64, out


def case_inputs(geometry, timesteps=20):
    """hp, params, x (B, 1, T, 88), wav (B, samples), t (B,) of one geometry: shared by the CPU and the GPU test."""
    C, layers, k, B, T = geometry
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=C, residual_layers=layers, kernel_size=k, timesteps=timesteps)
    p = R.synthetic_params(hp, seed=C + k)
    g = torch.Generator().manual_seed(1000 * k + T + B)
    wav = 0.1 * torch.randn(B, max(T * 512, 2048), generator=g)
    x = torch.randn(B, 1, T, 88, generator=g)
    t = torch.tensor(13).repeat(B)
    return hp, p, x, wav, t
