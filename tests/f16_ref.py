"""CPU restatement of precision "f16" (include/diffroll_amd.h: DR_PRECISION_F16) - test infrastructure.

It is tests/bf16_ref.py's restated residual block - the oracle's, with a rounding function at the four operands the header
names - with IEEE binary16, round to nearest even, subnormals kept, as that rounding.  Geometries, inputs, the chain
wrapper and the float64 comparison are bf16_ref's; what is added is the rounding itself, the two things the mode must NOT
do (rounding toward zero, flushing subnormals) and the subnormal-weight case that tells the last one apart.
"""
import torch

import bf16_ref as Q
from bf16_ref import CHAIN_GEOMETRY, CHAIN_STEPS, GEOMETRIES, case_inputs, rms, sample_chain  # noqa: F401  (lent to the tests)

# the two geometries of the subnormal-weight case: one 33-frame tile of one layer, and two tiles (the second one frame) of two
SUBNORMAL_GEOMETRIES = [(128, 1, 3, 1, 33), (128, 2, 9, 2, 65)]


def rne(x: torch.Tensor) -> torch.Tensor:
    """binary16(x), round to nearest even, in x's dtype (float64 goes through float32 first, as in bf16_ref.rne)."""
    return x.float().half().to(x.dtype)


def toward_zero(x: torch.Tensor) -> torch.Tensor:
    """binary16(x) rounded toward zero (what v_cvt_pkrtz_f16_f32 does): of the two binary16 neighbours of x the one of
    smaller magnitude.  Exact for every finite x whose magnitude binary16 can hold."""
    f = x.float()
    h = f.half()
    over = h.float().abs() > f.abs()                      # rounded away from zero: step one binary16 pattern back
    bits = h.view(torch.int16)
    return torch.where(over, (bits - 1).view(torch.float16), h).to(x.dtype)       # (sign-magnitude: pattern - 1 is toward 0)


def flush(x: torch.Tensor) -> torch.Tensor:
    """binary16(x), round to nearest even, then |h| < 2^-14 -> 0: an MFMA that flushes subnormal operands."""
    h = x.float().half()
    return torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h).to(x.dtype)


def errors(params, hp, x, spec, t, also=()):
    """float64 network, and (rms, max) error against it of the fp32-accumulated restatement ("f32"), the fp64-accumulated one
    ("f64") and the fp32-accumulated restatements with the roundings named in `also`: "rtz", "flush", "bf16".
    Returns (ref64, {name: (rms, max)})."""
    extra = {"rtz": toward_zero, "flush": flush, "bf16": Q.rne}
    ref64 = Q.denoise_as(params, hp, x, spec, t, torch.float64, Q.identity)
    out = {}
    for name, rnd, acc in (("f32", rne, None), ("f64", rne, torch.float64)) + tuple((n, extra[n], None) for n in also):
        e = Q.denoise_as(params, hp, x, spec, t, torch.float32, rnd, acc) - ref64
        out[name] = (rms(e), float(e.abs().max()))
    return ref64, out


def subnormal_inputs(geometry):
    """case_inputs with every residual layer's output projection (weight and bias) scaled by 2^-10 - which puts 38 % of
    those weights below 2^-14, binary16's smallest normal - and skip_projection.weight by 2^10: an exact fp32 compensation
    that keeps the stack visible in the output."""
    hp, p, x, wav, t = case_inputs(geometry)
    p = dict(p)
    for i in range(int(hp["residual_layers"])):
        for leaf in ("weight", "bias"):
            k = f"residual_layers.{i}.output_projection.{leaf}"
            p[k] = p[k] * 2.0 ** -10
    p["skip_projection.weight"] = p["skip_projection.weight"] * 2.0 ** 10
    return hp, p, x, wav, t
