"""Single layers of the 16-bit modes, element by element, on the GPU.

The precisions "bf16" and "f16" are held as whole networks only to the SIZE of their error (tests/test_gpu_bf16.py,
tests/test_gpu_f16.py): a fault of one element - one lane, one corner of a ragged tile - moves those statistics by nothing
(tests/test_layer_probe_cpu.py measures it).  One contraction of 16-bit operands with fp32 accumulation, though, is fixed to
fp32 accuracy once its operands are known, and tests/probe_ref.py's probe networks make them known and carry a layer's
output unchanged through the public forward call m(x, wav, t).  Per case (the smallest at which each code path of the
one-pass kernels can go wrong), per launch flavour (per-phase, and fused where C % 128 == 0), with every channel, frame and
clip read:

  conv + gate   G, the layer's rounded gated activation, is representable in the mode's format, and
                |G - g64| <= step16(g64) / 2 + 8 delta: g64 the float64 statement of the rounded operands (with the conditioner
                term of the spectrogram the call itself returns), delta the fp32 error of the pre-rounding gate measured on
                the CPU between the fp32 and the float64 statement of the case.
  pointwise     the skip half of the layer's 1x1 on that G (exact 16-bit data, so both sides contract the same operands):
                |got - ref| <= (C + 2) 2^-24 sum |w g| + 2^-24 |ref|, the fp32 accumulation bound.
  residual      through a pass-through layer l + 1: rnd(tanh(rnd(h_l + d))), the epilogue that writes the next layer's rounded
                input, within step16(h64 + d) + step16(got) of tanh(h64 + d) (probe_ref.check_residual: and within fp32 noise
                where h_l and d cancel and that is more).

precision "f32" runs first, as the anchor: there nothing is rounded, the bounds are the fp32 terms alone (8 delta for the gate),
and a failure means that the read-out or the input contract is wrong, not a 16-bit kernel.  Observed margins:
profiles/layer_probe_margins.txt (DR_PARITY_LOG)."""
import os

import pytest
import torch

import probe_ref as P
from testlib import make_model

pytestmark = pytest.mark.gpu


def _log(line):
    print(line)
    log = os.environ.get("DR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def _record(probe, tag, v, dlt=None, note=""):
    """The largest distance anywhere, and distance and bound at the element that uses most of its bound."""
    _log(f"layer_probe[{probe},{tag}] max {v.max:.3e}; at {v.worst}: {v.err:.3e} bound {v.bound:.3e}"
         + ("" if dlt is None else f" (delta {dlt:.3e} from the CPU restatement, x 8)") + note)


# (mode is the slower index: every case's f32 anchor runs, and reports, before the first 16-bit probe)
@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_single_layer_element_by_element(mode, case):
    C, L, k, base, bound, l, B, T = case
    hp, _, x, wav, t = P.inputs(case)
    m = make_model(hp, P.network(case, "conv"), precision=mode)
    for uncond in ((False, True) if case == P.SAMPLING_CASE else (False,)):
        dlt = P.delta(case, mode, uncond)
        for fused in ((0, 2) if C % 128 == 0 else (0,)):
            seen = {}

            def run(params):
                m.load_state_dict(params)
                m.engine.set_option("fused_stack", fused)
                got, spec = m(x, wav, t, sampling=uncond)
                seen["launch"], seen["spec"] = m.engine.launch_state()["mode"], spec.cpu()
                if mode != "f32":                        # (as in tests/test_gpu_f16.py; the anchor's flavour is only recorded)
                    assert seen["launch"] == ("fused_stack" if fused else "per_phase"), (case, mode, fused, seen["launch"])
                return got

            G = P.read(run, case, P.network(case, "conv"))
            tag = f"{mode},{P.case_id(case)},{seen['launch']},uncond={int(uncond)}"
            spec = seen["spec"]
            assert tuple(spec.shape) == (B, hp["n_mels"], T) and (not uncond or bool((spec == -1).all())), (case, tuple(spec.shape))
            assert torch.isfinite(G).all(), (case, mode, fused)
            assert P.representable(mode, G), (case, mode, fused, "the gate is not a tensor of the format's values")
            v = P.check_conv(case, mode, G, spec, dlt)
            _record("conv", tag, v, dlt)
            assert v.ok, (case, mode, fused, uncond, v)

            pw = P.read(run, case, P.network(case, "pointwise"))
            v, absum = P.check_pointwise(case, mode, pw, G)
            _record("pointwise", tag, v)
            assert v.ok, (case, mode, fused, uncond, v)
            if C % 64:                                   # (the engine pads to a multiple of 64: C = 96, 160)
                # padded channels (Cp != C) contribute nothing: the sums above run over the C real channels alone, and the
                # distance from them is below ONE average term of any output - which a padded row that took part would add
                assert v.max < float((absum / C).min()), (case, mode, v, float((absum / C).min()))

            if P.has_residual_probe(case):
                rs = P.read(run, case, P.network(case, "residual"))
                assert P.representable(mode, rs), (case, mode, fused)
                v, beyond = P.check_residual(case, mode, rs, G)
                _record("residual", tag, v, note="" if mode == "f32" else f"; beyond the two steps, inside the fp32 noise: {beyond}")
                assert v.ok, (case, mode, fused, uncond, v)
