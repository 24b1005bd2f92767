"""Precision "f16" (DR_PRECISION_F16) without a GPU: the restatement tests/f16_ref.py and the bands the GPU test
(tests/test_gpu_f16.py) holds the kernels to, the host's binary16 rounding, the boundary, the façade, the command line and
the launch plan.

As under bf16 (tests/test_bf16_cpu.py says why) the mode is held to the SIZE of its error against the float64 network, not
element-wise: the fp32- and the fp64-accumulated restatement agree to a fraction of a percent in rms, rounding toward zero
is 2.5 - 3.6 x worse, bf16 7.4 - 8.5 x, the exact path a thousand times better - the GPU test's band (0.5 .. 1.15 x the
restatement's rms, 2 x its max) admits every correct implementation and refuses all of those.  With output-projection
weights scaled into binary16's subnormal range the same band also refuses an MFMA that flushes subnormal operands
(several hundred times worse)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bf16_ref as Q
import chain_ref
import f16_ref as H
from diffroll_amd import _cabi
from oracle import diffroll_ref as R
from facade_fakes import clip, facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffroll_amd", "csrc")


def test_precisions_name_the_headers_value():
    assert _cabi.PRECISIONS == {"f32": 0, "bf16x3": 1, "bf16": 2, "f16": 4}
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    for name, key in (("F32", "f32"), ("BF16X3", "bf16x3"), ("BF16", "bf16"), ("F16", "f16")):
        assert int(re.search(rf"DR_PRECISION_{name} = (\d+)", text).group(1)) == _cabi.PRECISIONS[key], name
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", text).group(1)) == 11 == _cabi.DR_ABI_VERSION
    # the contract is in the header, at the enum; 3 is said to be reserved
    doc = re.sub(r"\s+", " ", text[text.index("DR_PRECISION_F16 = 4"):text.index("/* which spectrogram a dr_forward")])
    for word in ("round to nearest even", "ubnormal", "infinity", "fp32", "four operands", "diffusion_projection", "sigmoid * tanh",
                 "output projection", "NaN", "truncated", "65520"):
        assert word in doc, word
    enum = re.sub(r"\s+", " ", text[text.index("DR_PRECISION_F32 = 0"):text.index("DR_PRECISION_F16 = 4")])
    assert "3 is reserved" in enum


def test_null_handle_is_refused():
    assert _cabi.PRECISIONS["f16"] == 4
    if os.path.exists(_cabi.LIB_PATH):               # (built: a load failure is a failure, not a skip)
        assert _cabi.load_library().dr_set_precision(None, 4) == _cabi.DR_EINVAL


ROUND_DRIVER = r"""
    #include <cstdio>
    #include "f16_round.h"
    int main() {
        unsigned u;
        while (scanf("%x", &u) == 1) {
            float f;
            memcpy(&f, &u, 4);
            const unsigned a = dr::f16_rne_bits(u), b = dr::f16_rne(f);
            if (a != b) return 2;
            printf("%04x\n", a);
        }
        return 0;
    }
"""


def test_host_rounding_header_is_torch_float16_bit_for_bit(tmp_path):
    """diffroll_amd/csrc/f16_round.h (the weight packing's rounding) as a stand-alone program under the address and
    undefined-behaviour sanitizers, against torch.float16."""
    assert "f16" in _cabi.PRECISIONS
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src, exe = tmp_path / "f16_round.cpp", tmp_path / "f16_round"
    src.write_text(ROUND_DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    pats = np.array([
        0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001, 0xBF801000, 0xBF803000,      # ties to even (both ways), just off a tie
        0x33000000, 0x33000001, 0x32FFFFFF, 0xB3000000, 0xB3000001,                  # 2^-25: a tie, rounds to 0; the next float: 2^-24
        0x33800000, 0x33C00000, 0x34200000, 0x34600000, 0x387FA000, 0x387FE000,      # 2^-24, subnormal ties (1.5, 2.5, 3.5 ulp, 1022.5 ulp), ...
        0x387FC000, 0x387FDFFF, 0x387FE001, 0x387FFFFF,                              # the largest subnormal, and ties / near-ties up to the smallest normal
        0x38800000, 0x38800001, 0x38801000, 0xB87FC000, 0xB87FE000,                  # the smallest normal
        0x477FE000, 0x477FEFFF, 0x477FF000, 0x477FF001, 0xC77FEFFF, 0xC77FF000,      # 65504, the float below 65520, 65520 -> inf
        0x47800000, 0x7F7FFFFF, 0xFF7FFFFF,                                          # 65536, FLT_MAX
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x007FFFFF,      # +-0, +-inf, fp32 subnormals
        0x3F800000, 0x40490FDB, 0xC2F6E979, 0x3E99999A,
    ], dtype=np.uint32)
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    rnd = rnd[(rnd & 0x7F800000) != 0x7F800000]                                      # finite
    # random exponents seldom land in binary16's range: a second set with magnitudes 2^-27 .. 2^17
    near = ((rng.integers(100, 145, 4096, dtype=np.uint64) << 23) | rng.integers(0, 2 ** 23, 4096, dtype=np.uint64) |
            (rng.integers(0, 2, 4096, dtype=np.uint64) << 31)).astype(np.uint32)
    nan = np.array([0x7FC00000, 0x7F800001, 0xFFC12345], dtype=np.uint32)
    u = np.concatenate([pats, rnd, near, nan])
    out = subprocess.run([str(exe)], input="".join("%08x\n" % v for v in u), capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got = np.array([int(ln, 16) for ln in out.stdout.split()], dtype=np.uint16)
    assert got.size == u.size
    want = torch.from_numpy(u.view(np.float32).copy()).half().numpy().view(np.uint16)
    n = u.size - nan.size
    bad = np.nonzero(got[:n] != want[:n])[0]
    assert bad.size == 0, [("%08x" % u[i], "%04x" % got[i], "%04x" % want[i]) for i in bad[:8]]
    # a NaN stays a NaN, with its sign
    assert np.isnan(got[n:].view(np.float16)).all() and np.array_equal(got[n:] & 0x8000, (u[n:] >> 16) & 0x8000)
    # what the contract says about the edges, in numbers
    by = dict(zip(u[:pats.size].tolist(), got[:pats.size].tolist()))
    assert by[0x33000000] == 0x0000 and by[0x33000001] == 0x0001 and by[0xB3000000] == 0x8000
    assert by[0x387FC000] == 0x03FF and by[0x38800000] == 0x0400 and by[0x387FFFFF] == 0x0400
    assert by[0x477FE000] == 0x7BFF and by[0x477FEFFF] == 0x7BFF and by[0x477FF000] == 0x7C00 and by[0x7F7FFFFF] == 0x7C00


def test_the_restatements_roundings():
    """tests/f16_ref.py's own roundings: toward zero never grows a magnitude and differs from nearest by at most one
    pattern; flushing changes subnormals only."""
    assert "f16" in _cabi.PRECISIONS
    g = torch.Generator().manual_seed(2)
    x = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 2.0 ** -16, torch.tensor([0.0, -0.0, 65520.0, -65520.0, 1.0])])
    near, rtz, fl = H.rne(x), H.toward_zero(x), H.flush(x)
    assert bool((rtz.abs() <= x.abs()).all()) and bool((rtz.sign() * x.sign() >= 0).all())
    step = (near.half().view(torch.int16).int() - rtz.half().view(torch.int16).int()).abs()
    assert int(step.max()) == 1 and 0.3 < float((step == 1).float().mean()) < 0.7
    assert float(rtz[-3]) == 65504.0 and float(near[-3]) == float("inf")
    sub = near.abs() < 2.0 ** -14
    assert bool((fl[sub] == 0).all()) and torch.equal(fl[~sub], near[~sub]) and int((sub & (near != 0)).sum()) > 1000
    x64 = x.double()
    assert torch.equal(H.rne(x64).float(), near) and H.rne(x64).dtype == torch.float64


@pytest.mark.parametrize("geometry", H.GEOMETRIES, ids=lambda g: "C%d-L%d-k%d-B%d-T%d" % g)
def test_the_gpu_tests_bands_discriminate_and_the_reference_fits_them(geometry):
    """Per geometry of the GPU test, conditional and unconditional: the two restatements lie within 3 % of each other in
    rms error against float64 and within 1.4 x in max; rounding toward zero is at least 2 x in rms, bf16 at least 5 x, the
    exact oracle below 0.01 x."""
    assert "f16" in _cabi.PRECISIONS
    hp, p, x, wav, t = H.case_inputs(geometry)
    with torch.no_grad():
        spec = R.frontend(wav, hp, geometry[4])
    for uncond in (False, True):
        sp = torch.full_like(spec, -1.0) if uncond else spec
        ref64, e = H.errors(p, hp, x, sp, t, also=("rtz", "bf16"))
        print(geometry, "uncond" if uncond else "cond", {k: ("%.3e" % v[0], "%.3e" % v[1]) for k, v in e.items()})
        (r32, m32), (r64, m64), (rz, _), (rb, _) = e["f32"], e["f64"], e["rtz"], e["bf16"]
        assert 1 / 1.03 <= r32 / r64 <= 1.03, (geometry, uncond, e)
        assert 1 / 1.4 <= m32 / m64 <= 1.4, (geometry, uncond, e)
        assert rz >= 2.0 * r32, (geometry, uncond, e)
        assert rb >= 5.0 * r32, (geometry, uncond, e)
        with torch.no_grad():
            exact = H.rms(R.denoise(p, hp, x, sp, t).double() - ref64)
        print("   exact / f16", exact / r32)
        assert exact < 0.01 * r32, (geometry, uncond, exact, r32)


@pytest.mark.parametrize("geometry", H.SUBNORMAL_GEOMETRIES, ids=lambda g: "C%d-L%d-k%d-B%d-T%d" % g)
def test_subnormal_operands_matter_in_the_chosen_case(geometry):
    """Output projections scaled by 2^-10 (compensated exactly in the skip projection): the IEEE restatement's error stays
    where it was without the scaling, its two accumulations agree to 3 %, and flushing subnormal operands is at least 20 x
    worse - so the GPU test's band on this case decides whether the MFMA keeps subnormal operands."""
    assert "f16" in _cabi.PRECISIONS
    hp, p, x, wav, t = H.subnormal_inputs(geometry)
    w = torch.cat([p[f"residual_layers.{i}.output_projection.weight"].flatten() for i in range(geometry[1])])
    frac = float(((H.rne(w).abs() < 2.0 ** -14) & (w != 0)).float().mean())
    assert 0.3 < frac < 0.5, frac                                             # 38 % of the weights are binary16 subnormals
    with torch.no_grad():
        spec = R.frontend(wav, hp, geometry[4])
    _, e = H.errors(p, hp, x, spec, t, also=("flush",))
    hp0, p0, _, _, _ = H.case_inputs(geometry)
    _, e0 = H.errors(p0, hp0, x, spec, t)
    print(geometry, frac, {k: ("%.3e" % v[0], "%.3e" % v[1]) for k, v in e.items()}, "unscaled %.3e" % e0["f32"][0])
    (r32, _), (r64, _), (rf, _) = e["f32"], e["f64"], e["flush"]
    assert 1 / 1.03 <= r32 / r64 <= 1.03, (geometry, e)
    assert 0.5 * e0["f32"][0] <= r32 <= 2.0 * e0["f32"][0] and 2e-5 < r32 < 2e-4, (geometry, e, e0)      # measured: 5.6e-5 / 5.9e-5
    assert rf >= 20.0 * r32, (geometry, e)


def chain_inputs():
    hp, p, x, wav, _ = H.case_inputs(H.CHAIN_GEOMETRY, timesteps=H.CHAIN_STEPS)
    B, T = H.CHAIN_GEOMETRY[3:]
    nz = torch.randn(H.CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        spec = R.frontend(wav, hp, T)
    return hp, p, x, spec, nz


@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "generation_ddpm_x0"])
def test_the_chain_band_of_the_gpu_test(sampler):
    """The 8-step chains of the GPU test: the rms distance from the oracle's fp32 chain of the fp32- and the
    fp64-accumulated restated chain stay within 0.8 .. 1.25 of each other, and is above 1e-6."""
    assert "f16" in _cabi.PRECISIONS
    hp, p, x, spec, nz = chain_inputs()
    sc = None if sampler == "generation_ddpm_x0" else spec
    ref = chain_ref.sample_chain(p, hp, sampler, x, sc, nz, 0, w=0.5)
    a = H.rms(H.sample_chain(H.rne, None, p, hp, sampler, x, sc, nz, 0, w=0.5) - ref)
    b = H.rms(H.sample_chain(H.rne, torch.float64, p, hp, sampler, x, sc, nz, 0, w=0.5) - ref)
    print(sampler, a, b)
    assert a > 1e-6 and 0.8 <= a / b <= 1.25, (sampler, a, b)


def test_the_facade_sets_the_mode_once_and_no_option():
    assert "f16" in _cabi.PRECISIONS
    m, eng = facade("cfdg_ddpm_x0", precision="f16")
    assert eng.precision == "f16"                   # the constructor's keyword reached the engine at its first use
    wav, x, z, nz = clip(2, 24)
    m.sample(x, wav, noise=nz)
    assert not [c for c in eng.talk() if c[0].startswith("set_")]            # ... once: nothing is set again
    m, eng = facade("cfdg_ddpm_x0")
    m.precision = "f16"
    m.sample(x, wav, noise=nz)
    m.sample(x, wav, noise=nz)
    talk = eng.talk()
    assert [c for c in talk if c[0] == "set_precision"] == [("set_precision", "f16")], talk
    assert not [c for c in talk if c[0].startswith("set_") and c[0] != "set_precision"], talk
    # f32 -> f16 -> bf16 -> f16: exactly those calls (the first made above), and no option
    for mode in ("bf16", "f16", "f16"):
        m.precision = mode
        m.sample(x, wav, noise=nz)
    talk = eng.talk()
    assert [c for c in talk if c[0].startswith("set_")] == [("set_precision", "bf16"), ("set_precision", "f16")], talk


def test_command_line():
    from diffroll_amd import cli
    assert cli.build_config(["task=generation", "precision=f16"])["precision"] == "f16"
    for wrong in ("fp16", "half"):
        with pytest.raises(SystemExit) as err:
            cli.build_config(["task=generation", f"precision={wrong}"])
        msg = str(err.value)
        assert wrong in msg and all(repr(name) in msg for name in ("f32", "bf16x3", "bf16", "f16")), msg


PLAN_DRIVER = r"""
    #include <cstdio>
    #include "launch_plan.h"
    static_assert(dr::one_plane16(2) && dr::one_plane16(4) && !dr::one_plane16(0) && !dr::one_plane16(1) && !dr::one_plane16(3), "");
    int main() {
        // config 2 of bench.py per GPU: 16 guided clips of 125 frames, C = 512, L = 15, k = 9, dilations up to 8, 256 CUs
        for (int prec : {2, 4}) {
            dr::NetShape s{32, 16, 16, 125, 512, 15, 9, 8, prec, 256, 1, 2, 1, false, true};
            const dr::NetPlan p = dr::plan_network(s, dr::PlanKnobs{});
            const size_t lds = !p.stack_fl ? 0 : dr::stack3_lds_bytes(p.stack_fl, s.K, s.max_dil, prec);
            const dr::Tile pw = dr::pick_pointwise_tile(dr::PlanKnobs{}, 8, 32, 125, prec);
            printf("%d %d %d %d %d %zu %zu %zu %d,%d %d %zu\n", prec, p.stack_fl, p.stack_chunks, (int)p.fused_step, (int)p.use_tail, lds,
                   dr::gemm_lds_bytes(2, 1, 9, 8, prec, dr::EPI_GATE), dr::gemm_lds_bytes(1, 4, 1, 1, prec, dr::EPI_RES_SKIP), pw.flavor, pw.n,
                   (int)p.fold, dr::weight_slab_bytes(prec));
        }
        // a channel count that is no multiple of 128: no fused flavour
        dr::NetShape s{32, 16, 16, 125, 192, 3, 9, 4, 4, 256, 2, 2, 1, false, true};
        printf("%d\n", dr::plan_network(s, dr::PlanKnobs{}).stack_fl);
        return 0;
    }
"""


def test_launch_plan_at_config_2(tmp_path):
    assert "f16" in _cabi.PRECISIONS
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src, exe = tmp_path / "f16_plan.cpp", tmp_path / "f16_plan"
    src.write_text(PLAN_DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    bf16, f16 = rows[0], rows[1]
    assert (bf16[0], f16[0]) == ("2", "4")
    assert f16[1:] == bf16[1:], (bf16, f16)                              # flavour, chunks, LDS bytes, tile, accumulation, slab: bf16's row
    assert int(f16[1]) in (1, 2) and int(f16[2]) >= 1, f16              # a fused stack flavour
    assert (f16[3], f16[4]) == ("0", "0"), f16                          # no fused step, no tail: the tail kernel is fp32 only
    assert f16[8] == "0,1" and f16[10] == "8192", f16                    # the LDS-staged 1x1; 8 KiB weight slabs
    assert rows[2] == ["0"]                                              # stack_fl == 0 at C = 192
