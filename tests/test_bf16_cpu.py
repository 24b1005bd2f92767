"""Precision "bf16" (DR_PRECISION_BF16) without a GPU: the restatement tests/bf16_ref.py and the bands the GPU test
(tests/test_gpu_bf16.py) holds the kernels to, the rounding itself, the boundary, the façade, the command line and the
launch plan.

Why bands and not element-wise parity: two correct implementations of the mode differ by an accumulation order, a 1e-7
difference flips an occasional operand's rounding, each flip is a 2^-8 relative change and the layers amplify it.  The
SIZE of the error against the float64 network is stable: the fp32- and the fp64-accumulated restatement agree to a few
parts in a thousand in rms, a truncating implementation is 2.3 - 3.2 x worse.  The GPU test's bands (0.5 .. 1.15 x the
restatement's rms, 2 x its max) therefore admit every correct implementation and refuse both the exact path (four orders
of magnitude below) and a truncating one."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bf16_ref as Q
import chain_ref
from diffroll_amd import _cabi
from oracle import diffroll_ref as R
from facade_fakes import clip, facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_precisions_name_the_headers_value():
    assert _cabi.PRECISIONS["bf16"] == 2 and _cabi.PRECISIONS["bf16x3"] == 1 and _cabi.PRECISIONS["f32"] == 0
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    assert int(re.search(r"DR_PRECISION_BF16 = (\d+)", text).group(1)) == _cabi.PRECISIONS["bf16"]
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", text).group(1)) == 11 == _cabi.DR_ABI_VERSION
    # the contract is in the header, at the enum
    doc = re.sub(r"\s+", " ", text[text.index("DR_PRECISION_BF16 = 2"):text.index("/* which spectrogram a dr_forward")])
    for word in ("round to nearest even", "fp32", "diffusion_projection", "sigmoid * tanh", "output projection", "truncated"):
        assert word in doc, word


def test_null_handle_is_refused():
    assert _cabi.PRECISIONS["bf16"] == 2
    if os.path.exists(_cabi.LIB_PATH):               # (built: a load failure is a failure, not a skip)
        assert _cabi.load_library().dr_set_precision(None, 2) == _cabi.DR_EINVAL


def test_identity_rounding_is_the_oracle_bit_for_bit():
    assert "bf16" in _cabi.PRECISIONS
    hp, p, x, wav, t = Q.case_inputs((64, 3, 9, 2, 40))
    with torch.no_grad():
        spec = R.frontend(wav, hp, 40)
        want = R.denoise(p, hp, x, spec, t)
    assert torch.equal(Q.denoise(p, hp, x, spec, t), want)
    assert R.residual_block.__module__ == "oracle.diffroll_ref"          # the patch is gone
    assert not torch.equal(Q.denoise(p, hp, x, spec, t, rnd=Q.rne), want)


def rne_bits(u: np.ndarray) -> np.ndarray:
    """device_common.h: bf16_rne_bits on uint32 patterns."""
    u = u.astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)


def test_rne_agrees_with_the_kernels_integer_formula():
    assert "bf16" in _cabi.PRECISIONS
    pats = np.array([
        0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,      # ties to even (both ways), just off a tie
        0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008000, 0x0000FFFF,      # denormals (a tie among them, the largest)
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                              # +-0, +-inf
        0x7F7FFFFF, 0x7F7F7FFF,                                                      # the largest finite value rounds to inf; one below the tie does not
        0x3F800000, 0x40490FDB, 0xC2F6E979,
    ], dtype=np.uint32)
    rng = np.random.default_rng(3).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    rng = rng[(rng & 0x7F800000) != 0x7F800000]                                      # (finite: NaN patterns are looked at below)
    u = np.concatenate([pats, rng])
    got = Q.rne(torch.from_numpy(u.view(np.float32).copy())).numpy().view(np.uint32)
    assert np.array_equal(got, rne_bits(u))
    assert np.all((got & 0xFFFF) == 0)
    # the canonical NaN stays a NaN in both
    nan = np.array([0x7FC00000], dtype=np.uint32)
    assert np.isnan(rne_bits(nan).view(np.float32)).all() and torch.isnan(Q.rne(torch.from_numpy(nan.view(np.float32).copy()))).all()
    # float64 input: rounded as its float32
    x64 = torch.from_numpy(pats[:6].view(np.float32).astype(np.float64))
    assert np.array_equal(Q.rne(x64).float().numpy().view(np.uint32), rne_bits(pats[:6]))
    # truncation drops the low half and nothing else
    assert np.array_equal(Q.truncate(torch.from_numpy(u.view(np.float32).copy())).numpy().view(np.uint32), u & 0xFFFF0000)


@pytest.mark.parametrize("geometry", Q.GEOMETRIES, ids=lambda g: "C%d-L%d-k%d-B%d-T%d" % g)
def test_the_gpu_tests_bands_discriminate_and_the_reference_fits_them(geometry):
    """Per geometry of the GPU test, conditional and unconditional: the two restatements lie within 3 % of each other in
    rms error against float64 and within 1.4 x in max; the truncating one is at least 2 x in rms."""
    assert "bf16" in _cabi.PRECISIONS
    hp, p, x, wav, t = Q.case_inputs(geometry)
    with torch.no_grad():
        spec = R.frontend(wav, hp, geometry[4])
    for uncond in (False, True):
        sp = torch.full_like(spec, -1.0) if uncond else spec
        ref64, e = Q.errors(p, hp, x, sp, t, truncating=True)
        print(geometry, "uncond" if uncond else "cond", {k: ("%.3e" % v[0], "%.3e" % v[1]) for k, v in e.items()})
        (r32, m32), (r64, m64), (rt, _) = e["f32"], e["f64"], e["trunc"]
        assert 1 / 1.03 <= r32 / r64 <= 1.03, (geometry, uncond, e)
        assert 1 / 1.4 <= m32 / m64 <= 1.4, (geometry, uncond, e)
        assert rt >= 2.0 * r32, (geometry, uncond, e)
        # the exact path is far below the band's lower edge
        with torch.no_grad():
            exact = Q.rms(R.denoise(p, hp, x, sp, t).double() - ref64)
        assert exact < 0.01 * r32, (geometry, uncond, exact, r32)


@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "generation_ddpm_x0"])
def test_the_chain_band_of_the_gpu_test(sampler):
    """The 8-step chains of the GPU test: the rms distance from the oracle's fp32 chain of the fp32- and the
    fp64-accumulated restated chain stay within 0.8 .. 1.25 of each other."""
    assert "bf16" in _cabi.PRECISIONS
    hp, p, x, spec, nz = chain_inputs()
    sc = None if sampler == "generation_ddpm_x0" else spec
    ref = chain_ref.sample_chain(p, hp, sampler, x, sc, nz, 0, w=0.5)
    a = Q.rms(Q.sample_chain(Q.rne, None, p, hp, sampler, x, sc, nz, 0, w=0.5) - ref)
    b = Q.rms(Q.sample_chain(Q.rne, torch.float64, p, hp, sampler, x, sc, nz, 0, w=0.5) - ref)
    print(sampler, a, b)
    assert a > 1e-5 and 0.8 <= a / b <= 1.25, (sampler, a, b)


def chain_inputs():
    hp, p, x, wav, _ = Q.case_inputs(Q.CHAIN_GEOMETRY, timesteps=Q.CHAIN_STEPS)
    B, T = Q.CHAIN_GEOMETRY[3:]
    nz = torch.randn(Q.CHAIN_STEPS, B, 1, T, 88, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        spec = R.frontend(wav, hp, T)
    return hp, p, x, spec, nz


def test_the_facade_sets_the_mode_once_and_no_option():
    assert "bf16" in _cabi.PRECISIONS
    m, eng = facade("cfdg_ddpm_x0", precision="bf16")
    assert eng.precision == "bf16"                  # the constructor's keyword reached the engine at its first use
    m, eng = facade("cfdg_ddpm_x0")
    m.precision = "bf16"
    wav, x, z, nz = clip(2, 24)
    m.sample(x, wav, noise=nz)
    m.sample(x, wav, noise=nz)
    talk = eng.talk()
    assert [c for c in talk if c[0] == "set_precision"] == [("set_precision", "bf16")], talk
    assert not [c for c in talk if c[0].startswith("set_") and c[0] != "set_precision"], talk
    # the attribute works the same way, and a third mode is not a second spelling of one of the others
    m.precision = "f32"
    m.sample(x, wav, noise=nz)
    m.precision = "bf16"
    m.sample(x, wav, noise=nz)
    assert [c for c in eng.talk() if c[0] == "set_precision"] == [("set_precision", "f32"), ("set_precision", "bf16")]


def test_command_line():
    from diffroll_amd import cli
    assert cli.build_config(["task=generation", "precision=bf16"])["precision"] == "bf16"
    assert cli.build_config(["task=generation", "precision=bf16x3"])["precision"] == "bf16x3"
    assert cli.build_config(["task=generation"])["precision"] == "f32"
    with pytest.raises(SystemExit) as err:
        cli.build_config(["task=generation", "precision=fp16"])
    assert "bf16" in str(err.value) and "fp16" in str(err.value)


PLAN_DRIVER = r"""
    #include <cstdio>
    #include "launch_plan.h"
    int main() {
        // config 2 of bench.py per GPU: 16 guided clips of 125 frames, C = 512, L = 15, k = 9, dilations up to 8, 256 CUs
        for (int prec = 0; prec <= 2; ++prec) {
            dr::NetShape s{32, 16, 16, 125, 512, 15, 9, 8, prec, 256, 1, 2, 1, false, true};
            const dr::NetPlan p = dr::plan_network(s, dr::PlanKnobs{});
            const size_t lds = !p.stack_fl ? 0 : prec ? dr::stack3_lds_bytes(p.stack_fl, s.K, s.max_dil, prec)
                                                      : dr::stack_lds_bytes(p.stack_fl, s.K, s.max_dil);
            const dr::Tile pw = dr::pick_pointwise_tile(dr::PlanKnobs{}, 8, 32, 125, prec);
            printf("%d %d %d %d %d %zu %zu %zu %d,%d\n", prec, p.stack_fl, p.stack_chunks, (int)p.fused_step, (int)p.use_tail, lds,
                   dr::gemm_lds_bytes(2, 1, 9, 8, prec, dr::EPI_GATE), dr::gemm_lds_bytes(1, 4, 1, 1, prec, dr::EPI_RES_SKIP), pw.flavor, pw.n);
        }
        // a channel count that is no multiple of 128: no fused flavour in either reduced precision
        for (int prec = 1; prec <= 2; ++prec) {
            dr::NetShape s{32, 16, 16, 125, 192, 3, 9, 4, prec, 256, 2, 2, 1, false, true};
            printf("%d\n", dr::plan_network(s, dr::PlanKnobs{}).stack_fl);
        }
        return 0;
    }
"""


def test_launch_plan_at_config_2(tmp_path):
    assert "bf16" in _cabi.PRECISIONS
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "bf16_plan.cpp"
    src.write_text(PLAN_DRIVER)
    exe = tmp_path / "bf16_plan"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    by = {int(r[0]): r for r in rows[:3]}
    for prec in (1, 2):
        _, fl, chunks, fused_step, use_tail, lds, conv, pw, tile = by[prec]
        assert int(fl) in (1, 2) and int(chunks) >= 1, by[prec]          # a fused stack flavour
        assert (fused_step, use_tail) == ("0", "0"), by[prec]            # the tail kernel is fp32 only
        assert tile == "0,1", by[prec]                                   # the LDS-staged 1x1 of that precision
    assert by[0][3:5] == ["1", "1"]                                       # (exact fp32 takes the fused step here)
    assert by[2][1] == by[1][1]                                           # the same flavour as bf16x3 ...
    assert 0 < int(by[2][5]) < int(by[1][5]) <= 160 * 1024                # ... in less LDS
    assert 3 * int(by[2][6]) == int(by[1][6])                             # X tiles of a third the rows
    assert rows[3:] == [["0"], ["0"]]
