"""Option "exact_below" (include/diffroll_amd.h) without a GPU: the rule of a step's precision (csrc/launch_plan.h:
step_precision), what the option buys on the restated chains (tests/exact_ref.py), the precondition of the band the GPU test
(tests/test_gpu_exact_below.py) holds the mixed chains to, and the surface - header, library, façade, command line,
checkpoint override."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import exact_ref as X
from facade_fakes import clip, facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = X.CHAIN_STEPS


# ---------------------------------------------------------------------------------------------- 1. the rule
RULE_DRIVER = r"""
    #include <cstdio>
    #include "launch_plan.h"
    static_assert(dr::step_precision(DR_PRECISION_BF16, 3, 2) == DR_PRECISION_F32, "a constant expression");
    static_assert(dr::exact_below_ok(0, 8) && dr::exact_below_ok(8, 8) && !dr::exact_below_ok(-1, 8) && !dr::exact_below_ok(9, 8), "range");
    int main() {
        int prec, v, t;
        while (scanf("%d %d %d", &prec, &v, &t) == 3) printf("%d\n", dr::step_precision(prec, v, t));
        return 0;
    }
"""


def test_the_rule_of_a_steps_precision(tmp_path):
    """step_precision over the four modes for v = 0, 1, S - 1 and S with t on either side of v, and the range
    dr_set_option accepts."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "rule.cpp"
    src.write_text(RULE_DRIVER)
    exe = tmp_path / "rule"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    from diffroll_amd import _cabi
    cases = [(prec, v, t) for prec in sorted(_cabi.PRECISIONS.values()) for v in (0, 1, S - 1, S)
             for t in sorted({0, max(v - 1, 0), min(v, S - 1), min(v + 1, S - 1), S - 1})]
    assert len({p for p, _, _ in cases}) == 4
    out = subprocess.run([str(exe)], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(cases)
    for (prec, v, t), got in zip(cases, out):
        assert int(got) == (0 if t < v else prec) == X.step_precision(prec, v, t), (prec, v, t, got)
    # both sides of every boundary were asked
    for v in (1, S - 1, S):
        assert (2, v, v - 1) in cases and (v == S or (2, v, v) in cases)


# ---------------------------------------------------------------------------------------------- 2. what the option buys
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("sampler", X.SAMPLERS)
def test_the_last_two_steps_exact_buy_back_three_quarters_of_the_error(sampler, mode):
    """8 steps on CHAIN_GEOMETRY, w = 0.5: with the last two steps exact the restated chain ends under a quarter as far from
    the fp32 chain as the all-reduced chain (observed ratios 0.019 - 0.050 in both modes)."""
    row = [X.distance(mode, sampler, v) for v in range(S + 1)]
    print(f"\nexact_below[{mode},{sampler},{S} steps] rms distance from the fp32 chain by v = 0 .. {S}: " + " ".join(f"{d:.2e}" for d in row)
          + f"   ratio v=2 / v=0 {row[2] / row[0]:.4f}")
    assert row[S] == 0.0                              # every step exact: the fp32 chain itself
    assert row[0] > 1e-5
    assert row[2] < 0.25 * row[0], (sampler, mode, row)


# ---------------------------------------------------------------------------------------------- 3. the GPU band's precondition
@pytest.mark.parametrize("mode,sampler,v", X.BAND_CASES, ids=["%s-%s-v%d" % c for c in X.BAND_CASES])
def test_the_gpu_band_has_something_to_measure(mode, sampler, v):
    """The restated mixed chains the GPU test compares against end more than 1e-5 rms from the fp32 chain (observed 1.2e-4,
    2.6e-5, 9.4e-5, 1.9e-5, 1.5e-5), and the fp32- and fp64-accumulated restatements stay within 0.8 .. 1.25 of each other -
    the precondition tests/test_bf16_cpu.py states for the band of whole chains."""
    a, b = X.distance(mode, sampler, v), X.distance(mode, sampler, v, torch.float64)
    print(f"\nexact_below band[{mode},{sampler},v={v}] fp32-accumulated {a:.3e} fp64-accumulated {b:.3e} ratio {a / b:.3f}")
    assert a > 1e-5 and b > 1e-5, (a, b)
    assert 0.8 <= a / b <= 1.25, (a, b)


@pytest.mark.parametrize("name,v", X.STATEFUL_BAND, ids=["%s-v%d" % c for c in X.STATEFUL_BAND])
def test_the_stateful_gpu_band_has_something_to_measure(name, v):
    """The same precondition for the combinations whose state runs across the boundary - "cfg_project" + "cfg_momentum" and
    "guidance_stride" 2, restated by their own files (tests/momentum_ref.py, tests/stride_ref.py) with the rounding at the
    steps t >= v: bf16 at v = 1 and v = 3 (observed 1.4e-4, 3.5e-5, 1.3e-4, 1.7e-5)."""
    a, b = X.stateful_distance(name, v), X.stateful_distance(name, v, torch.float64)
    print(f"\nexact_below band[bf16,{name},v={v}] fp32-accumulated {a:.3e} fp64-accumulated {b:.3e} ratio {a / b:.3f}")
    assert a > 1e-5 and b > 1e-5, (a, b)
    assert 0.8 <= a / b <= 1.25, (a, b)


def test_no_band_inside_fp32_noise():
    assert ("bf16", "generation_ddpm_x0", 2) not in X.BAND_CASES       # (6.6e-6: inside the fp32 chain's own noise)
    assert all(v in (1, 2) for _, _, v in X.BAND_CASES)


# ---------------------------------------------------------------------------------------------- 4. the surface
def test_option_is_public_and_documented():
    from diffroll_amd import _cabi
    from diffroll_amd.engine import _MIRRORED, Engine
    from testlib import header_functions
    name = "exact_below"
    assert name in _cabi.PUBLIC_OPTIONS and _MIRRORED[name] == 0 and getattr(Engine, name) == 0
    assert f"'{name}'" in Engine.set_option.__doc__ and f"'{name}'" in Engine.holding.__doc__
    assert _cabi.DR_ABI_VERSION == 11 and sorted(_cabi.PRECISIONS.items()) == [("bf16", 2), ("bf16x3", 1), ("f16", 4), ("f32", 0)]
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", text).group(1)) == 11
    assert len(header_functions()) == len(_cabi.EXPORTS) == 30
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    begin = re.search(r'"exact_below"\s+\[0\]', doc)
    assert begin
    flat = re.sub(r"\s*\n \*\s*", " ", doc[begin.start():doc.index("Unknown names")])
    for word in ("0 (off), or v in 1 .. timesteps", "t < v runs in DR_PRECISION_F32", "t >= v runs in the selected mode",
                 "0 <= v <= timesteps", "DR_EINVAL at the set", "the previous value stays in force", "the real diffusion step",
                 '"sampling_steps"', "dr_step, dr_sample and dr_sample_checked", "healed time-out",
                 "dr_forward and dr_forward_steps", "EXEMPT", "keep the engine's mode", "Under DR_PRECISION_F32 the option is accepted and changes nothing",
                 "DR_MODE_FUSED_STACK_TAIL", "computes its own input layer", "primes nothing", "no refusals",
                 "dr_launch_state reports the last step that ran", "captured chain's key", "byte-identical",
                 "Nothing is known about quality", "INTEGRATION.md 3c"):
        assert word in flat, word
    for doc_name, words in (("README.md", ("exact_below", "profiles/exact_tail_sweep.txt", "profiles/exact_tail_kernel_resources.txt",
                                           "profiles/exact_tail_margins.txt")),
                            ("INTEGRATION.md", ('"exact_below"', "task.sampling.exact_below=")),
                            ("DESIGN.md", ("exact_below",))):
        body = open(os.path.join(ROOT, doc_name)).read()
        for word in words:
            assert word in body, (doc_name, word)
    # the two places that state each sampling option: once in the engine, once in the façade
    state = open(os.path.join(ROOT, "diffroll_amd", "csrc", "engine_state.h")).read()
    assert "int exact_below = 0;" in state and "exact_below == o.exact_below" in state
    from diffroll_amd import schedule
    assert "exact_below" in schedule.sampling_options({"type": "cfdg_ddpm_x0"}, 200)


def test_the_built_library_knows_the_option():
    """Without a GPU no engine exists to set the option on (the range is held on the GPU: tests/test_gpu_exact_below.py).
    Here: the library carries the option's refusal text, and a null handle is DR_EINVAL, never a crash."""
    from diffroll_amd import _cabi
    if not os.path.exists(_cabi.LIB_PATH):
        pytest.skip("the library is not built (python -m diffroll_amd.build)")
    lib = _cabi.load_library()                        # (built: a load failure is a failure, not a skip)
    assert b"exact_below is 0 (off) or v in [1, timesteps = %d]" in open(_cabi.LIB_PATH, "rb").read()
    assert lib.dr_set_option(None, b"exact_below", 5) == _cabi.DR_EINVAL


def test_check_exact_below():
    from diffroll_amd.schedule import check_exact_below
    assert check_exact_below(None, S) == 0 and check_exact_below(0, S) == 0 and check_exact_below(S, S) == S
    assert check_exact_below(3, S) == 3 and check_exact_below(25, 200) == 25
    for bad in (-1, S + 1, 1.5, "5", True, [5]):
        with pytest.raises(ValueError, match=re.escape("exact_below must be") + ".*" + re.escape(repr(bad))):
            check_exact_below(bad, S)


def test_facade_reads_the_value_at_every_use():
    """The façade on the recording engine (tests/facade_fakes.py): the first call sets the option in front of the chain, later
    calls with the same hparams set nothing, a change sets the new value once, None sets 0; a bad value is refused before
    the engine is reached; every sampler and every precision take it."""
    m, eng = facade("cfdg_ddpm_x0", precision="bf16")
    wav, x, _, z = clip(2, 8)
    assert m.exact_below() == 0
    m.hparams.sampling.exact_below = 2
    assert m.exact_below() == 2 and m.sampling_options()["exact_below"] == 2
    m.sample(x, wav, noise=z)
    first = eng.talk()
    assert [c for c in first if c[0] == "set_option"] == [("set_option", "exact_below", 2)] and eng.exact_below == 2
    assert first.index(("set_option", "exact_below", 2)) < [c[0] for c in first].index("sample")
    m.sample(x, wav, noise=z)
    m.sample(x, wav, seed=3)
    assert not [c for c in eng.talk() if c[0] == "set_option"]
    m.hparams.sampling.exact_below = 6                # = timesteps: every step exact
    m.sample(x, wav, noise=z)
    assert [c for c in eng.talk() if c[0] == "set_option"] == [("set_option", "exact_below", 6)]
    m.hparams.sampling.exact_below = None
    m.sample(x, wav, noise=z)
    assert [c for c in eng.talk() if c[0] == "set_option"] == [("set_option", "exact_below", 0)]
    m.hparams.sampling.exact_below = 3
    m.__dict__["_stride1"] = True                     # the reference's single-step methods are chain steps too: the option stays
    assert m.exact_below() == 3
    m.__dict__["_stride1"] = False
    for bad in (7, -1, "2", 2.0, True):
        m.hparams.sampling.exact_below = bad          # refused at use, before the engine is reached
        with pytest.raises(ValueError, match="exact_below must be"):
            m.engine
        with pytest.raises(ValueError, match="exact_below must be"):
            m.sample(x, wav, noise=z)
        assert not eng.talk()
        with pytest.raises(ValueError, match="exact_below must be"):
            facade("cfdg_ddpm_x0", sampling={"exact_below": bad})
    m.hparams.sampling.exact_below = 2
    m.hparams.sampling.update(guidance_interval=[1, 4], solver_order=2, solver_noise=1, steps=4, draws=2, x0_clip=1, guidance_stride=2)
    assert m.exact_below() == 2                       # (it combines with everything: no refusals)
    for sampler in ("ddpm_x0", "generation_ddpm_x0", "ddim", "ddim2ddpm"):
        assert facade(sampler, sampling={"exact_below": 2})[0].exact_below() == 2
    plain, eng2 = facade("cfdg_ddpm_x0")
    plain.sample(x, wav, noise=z)
    assert not [c for c in eng2.talk() if c[0] == "set_option" and c[1] == "exact_below"]
    assert "exact_below" in type(m).sample.__doc__


def test_load_from_checkpoint_override(golden_dir):
    from diffroll_amd import ClassifierFreeDiffRoll
    path = os.path.join(golden_dir, "trained_small.ckpt")
    got = ClassifierFreeDiffRoll.load_from_checkpoint(path, precision="bf16", sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "exact_below": 25})
    assert got.exact_below() == 25 and got.precision == "bf16"
    assert ClassifierFreeDiffRoll.load_from_checkpoint(path).exact_below() == 0
    T = int(got.hparams.timesteps)
    assert ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "exact_below": T}).exact_below() == T
    with pytest.raises(ValueError, match="exact_below must be"):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "exact_below": T + 1})


def test_cli():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "precision=bf16", "task.sampling.w=3", "task.sampling.exact_below=25"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 3, "exact_below": 25} and cfg["precision"] == "bf16"
    assert "exact_below" not in cli.build_config(["task=transcription"])["task"]["sampling"]
    assert cli.build_config(["task=transcription", "task.sampling.exact_below=null"])["task"]["sampling"]["exact_below"] is None
    S_cli = cli.build_config(["task=transcription"])["task"]["timesteps"]
    assert cli.build_config(["task=generation", f"task.sampling.exact_below={S_cli}", "task.sampling.steps=50"])["task"]["sampling"]["exact_below"] == S_cli
    for bad in (str(S_cli + 1), "-1", "2.5", "two"):
        with pytest.raises(SystemExit, match="task.sampling.exact_below"):
            cli.build_config(["task=transcription", f"task.sampling.exact_below={bad}"])


def test_sharding_hands_the_option_to_every_rank():
    """sample_shard runs model.sample on the rank's engine: the option travels in hparams.sampling with the model, as the
    precision does."""
    from diffroll_amd import distributed
    m, eng = facade("cfdg_ddpm_x0", precision="f16")
    m.hparams.sampling.exact_below = 2
    wav, x, _, z = clip(4, 8)
    for rank in (0, 1):
        distributed.sample_shard(m, x, wav, z, 0, rank, 2)
    talk = eng.talk()
    assert [c for c in talk if c[0] == "set_option" and c[1] == "exact_below"] == [("set_option", "exact_below", 2)]
    assert len([c for c in talk if c[0] == "sample"]) == 2 and eng.exact_below == 2 and eng.precision == "f16"
    assert "exact_below" in distributed.sample_shard.__doc__
