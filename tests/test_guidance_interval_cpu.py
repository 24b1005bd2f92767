"""Guidance interval (options "guidance_t_min" / "guidance_t_max", include/diffroll_amd.h) without a GPU: the options'
names and value rules, the planner's per-step evaluation shapes (csrc/launch_plan.h compiled without HIP, as
tests/test_launch_plan_cpu.py does), the restatement of tests/chain_ref.py with an interval against itself without one, the facade's
hparams.sampling.guidance_interval and the CLI's task.sampling.guidance_interval."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from oracle import diffroll_ref as R

import chain_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin lines:  "opt <is_max> <value> <S>"                           -> guidance_value_ok
#               "empty <lo> <hi> <S>"                                -> GuidanceInterval::empty
#               "step <NB> <n_cond> <B> <lo> <hi> <S> <w_zero> <t> <next_t>" -> plan_step: NB n_cond dual | NB n_cond dual (next)
DRIVER = r"""
    #include <cstdio>
    #include <cstring>
    #include "launch_plan.h"
    int main() {
        char line[256];
        while (fgets(line, sizeof line, stdin)) {
            int a[9];
            if (sscanf(line, "opt %d %d %d", a, a + 1, a + 2) == 3) {
                printf("%d\n", (int)dr::guidance_value_ok(a[0] != 0, a[1], a[2]));
            } else if (sscanf(line, "empty %d %d %d", a, a + 1, a + 2) == 3) {
                dr::GuidanceInterval g; g.lo = a[0]; g.hi = a[1];
                printf("%d %d\n", (int)g.empty(a[2]), g.hi_eff(a[2]));
            } else if (sscanf(line, "step %d %d %d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8) == 9) {
                dr::GuidanceInterval g; g.lo = a[3]; g.hi = a[4];
                const dr::StepShapes p = dr::plan_step(a[0], a[1], a[2], g, a[5], a[6] != 0, a[7], a[8]);
                printf("%d %d %d %d %d %d\n", p.now.NB, p.now.n_cond, (int)p.now.dual, p.next.NB, p.next.n_cond, (int)p.next.dual);
            } else {
                printf("bad line\n");
                return 1;
            }
        }
        return 0;
    }
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("guidance_plan")
    src = d / "guidance_plan_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "guidance_plan_driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def ask(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


# ---------------------------------------------------------------------------------------------- 1. options
def test_option_names_are_public_and_documented():
    from diffroll_amd import _cabi
    assert _cabi.DR_ABI_VERSION == 11
    assert "guidance_t_min" in _cabi.PUBLIC_OPTIONS and "guidance_t_max" in _cabi.PUBLIC_OPTIONS
    for neighbour in ("guidance_t", "guidance_t_mid", "guidance_interval", "guidance_w"):
        assert neighbour not in _cabi.PUBLIC_OPTIONS
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", text).group(1)) == 11
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    assert re.search(r'"guidance_t_min"\s+\[0\]', doc) and re.search(r'"guidance_t_max"\s+\[-1\]', doc)
    for word in ("DR_SAMPLER_CFDG_DDPM_X0", "_INPAINTING_DDPM_X0", "_CFDG_DDIM_X0", "lo <= t <= hi", "captured chain's key"):
        assert word in doc, word
    # the library's own code knows exactly these two names (and the set-time messages name the range)
    abi = open(os.path.join(ROOT, "diffroll_amd", "csrc", "abi.hip")).read()
    assert set(re.findall(r'n == "(guidance\w*)"', abi)) == {"guidance_t_min", "guidance_t_max"}


def test_no_gpu_engine_still_fails_loudly_and_unknown_names_are_names():
    """Without a GPU there is no engine to set an option on (dr_create fails, tests/test_cabi_cpu.py); a null handle is
    DR_EINVAL for the new names as for the old ones - never a crash."""
    from diffroll_amd import _cabi
    try:
        lib = _cabi.load_library()
    except RuntimeError:
        pytest.skip("library not built")
    for name in (b"guidance_t_min", b"guidance_t_max", b"guidance_t_mid"):
        assert lib.dr_set_option(None, name, 0) == _cabi.DR_EINVAL


def test_option_value_rules(driver):
    S = 12
    cases = [(0, v, v >= 0 and v < S) for v in (-2, -1, 0, 1, 11, 12, 13)]
    cases += [(1, v, v >= -1 and v < S) for v in (-2, -1, 0, 1, 11, 12, 13)]
    got = ask(driver, [f"opt {m} {v} {S}" for m, v, _ in cases])
    assert [g[0] for g in got] == [int(ok) for _, _, ok in cases]
    # lo > hi is found at the call, from the effective pair (hi = -1 is S - 1)
    got = ask(driver, [f"empty 0 -1 {S}", f"empty 11 -1 {S}", f"empty 4 8 {S}", f"empty 8 8 {S}", f"empty 9 8 {S}", f"empty 1 0 {S}"])
    assert got == [(0, 11), (0, 11), (0, 8), (0, 8), (1, 8), (1, 0)]


# ---------------------------------------------------------------------------------------------- 2. planner
S12, B = 12, 2


def shapes(driver, steps, lo, hi, w_zero=False, NB=2 * B, n_cond=B):
    nxt = steps[1:] + [-1]
    return ask(driver, [f"step {NB} {n_cond} {B} {lo} {hi} {S12} {int(w_zero)} {t} {n}" for t, n in zip(steps, nxt)])


def expected(steps, lo, hi):
    """The definition: guided iff lo <= t <= hi -> 2B evaluations, B conditional, dual; else B conditional ones."""
    ev = lambda t: (0, 0, 0) if t < 0 else ((2 * B, B, 1) if lo <= t <= hi else (B, B, 0))
    return [ev(t) + ev(n) for t, n in zip(steps, steps[1:] + [-1])]


@pytest.mark.parametrize("n", [0, 6])
def test_planner_sequence_over_an_interval(driver, n):
    steps = CR.visited(S12, n)
    if n == 6:
        assert steps == [11, 9, 7, 4, 2, 0]
    got = shapes(driver, steps, 4, 8)
    assert got == expected(steps, 4, 8)
    # spelled out for the full order: (NB, dual now, dual next)
    if n == 0:
        assert [(g[0], g[2], g[5]) for g in got] == (
            [(2, 0, 0)] * 2 + [(2, 0, 1)] + [(4, 1, 1)] * 4 + [(4, 1, 0)] + [(2, 0, 0)] * 3 + [(2, 0, 0)])
    else:
        assert [(g[0], g[2], g[5]) for g in got] == [(2, 0, 0), (2, 0, 1), (4, 1, 1), (4, 1, 0), (2, 0, 0), (2, 0, 0)]


@pytest.mark.parametrize("n", [0, 6])
def test_defaults_reproduce_todays_plan(driver, n):
    """Defaults: every step of a guiding sampler is the 2B dual step (w != 0) or the B conditional step (w == 0) - the
    rule run_step had; [0, S - 1] is the defaults field for field; the samplers that do not guide keep their shape."""
    steps = CR.visited(S12, n)
    nxt = lambda row: [row if t >= 0 else (0, 0, 0) for t in steps[1:] + [-1]]
    dflt = shapes(driver, steps, 0, -1)
    assert dflt == [(2 * B, B, 1) + m for m in nxt((2 * B, B, 1))]
    assert shapes(driver, steps, 0, S12 - 1) == dflt
    zero = shapes(driver, steps, 0, -1, w_zero=True)
    assert zero == [(B, B, 0) + m for m in nxt((B, B, 0))]
    assert shapes(driver, steps, 4, 8, w_zero=True) == zero              # w == 0 stays what it is under any interval
    for NB, n_cond in ((B, B), (B, 0)):                                  # ddpm_x0 ..., generation_ddpm_x0
        got = shapes(driver, steps, 4, 8, NB=NB, n_cond=n_cond)
        assert got == [(NB, n_cond, 0) + m for m in nxt((NB, n_cond, 0))]


# ---------------------------------------------------------------------------------------------- 3. restatement
def _reduced():
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=64, residual_layers=2, kernel_size=3, timesteps=S12)
    p = R.synthetic_params(hp, seed=5)
    g = torch.Generator().manual_seed(6)
    Tn = 24
    wav = 0.1 * torch.randn(B, Tn * 512, generator=g)
    x = torch.randn(B, 1, Tn, 88, generator=g)
    noise = torch.randn(S12, B, 1, Tn, 88, generator=g)
    return hp, p, x, R.frontend(wav, hp, Tn), noise


@pytest.mark.parametrize("sampler", ["cfdg_ddpm_x0", "cfdg_ddim_x0"])
def test_restatement_whole_chain_and_zero_weight(sampler):
    hp, p, x, spec, noise = _reduced()
    for n in (0, 6):
        full = CR.sample_chain(p, hp, sampler, x, spec, noise, n, w=0.5)
        assert torch.equal(CR.sample_chain(p, hp, sampler, x, spec, noise, n, w=0.5, interval=(0, S12 - 1)), full)
        plain = CR.sample_chain(p, hp, sampler, x, spec, noise, n, w=0.0)
        assert torch.equal(CR.sample_chain(p, hp, sampler, x, spec, noise, n, w=0.0, interval=(4, 8)), plain)
        # ... which is the chain of the conditional evaluation alone
        alone = CR.sample_chain(p, hp, "ddpm_x0" if sampler == "cfdg_ddpm_x0" else "ddim_x0", x, spec, noise, n)
        assert torch.equal(plain, alone)
        mixed = CR.sample_chain(p, hp, sampler, x, spec, noise, n, w=0.5, interval=(4, 8))
        assert not torch.equal(mixed, full) and not torch.equal(mixed, plain)


# ---------------------------------------------------------------------------------------------- 4. Python surface
def _model(**kw):
    from diffroll_amd import ClassifierFreeDiffRoll
    base = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=229, norm_args=[0, 1, "imagewise"],
                residual_layers=2, kernel_size=3, dilation_base=2, dilation_bound=4,
                spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000,
                               center=True, normalized=True, pad_mode="reflect"),
                timesteps=200)
    base.update(kw)
    return ClassifierFreeDiffRoll(**base)


def test_check_guidance_interval():
    from diffroll_amd.schedule import GUIDING_SAMPLERS, check_guidance_interval
    assert set(GUIDING_SAMPLERS) == {"cfdg_ddpm_x0", "inpainting_ddpm_x0", "cfdg_ddim_x0"}
    assert check_guidance_interval(None, 200) == (0, -1)
    assert check_guidance_interval(None, 200, "ddim") == (0, -1)
    assert check_guidance_interval([60, 140], 200, "cfdg_ddpm_x0") == (60, 140)
    assert check_guidance_interval((0, 199), 200) == (0, 199) and check_guidance_interval([7, 7], 200) == (7, 7)
    for bad in ([140, 60], [0, 200], [-1, 5], [0], [0, 1, 2], 5, "0,5", [0.0, 5], [True, 5], [0, None]):
        with pytest.raises(ValueError):
            check_guidance_interval(bad, 200, "cfdg_ddpm_x0")
    for sampler in ("ddpm_x0", "generation_ddpm_x0", "ddim_x0", "ddpm", "ddim", "ddim2ddpm"):
        with pytest.raises(ValueError, match="guides"):
            check_guidance_interval([60, 140], 200, sampler)


def test_facade_hparams_guidance_interval():
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5})
    assert m.guidance_interval() == (0, -1)
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "guidance_interval": None})
    assert m.guidance_interval() == (0, -1)
    m = _model(sampling={"type": "inpainting_ddpm_x0", "w": 0.5, "guidance_interval": [60, 140]})
    assert m.guidance_interval() == (60, 140)
    m.hparams.sampling.guidance_interval = [0, 20]                # read at every use
    assert m.guidance_interval() == (0, 20)
    m.hparams.sampling.guidance_interval = [20, 0]                # ... and refused there, before the engine is reached
    with pytest.raises(ValueError):
        m.engine
    with pytest.raises(ValueError):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    for bad in ([140, 60], [0, 200], [1], "all"):
        with pytest.raises(ValueError):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "guidance_interval": bad})
    with pytest.raises(ValueError, match="guides"):
        _model(sampling={"type": "ddim", "guidance_interval": [60, 140]})


def test_cli_guidance_interval():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "task.sampling.guidance_interval=[60,140]"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 0.5, "guidance_interval": [60, 140]}
    cfg = cli.build_config(["task=inpainting", "task.sampling.guidance_interval=[0,199]", "task.sampling.steps=50"])
    assert cfg["task"]["sampling"]["guidance_interval"] == [0, 199] and cfg["task"]["sampling"]["steps"] == 50
    assert cli.build_config(["task=transcription", "task.sampling.guidance_interval=null"])["task"]["sampling"]["guidance_interval"] is None
    assert "guidance_interval" not in cli.build_config(["task=transcription"])["task"]["sampling"]
    for bad in ("[140,60]", "[0,200]", "60", "[60]", "[1.5,3]", "sixty"):
        with pytest.raises(SystemExit):
            cli.build_config(["task=transcription", f"task.sampling.guidance_interval={bad}"])
    with pytest.raises(SystemExit):                                # generation does not guide
        cli.build_config(["task=generation", "task.sampling.guidance_interval=[60,140]"])
