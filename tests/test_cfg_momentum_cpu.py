"""Option "cfg_momentum" without a GPU: the restated recurrence (tests/momentum_ref.py) against the explicit sum, the restated
chains the GPU tests compare with (tests/momentum_cases.py) shown to carry momentum, momentum_step of csrc/chain_tables.h
through a compiled stand-alone harness, the Python surface - validator, facade, checkpoint override, CLI - the documents, the
built library and the structural facts of the new kernels' text."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from testlib import ATOL, S

import chain_ref as CR
import momentum_cases as MC
import momentum_ref as MR
import project_ref as PR
import thresh_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. the recurrence
@pytest.mark.parametrize("beta", [-5000, 5000, -7500, 9999])
def test_recurrence_is_the_explicit_sum(beta):
    """m_t = sum_j beta^j d_{t-j} in float64, to fp32 rounding: t + 1 terms of magnitude <= |d|max / (1 - |beta|), each step
    two roundings of relative size 2^-24."""
    g = torch.Generator().manual_seed(abs(beta))
    c = [torch.randn(2, 5, 88, generator=g) for _ in range(12)]
    y = [ci + 0.3 * torch.randn(2, 5, 88, generator=g) for ci in c]
    m, ds = None, []
    for t in range(12):
        m, yb = MR.recurrence(y[t], c[t], m, beta)
        ds.append(y[t] - c[t])
        want = MR.explicit_sum(ds, beta)
        bound = 2.0 ** -23 * (t + 1) * float(torch.stack(ds).abs().max()) / (1.0 - abs(beta) / 10000.0)
        assert float((m.double() - want).abs().max()) <= bound, (t, beta)
        assert torch.equal(yb, c[t] + m)
        if t == 0:
            assert torch.equal(m, ds[0])              # the step that starts the state reads nothing
    assert float(MR.factor(-5000)) == -0.5 and MR.factor(3333).dtype == torch.float32


def test_group_ab_without_state_is_project_refs():
    g = torch.Generator().manual_seed(3)
    c, u = torch.randn(2, 7, 88, generator=g) + 0.5, torch.randn(2, 7, 88, generator=g)
    groups = TR.clip_groups(2)
    ab, m = MR.group_ab(c, u, 3.0, None, -5000, 10000, 500, groups)
    y = PR.blended(c, u, 3.0, groups, None)[1]
    assert torch.equal(m, y - c)
    # yb = c + (y - c) is y up to one rounding: the pairs agree closely, and exactly where yb == y
    ref = PR.group_ab(c, u, 3.0, 10000, 500, groups)
    assert np.allclose(ab, ref, rtol=1e-5, atol=1e-6)
    ab2, m2 = MR.group_ab(c, u, 3.0, m, -5000, 10000, 500, groups)
    assert torch.equal(m2, (y - c) + MR.factor(-5000) * m) and not np.array_equal(ab2, ab)
    # a non-finite state stays non-finite, and its group gets the identity pair
    bad = m.clone()
    bad[1, 3, 5] = float("inf")
    ab3, m3 = MR.group_ab(c, u, 3.0, bad, -5000, 10000, 500, groups)
    assert not torch.isfinite(m3[1, 3, 5]) and tuple(ab3[1]) == (0.0, 1.0) and tuple(ab3[0]) == tuple(ab2[0])
    _, m4 = MR.group_ab(c, u, 3.0, m3, -5000, 10000, 500, groups)
    assert not torch.isfinite(m4[1, 3, 5]) and torch.isfinite(m4[0]).all()


# ---------------------------------------------------------------------------------------------- 2. the chains the GPU tests use
def test_restated_chain_carries_momentum():
    """B = 2, T = 40, 20 steps, w = 3 (rescale_cases): beta = -0.5 moves the roll by at least 100 ATOL, m differs from d at every
    guided step after the first, and the rms ratio |m| / |d| per step is printed (README)."""
    roll = MC.assert_active("cfdg_ddpm_x0", *MC.MAIN)
    _, seen, rms = MC.reference("cfdg_ddpm_x0", *MC.MAIN)
    off, seen_off, rms_off = MC.reference("cfdg_ddpm_x0", 0, *MC.MAIN[1:])
    assert not rms_off and list(seen_off) == list(seen) == list(rms) and len(seen) == MC.N_STEPS
    assert float((roll - off).abs().max()) >= 100 * ATOL
    steps = list(rms)
    print("\nstep: rms |m| / rms |d| under beta = -0.5 (cfdg_ddpm_x0, w = 3, cfg_project 1.0, cfg_norm 0.05)")
    for t in steps:
        m, d = rms[t]
        print(f"  t {t:3d}: {m / d:.3f}")
    assert rms[steps[0]][0] == rms[steps[0]][1]                   # the first guided step: m is d
    assert all(rms[t][0] != rms[t][1] for t in steps[1:])


def test_momentum_0_is_project_refs_chain():
    hp, p, _, x, noise = MC.setup()
    off, seen, rms = MC.reference("cfdg_ddpm_x0", 0, 10000, 500)
    ref, seen_ref = MC.PC.reference("cfdg_ddpm_x0", 10000, 500)
    assert torch.equal(off, ref) and not rms and seen == seen_ref


@pytest.mark.parametrize("values", MC.VALUES, ids=[str(v[0]) for v in MC.VALUES])
@pytest.mark.parametrize("sampler", MC.GUIDING)
def test_gpu_chain_cases_are_active(sampler, values):
    MC.assert_active(sampler, *values)


@pytest.mark.parametrize("values", MC.VALUES, ids=[str(v[0]) for v in MC.VALUES])
@pytest.mark.parametrize("name,kw,_", MC.OPTION_CASES, ids=[c[0] for c in MC.OPTION_CASES])
def test_gpu_option_cases_are_active(name, kw, _, values):
    MC.assert_active("cfdg_ddpm_x0", *values, **kw)
    if "interval" in kw:                              # the state starts at the first step inside the interval
        _, seen, rms = MC.reference("cfdg_ddpm_x0", *values, **kw)
        first = max(rms)
        assert all(kw["interval"][0] <= t <= kw["interval"][1] for t in rms) and rms[first][0] == rms[first][1]


# ---------------------------------------------------------------------------------------------- 3. momentum_step
DRIVER = r"""
    #include <cstdio>
    #include <iostream>
    #include <sstream>
    #include <string>
    #include "chain_tables.h"
    int main() {
        dr::ChainSteps steps;
        std::string line, cmd;
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            in >> cmd;
            if (cmd == "steps") {
                int S = 0, n = 0;
                in >> S >> n;
                steps = dr::ChainSteps(S, n);
            } else if (cmd == "mom") {      // mom VALID SAMPLER B T t | SAMPLER B T t START_STEP LO HI W_ZERO
                dr::MomentumKey k;
                dr::GuidanceInterval g;
                int valid = 0, sampler = 0, B = 0, T = 0, t = 0, start = 0, wz = 0;
                in >> valid >> k.sampler >> k.B >> k.T >> k.t >> sampler >> B >> T >> t >> start >> g.lo >> g.hi >> wz;
                k.valid = valid != 0;
                const dr::MomentumVerdict v = dr::momentum_step(k, sampler, B, T, t, steps, start, g, steps.S(), wz != 0);
                const int out[2] = {(int)v.what, v.expect};
                fwrite(out, 4, 2, stdout);
            } else return 1;
        }
        return 0;
    }
"""
STARTS, CONTINUES, REFUSED = 0, 1, 2      # dr::MomentumStep


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("momentum_step")
    src = d / "momentum_step_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "momentum_step_driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def ask(driver, lines):
    r = subprocess.run([driver], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return [struct.unpack_from("<ii", r.stdout, 8 * i) for i in range(len(r.stdout) // 8)]


def test_momentum_rule_of_dr_step(driver):
    steps = CR.visited(200, 20)
    assert steps[:4] == [199, 189, 178, 168] and [t for t in steps if 60 <= t <= 140] == [136, 126, 115, 105, 94, 84, 73, 63]
    key, call, none = "1 1 2 40", "1 2 40", "0 -1 0 0 -1"
    whole, inter = "0 -1 0", "60 140 0"
    cases = [
        # a respaced chain, every step guides
        (f"{none} {call} 199 -1 {whole}", (STARTS, 199)),
        (f"{key} 178 {call} 199 -1 {whole}", (STARTS, 199)),            # the first guided step starts, whatever is held
        (f"{key} 199 {call} 189 -1 {whole}", (CONTINUES, 189)),
        (f"{key} 10 {call} 0 -1 {whole}", (CONTINUES, 0)),
        (f"{key} 199 {call} 178 -1 {whole}", (REFUSED, 189)),           # a step skipped,
        (f"{key} 189 {call} 189 -1 {whole}", (REFUSED, 178)),           # repeated
        (f"{none} {call} 189 -1 {whole}", (REFUSED, 199)),              # nothing held
        (f"{key} 199 2 2 40 189 -1 {whole}", (REFUSED, 199)),           # another sampler,
        (f"{key} 199 1 3 40 189 -1 {whole}", (REFUSED, 199)),           # batch
        (f"{key} 199 1 2 41 189 -1 {whole}", (REFUSED, 199)),           # or frame count
        (f"{key} 0 {call} 10 -1 {whole}", (REFUSED, 199)),              # behind step 0 nothing follows
        # under the interval [60, 140]: the first visited step inside it starts; the steps above and below are never asked about
        (f"{none} {call} 136 -1 {inter}", (STARTS, 136)),
        (f"{key} 136 {call} 126 -1 {inter}", (CONTINUES, 126)),
        (f"{key} 73 {call} 63 -1 {inter}", (CONTINUES, 63)),
        (f"{key} 136 {call} 115 -1 {inter}", (REFUSED, 126)),
        (f"{key} 63 {call} 52 -1 {inter}", (REFUSED, 136)),             # (a caller's error: 52 does not guide)
        (f"{none} {call} 126 -1 {inter}", (REFUSED, 136)),
        # from a start step
        (f"{none} {call} 168 168 {whole}", (STARTS, 168)),
        (f"{key} 199 {call} 168 168 {whole}", (STARTS, 168)),
        (f"{key} 168 {call} 157 168 {whole}", (CONTINUES, 157)),
        (f"{none} {call} 199 168 {whole}", (REFUSED, 168)),             # above the start: not this chain's
        (f"{none} {call} 136 168 {inter}", (STARTS, 136)),              # a start above the interval: its first step inside
        (f"{none} {call} 105 105 {inter}", (STARTS, 105)),              # a start inside it
        (f"{key} 105 {call} 94 105 {inter}", (CONTINUES, 94)),
        (f"{none} {call} 136 105 {inter}", (REFUSED, 105)),
    ]
    got = ask(driver, ["steps 200 20"] + [f"mom {c}" for c, _ in cases])
    assert len(got) == len(cases)
    for (c, want), g in zip(cases, got):
        assert g == want, (c, g)
    # every step of a full chain with a gap: under [10, 30] step t continues exactly the state of t + 1, 30 starts
    pairs = [(k, t) for k in range(10, 31) for t in range(10, 31)]
    full = ask(driver, ["steps 50 0"] + [f"mom {key} {k} {call} {t} -1 10 30 0" for k, t in pairs])
    for (k, t), g in zip(pairs, full):
        want = (STARTS, 30) if t == 30 else (CONTINUES, t) if t == k - 1 else (REFUSED, k - 1 if k > 10 else 30)
        assert g == want, (k, t, g)


# ---------------------------------------------------------------------------------------------- 4. the Python surface
def test_check_cfg_momentum():
    from diffroll_amd.schedule import GUIDING_SAMPLERS, check_cfg_momentum
    for off in (None, 0, False, 0.0):
        assert check_cfg_momentum(off) == 0 and check_cfg_momentum(off, "ddim") == 0 and check_cfg_momentum(off, "cfdg_ddpm_x0", None, None) == 0
    for s in GUIDING_SAMPLERS:
        assert check_cfg_momentum(-0.5, s, 1.0, None) == -5000 and check_cfg_momentum(-0.75, s, None, 0.05) == -7500
        assert check_cfg_momentum(0.5, s, 1.0, 0.05) == 5000 and check_cfg_momentum(-0.9999, s, 1.0) == -9999
        assert check_cfg_momentum(0.0001, s, 1.0) == 1
    for bad in (1.0, -1.0, 1, -1, 1.5, -2, -5000, "-0.5", [-0.5], True, 0.00001, -0.99999):
        with pytest.raises(ValueError, match=re.escape("cfg_momentum must be") + ".*" + re.escape(repr(bad))):
            check_cfg_momentum(bad, "cfdg_ddpm_x0", 1.0, 0.05)
    for s in ("ddpm_x0", "generation_ddpm_x0", "ddim_x0", "ddpm", "ddim", "ddim2ddpm"):
        with pytest.raises(ValueError, match=r"cfg_momentum = -0.5 needs a sampler that guides"):
            check_cfg_momentum(-0.5, s, 1.0, 0.05)
    for partners in ((None, None), (0, 0.0), (False, None), ()):
        with pytest.raises(ValueError, match=r"cfg_momentum = -0.5 needs cfg_project or cfg_norm"):
            check_cfg_momentum(-0.5, "cfdg_ddpm_x0", *partners)


def _model(**kw):
    from diffroll_amd import ClassifierFreeDiffRoll
    base = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=229, norm_args=[0, 1, "imagewise"],
                residual_layers=2, kernel_size=3, dilation_base=2, dilation_bound=4,
                spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000,
                               center=True, normalized=True, pad_mode="reflect"),
                timesteps=S)
    base.update(kw)
    return ClassifierFreeDiffRoll(**base)


def test_facade_hparams():
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0})
    assert m.cfg_momentum() == 0
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_project": 1.0, "cfg_norm": 0.05, "cfg_momentum": -0.5})
    assert m.cfg_momentum() == -5000 and m.sampling_options()["cfg_momentum"] == -5000
    m.hparams.sampling.cfg_momentum = None            # read at every use
    assert m.cfg_momentum() == 0 and m.cfg_project() == 10000
    m.hparams.sampling.cfg_momentum = -0.75
    m.__dict__["_stride1"] = True                     # one of the reference's single-step methods is running
    assert m.cfg_momentum() == 0 and m.cfg_project() == 0
    m.__dict__["_stride1"] = False
    assert m.cfg_momentum() == -7500
    m.hparams.sampling.cfg_momentum = -1.5            # refused at use, before the engine is reached
    with pytest.raises(ValueError, match="cfg_momentum must be"):
        m.engine
    with pytest.raises(ValueError, match="cfg_momentum must be"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    m.hparams.sampling.cfg_momentum = -0.5
    m.hparams.sampling.cfg_project = None
    assert m.cfg_momentum() == -5000                  # (the bound alone is a partner)
    m.hparams.sampling.cfg_norm = None
    with pytest.raises(ValueError, match="cfg_momentum = -0.5 needs cfg_project or cfg_norm"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    m.hparams.sampling.cfg_project = 1.0
    m.hparams.sampling.cfg_rescale = 0.7              # the partners' refusals cover it, with no new text
    with pytest.raises(ValueError, match="cfg_project = 1.0 does not combine with cfg_rescale = 0.7"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    m.hparams.sampling.cfg_rescale = None
    m.hparams.sampling.x0_clip = 1
    assert m.cfg_momentum() == -5000                  # (the clamp combines)
    m.hparams.sampling.x0_threshold = 0.995
    with pytest.raises(ValueError, match="cfg_project = 1.0 does not combine with x0_threshold = 0.995"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    for bad in (1.0, "-0.5", -5000):
        with pytest.raises(ValueError, match="cfg_momentum must be"):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "cfg_project": 1.0, "cfg_momentum": bad})
    with pytest.raises(ValueError, match="needs a sampler that guides"):
        _model(sampling={"type": "ddpm_x0", "cfg_momentum": -0.5})
    with pytest.raises(ValueError, match="needs cfg_project or cfg_norm"):
        _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_momentum": -0.5})
    assert "cfg_momentum" in type(m).sample.__doc__


def test_load_from_checkpoint_override(golden_dir):
    from diffroll_amd import ClassifierFreeDiffRoll
    path = os.path.join(golden_dir, "trained_small.ckpt")
    got = ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_project": 1.0, "cfg_momentum": -0.5})
    assert got.cfg_momentum() == -5000 and got.cfg_project() == 10000
    assert ClassifierFreeDiffRoll.load_from_checkpoint(path).cfg_momentum() == 0
    with pytest.raises(ValueError, match="cfg_momentum must be"):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_project": 1.0, "cfg_momentum": -1})
    with pytest.raises(ValueError, match="needs cfg_project or cfg_norm"):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_momentum": -0.5})


def test_cli():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "task.sampling.w=3", "task.sampling.cfg_project=1.0", "task.sampling.cfg_norm=0.05",
                            "task.sampling.cfg_momentum=-0.5"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 3, "cfg_project": 1.0, "cfg_norm": 0.05, "cfg_momentum": -0.5}
    assert "cfg_momentum" not in cli.build_config(["task=transcription"])["task"]["sampling"]
    assert cli.build_config(["task=transcription", "task.sampling.cfg_momentum=null"])["task"]["sampling"]["cfg_momentum"] is None
    for bad in ("1.0", "-1", "-5000", "high", "1.5"):
        with pytest.raises(SystemExit, match="task.sampling.cfg_momentum"):
            cli.build_config(["task=transcription", "task.sampling.cfg_project=1.0", f"task.sampling.cfg_momentum={bad}"])
    with pytest.raises(SystemExit, match="task.sampling.cfg_momentum.*needs a sampler that guides"):
        cli.build_config(["task=transcription", "task.sampling.type=ddim", "task.sampling.cfg_momentum=-0.5"])
    with pytest.raises(SystemExit, match="task.sampling.cfg_momentum.*needs cfg_project or cfg_norm"):
        cli.build_config(["task=transcription", "task.sampling.cfg_momentum=-0.5"])
    with pytest.raises(SystemExit, match="task.sampling.cfg_norm.*does not combine with cfg_rescale"):
        cli.build_config(["task=transcription", "task.sampling.cfg_norm=0.05", "task.sampling.cfg_momentum=-0.5", "task.sampling.cfg_rescale=0.7"])
    with pytest.raises(SystemExit, match="task.sampling.cfg_project.*does not combine with x0_threshold"):
        cli.build_config(["task=transcription", "task.sampling.cfg_project=1.0", "task.sampling.cfg_momentum=-0.5", "task.sampling.x0_clip=1",
                          "task.sampling.x0_threshold=0.995"])


# ---------------------------------------------------------------------------------------------- 5. the documents
def test_option_is_public_and_documented():
    from diffroll_amd import _cabi
    from diffroll_amd.engine import _MIRRORED, Engine
    name = "cfg_momentum"
    assert name in _cabi.PUBLIC_OPTIONS and _MIRRORED[name] == 0 and getattr(Engine, name) == 0
    assert f"'{name}'" in Engine.set_option.__doc__ and f"'{name}'" in Engine.holding.__doc__
    assert "dr_debug_momentum" in _cabi.DEBUG_EXPORTS and callable(Engine.momentum_stats)
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    begin = re.search(r'"cfg_momentum"\s+\[0\]', doc)
    assert begin
    flat = re.sub(r"\s*\n \*\s*", " ", doc[begin.start():doc.index("Unknown names")])
    for word in ("-9999 .. 9999", "Sadat et al", "bf = (float)((double)cfg_momentum / 10000.0)", "d  = y - c", "m  = d + (bf * m_prev)",
                 "STARTS the state (nothing is read)", "yb = c + m", "d_i = (double)yb_i - (double)c_i", "y' = (a c) + (b yb)",
                 "y' = yb where a == 0.0f and b == 1.0f", "no contraction", "each operation rounded once",
                 "A non-finite m stays non-finite", "a = 0.0f, b = 1.0f", "updated in place", '"start_step"',
                 '"guidance_t_min" / "guidance_t_max"', "neither read nor write the state", "continues from the last guided one",
                 "no memset, no host help, every replay restarts by itself", "csrc/momentum.hip", "DR_MODE_FUSED_STACK", "DR_ESTATE",
                 "naming the step expected next", "dr_sample", "every option change that ends a solver history",
                 'a change of "cfg_momentum" itself', "naming the three options", "stating the range", "captured chain's key",
                 "each rank holds the state of its rows", "Nothing is known about quality", "INTEGRATION.md 3c"):
        assert word in flat, word
    partners = re.sub(r"\s*\n \*\s*", " ", doc[re.search(r'"cfg_project"\s+\[0\]', doc).start():begin.start()])
    assert 'without its momentum, which is option "cfg_momentum" below' in partners
    assert "dr_debug_momentum(" in open(os.path.join(ROOT, "include", "diffroll_amd_debug.h")).read()
    for doc_name, words in (("README.md", ("cfg_momentum", "profiles/momentum_kernel_resources.txt", "profiles/momentum_sweep.txt",
                                           "Nothing is known about quality")),
                            ("INTEGRATION.md", ('"cfg_momentum"', "task.sampling.cfg_momentum=-0.5"))):
        body = open(os.path.join(ROOT, doc_name)).read()
        for word in words:
            assert word in body, (doc_name, word)
    abi = open(os.path.join(ROOT, "diffroll_amd", "csrc", "abi.hip")).read()
    assert '{"cfg_momentum", &ChainOptions::cfg_momentum,' in abi and "momentum_step(" in abi      # (its row of the option table)


def test_the_built_library_knows_the_option():
    """Without a GPU no engine exists to set the option on.  What can be held: the library exports dr_debug_momentum, carries
    the option's own refusal texts (a library without it has none), and a null handle is DR_EINVAL, never a crash."""
    from diffroll_amd import _cabi
    if not os.path.exists(_cabi.LIB_PATH):
        pytest.skip("the library is not built (python -m diffroll_amd.build)")
    lib = _cabi.load_library()                        # (built: a load failure is a failure, not a skip)
    assert hasattr(lib, "dr_debug_momentum")
    blob = open(_cabi.LIB_PATH, "rb").read()
    for text in (b"cfg_momentum is 0 (off) or beta in units of 1 / 10000, -9999 .. 9999", b"cfg_project = %d and cfg_norm = %d are both off",
                 b"continues no momentum state - the step expected next is %d", b"dr_debug_momentum: cfg_momentum is 0 (off)"):
        assert text in blob, text
    assert lib.dr_set_option(None, b"cfg_momentum", -5000) == _cabi.DR_EINVAL
    assert lib.dr_debug_momentum(None, None, None, None, None, 1, 1, 0.0, None, None) == _cabi.DR_EINVAL


def test_the_new_kernels_text_and_the_parents():
    """The momentum form is a further instantiation of update_quad and a second argument: UpdateArgs does not grow, tail.hip
    learns nothing, the new quad function's clamp call lives in momentum_quad.h; contraction is off throughout the new files,
    which use no floating-point atomic and wait for nobody."""
    csrc = os.path.join(ROOT, "diffroll_amd", "csrc")
    tail = open(os.path.join(csrc, "tail.hip")).read().lower()
    assert "momentum" not in tail and "cfg_" not in tail
    kern = open(os.path.join(csrc, "kernels.h")).read()
    upd = kern[kern.index("struct UpdateArgs {"):kern.index("// (mode 5) the half the step reads")]
    assert "momentum" not in upd.lower() and upd.rstrip().endswith("float clamp_lo, clamp_hi;\n};".rstrip())
    assert "struct MomentumUpd {" in kern and "struct MomentumArgs {" in kern
    quad = open(os.path.join(csrc, "momentum_quad.h")).read()
    hip = open(os.path.join(csrc, "momentum.hip")).read()
    assert quad.count("clamp_quad(") == 1 and "clamp_quad" not in hip and "clamp_quad" not in open(os.path.join(csrc, "update.hip")).read()
    # the parent's pieces, reused: its frame sums and its record writer (project_coef inside) from project_quad.h, the groups'
    # places in the skeleton the three statistics share and in the update's form
    skel = open(os.path.join(csrc, "group_sums.h")).read()
    pquad = open(os.path.join(csrc, "project_quad.h")).read()
    record = pquad[pquad.index("DR_DEVINL void project_record("):]
    assert "project_frame(" in hip and "project_record(" in hip and "project_coef(" in record[:record.index("\n}\n")]
    assert "thresh_place(" in skel and "thresh_place(" in quad and '#include "group_sums.h"' in hip
    pragma = "#pragma clang fp contract(off)"
    assert hip.index(pragma) < hip.index("DR_DEVINL") and quad.count(pragma) == quad.count("DR_DEVINL void") == 3
    assert skel.index(pragma) < skel.index("DR_DEVINL") and skel.count(pragma) == skel.count("DR_DEVINL") + 1
    code = "\n".join(line.split("//")[0] for line in (hip + quad + skel).splitlines())
    for banned in ("unsafeAtomicAdd", "atomicAdd(", "atomicMax(", "atomicMin(", "while (", "__builtin_amdgcn_s_sleep"):
        assert banned not in code, banned
    for kernel in ("momentum_roll_kernel", "momentum_grid_kernel", "update_momentum_kernel"):
        assert kernel in code, kernel
    # the momentum kernel hands its MomentumUpd to update_quad, whose form it selects
    assert re.search(r"void update_momentum_kernel\(const UpdateArgs a, const MomentumUpd mo\) \{[^}]*update_quad\(a, i4, &y, mo\)", code)
    assert "DR_DEVINL void form_quad(const UpdateArgs& a, const MomentumUpd& mo," in quad
    from diffroll_amd import build
    assert "momentum.hip" in build.SOURCES and any(h.endswith("momentum_quad.h") for h in build.HEADERS)
