"""Option "cfg_rescale" (include/diffroll_amd.h) without a GPU: the restated factor of tests/rescale_ref.py against torch.std
(the definition), its identities, that the inputs of the GPU tests rescale at all, and the Python surface
(check_cfg_rescale, hparams.sampling.cfg_rescale, the CLI, the documents)."""
import os
import re

import numpy as np
import pytest
import torch

from testlib import ATOL

import clip_cases as CC
import rescale_cases as RC
import rescale_ref as RR
import thresh_cases as TC
import thresh_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = CC.S


# ---------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("T", [1, 40, 640])
def test_restated_factor_is_the_ratio_of_torch_std(T):
    """N = 88, 3 520, 56 320: rho = std(c) / std(y) on the flattened roll (Bessel's correction cancels), g = 1 + phi (rho - 1);
    1e-12 relative in double - the order of the sums and the one-pass variance move far less than that on these inputs."""
    g = torch.Generator().manual_seed(T)
    c, u = 0.3 * torch.randn(2, 1, T, 88, generator=g) + 0.1, 0.4 * torch.randn(2, 1, T, 88, generator=g)
    y = RR.guided(c, u, 3.0)
    for value in (1, 5000, 7000, 10000):
        for b, rows in enumerate(TR.clip_groups(2)):
            N, S1c, S2c = RR.group_sums(c, rows)
            _, S1y, S2y = RR.group_sums(y, rows)
            assert N == T * 88
            with np.errstate(all="ignore"):
                rho = np.sqrt((S2c - S1c * (S1c / N)) / (S2y - S1y * (S1y / N)))
            want = float(torch.std(c[b].double().reshape(-1)) / torch.std(y[b].double().reshape(-1)))
            assert abs(rho - want) <= 1e-12 * want, (T, value, b, rho, want)
            got = RR.group_g(c, u, 3.0, value, TR.clip_groups(2))[b]
            assert got == np.float32(1.0 + value / 10000.0 * (rho - 1.0)) and got.dtype == np.float32


def test_identities():
    g = torch.Generator().manual_seed(4)
    c, u = torch.randn(2, 1, 3, 88, generator=g), torch.randn(2, 1, 3, 88, generator=g)
    groups = TR.clip_groups(2)
    one = np.float32(1.0)
    assert RR.factor(0, 88, 1.0, 2.0, 3.0, 40.0) == one                            # phi = 0
    assert (RR.group_g(c, u, 0.0, 7000, groups) == one).all()                       # w = 0: y is c
    assert (RR.group_g(c, None, 3.0, 7000, groups) == one).all()                    # no u
    flat = torch.full((2, 1, 3, 88), 0.75)
    assert (RR.group_g(flat, flat, 3.0, 7000, groups) == one).all()                 # a constant y (Vy = 0)
    assert (RR.group_g(flat, u, 3.0, 10000, groups) != one).all()                   # ... a constant c alone is not: rho = 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        cb = c.clone()
        cb[1, 0, 2, 5] = bad
        got = RR.group_g(cb, u, 3.0, 7000, groups)
        assert got[1] == one and got[0] != one and got[0] == RR.group_g(c, u, 3.0, 7000, groups)[0], bad
    assert RR.factor(7000, 88, 0.0, -1.0, 0.0, 5.0) == one                          # !(Vc >= 0)
    assert RR.factor(10000, 88, 0.0, 1e300, 0.0, 1e-300) == one                     # g not finite in fp32


def test_window_groups_share_one_factor_and_count_every_frame_once():
    """Three windows of 8 frames sharing 2: g over the canvas equals g of the canvas as one clip where the canvas has a single
    block per row (the order of the sums then only differs by where the rows' blocks end)."""
    g = torch.Generator().manual_seed(6)
    c, u = torch.randn(3, 1, 8, 88, generator=g), torch.randn(3, 1, 8, 88, generator=g)
    groups = TR.window_groups(3, 2)
    for mode in (0, 1, 2):
        got = RR.group_g(c, u, 3.0, 7000, groups, plan=(2, mode))
        assert got.shape == (1,) and abs(float(got[0]) - 1.0) > 0.1
    assert RR.group_g(c, u, 3.0, 7000, TR.window_groups(3, 2, marks=(2,)), plan=(2, 0)).shape == (2,)
    N, _, _ = RR.group_sums(c, groups[0])
    assert N == (8 + 6 + 6) * 88


# ---------------------------------------------------------------------------------------------- 2. the GPU inputs are active
def test_the_issues_figures():
    """clip_cases.setup() with the guided case of thresh_cases (cfdg_ddpm_x0, w = 3), 20 steps, phi = 0.7: |g - 1| >= 0.4 at
    every visited step and roll, and the rescaled roll is more than 100 ATOL from the unrescaled one's."""
    hp, p, _, x, noise, spec = CC.setup()
    sampler, w, _, _ = TC.GUIDED
    roll, gs = RR.sample_chain(p, hp, sampler, x, spec, noise, 20, cfg_rescale=7000, w=w)
    off, none = RR.sample_chain(p, hp, sampler, x, spec, noise, 20, cfg_rescale=0, w=w)
    g = np.concatenate(list(gs.values()))
    print(f"\ng in {g.min():.3f} .. {g.max():.3f}; max |rescaled - unrescaled| {float((roll - off).abs().max()):.3e}")
    assert g.shape == (40,) and (np.abs(g - 1.0) >= 0.4).all() and not none
    assert float((roll - off).abs().max()) > 100 * ATOL
    import chain_ref as CR
    assert torch.equal(off, CR.sample_chain(p, hp, sampler, x, spec, noise, 20, w=w))      # value 0 is chain_ref's chain


@pytest.mark.parametrize("sampler", RC.GUIDING)
def test_gpu_chain_cases_are_active(sampler):
    for value in RC.VALUES:
        RC.assert_active(sampler, value)


@pytest.mark.parametrize("name,kw,_", RC.OPTION_CASES, ids=[c[0] for c in RC.OPTION_CASES])
def test_gpu_option_cases_are_active(name, kw, _):
    roll = RC.assert_active("cfdg_ddpm_x0", 7000, **kw)
    # the option beside the rescale matters on these inputs: its chain is not the plain rescaled one
    assert float((roll - RC.reference("cfdg_ddpm_x0", 7000)[0]).abs().max()) >= 100 * ATOL
    if "interval" in kw:                              # the steps outside the interval do not guide: no g there
        _, gs = RC.reference("cfdg_ddpm_x0", 7000, **kw)
        assert gs and all(kw["interval"][0] <= t <= kw["interval"][1] for t in gs) and len(gs) < RC.N_STEPS


# ---------------------------------------------------------------------------------------------- 3. the Python surface
def test_check_cfg_rescale():
    from diffroll_amd.schedule import GUIDING_SAMPLERS, check_cfg_rescale
    for off in (None, 0, False, 0.0):
        assert check_cfg_rescale(off) == 0 and check_cfg_rescale(off, "ddim") == 0
    for s in GUIDING_SAMPLERS:
        assert check_cfg_rescale(0.7, s) == 7000 and check_cfg_rescale(1, s) == 10000 and check_cfg_rescale(1.0, s) == 10000
        assert check_cfg_rescale(0.0001, s) == 1 and check_cfg_rescale(0.5, s) == 5000
    for bad in (1.0001, -0.1, 2, 7000, "0.7", [0.7], True, 0.00001):
        with pytest.raises(ValueError, match=re.escape("cfg_rescale must be") + ".*" + re.escape(repr(bad))):
            check_cfg_rescale(bad, "cfdg_ddpm_x0")
    for s in ("ddpm_x0", "generation_ddpm_x0", "ddim_x0", "ddpm", "ddim", "ddim2ddpm"):
        with pytest.raises(ValueError, match=r"cfg_rescale = 0.7 needs a sampler that guides"):
            check_cfg_rescale(0.7, s)


def _model(**kw):
    from diffroll_amd import ClassifierFreeDiffRoll
    base = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=229, norm_args=[0, 1, "imagewise"],
                residual_layers=2, kernel_size=3, dilation_base=2, dilation_bound=4,
                spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000,
                               center=True, normalized=True, pad_mode="reflect"),
                timesteps=S)
    base.update(kw)
    return ClassifierFreeDiffRoll(**base)


def test_facade_hparams_cfg_rescale():
    assert _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0}).cfg_rescale() == 0
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_rescale": 0.7})
    assert m.cfg_rescale() == 7000 and m.sampling_options()["cfg_rescale"] == 7000
    m.hparams.sampling.cfg_rescale = None             # read at every use
    assert m.cfg_rescale() == 0
    m.hparams.sampling.cfg_rescale = 0.5
    m.__dict__["_stride1"] = True                     # one of the reference's single-step methods is running
    assert m.cfg_rescale() == 0
    m.__dict__["_stride1"] = False
    assert m.cfg_rescale() == 5000
    m.hparams.sampling.cfg_rescale = 1.5              # refused at use, before the engine is reached
    with pytest.raises(ValueError, match="cfg_rescale must be"):
        m.engine
    with pytest.raises(ValueError, match="cfg_rescale must be"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    for bad in (1.3, 7000, "0.7"):
        with pytest.raises(ValueError, match="cfg_rescale must be"):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "cfg_rescale": bad})
    with pytest.raises(ValueError, match="needs a sampler that guides"):
        _model(sampling={"type": "ddpm_x0", "cfg_rescale": 0.7})


def test_cli_cfg_rescale():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "task.sampling.w=3", "task.sampling.cfg_rescale=0.7"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 3, "cfg_rescale": 0.7}
    assert "cfg_rescale" not in cli.build_config(["task=transcription"])["task"]["sampling"]
    assert cli.build_config(["task=transcription", "task.sampling.cfg_rescale=null"])["task"]["sampling"]["cfg_rescale"] is None
    for bad in ("1.3", "2", "7000", "high", "-0.5"):
        with pytest.raises(SystemExit, match="task.sampling.cfg_rescale"):
            cli.build_config(["task=transcription", f"task.sampling.cfg_rescale={bad}"])
    with pytest.raises(SystemExit, match="task.sampling.cfg_rescale.*needs a sampler that guides"):
        cli.build_config(["task=transcription", "task.sampling.type=ddim", "task.sampling.cfg_rescale=0.7"])


# ---------------------------------------------------------------------------------------------- 4. the documents
def test_option_is_public_and_documented():
    from diffroll_amd import _cabi
    from diffroll_amd.engine import _MIRRORED, Engine
    assert "cfg_rescale" in _cabi.PUBLIC_OPTIONS and "dr_debug_rescale" in _cabi.DEBUG_EXPORTS
    assert _MIRRORED["cfg_rescale"] == 0 and Engine.cfg_rescale == 0
    assert "'cfg_rescale'" in Engine.set_option.__doc__ and "'cfg_rescale'" in Engine.holding.__doc__
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    begin = re.search(r'"cfg_rescale"\s+\[0\]', doc)
    assert begin
    flat = re.sub(r"\s*\n \*\s*", " ", doc[begin.start():doc.index("Unknown names")])
    for word in ("1 .. 10000", "7000", "Lin et al. 2024", "g = 1.0f exactly", "Vc = S2c - S1c (S1c / N)", "rho = sqrt(Vc / Vy)",
                 "in pitch order", "blocks of 64", "in row, then block order", "no floating-point atomic", "frames [O, T)",
                 "DR_MODE_FUSED_STACK", "keeps its tail kernel", "naming the value", '"x0_clip" / "x0_threshold" (neither is required)',
                 "ranks |g y - m|", "all three precisions", "sharding", "captured chain's key", "dr_sample_checked", "INTEGRATION.md 3c"):
        assert word in flat, word
    assert "dr_debug_rescale(" in open(os.path.join(ROOT, "include", "diffroll_amd_debug.h")).read()
    for doc_name, words in (("README.md", ("cfg_rescale", "profiles/rescale_kernel_resources.txt")),
                            ("INTEGRATION.md", ('"cfg_rescale"', "task.sampling.cfg_rescale"))):
        body = open(os.path.join(ROOT, doc_name)).read()
        for word in words:
            assert word in body, (doc_name, word)
    abi = open(os.path.join(ROOT, "diffroll_amd", "csrc", "abi.hip")).read()
    assert '{"cfg_rescale", &ChainOptions::cfg_rescale,' in abi      # (its row of the option table)
    assert set(re.findall(r'n == "(guidance\w*)"', abi)) == {"guidance_t_min", "guidance_t_max"}


def test_the_built_library_knows_the_option():
    """Without a GPU no engine exists to set the option on.  What can be held: the library exports dr_debug_rescale, carries the
    option's own refusal text (a library without the option has neither), and a null handle is DR_EINVAL, never a crash."""
    from diffroll_amd import _cabi
    if not os.path.exists(_cabi.LIB_PATH):
        pytest.skip("the library is not built (python -m diffroll_amd.build)")
    lib = _cabi.load_library()                        # (built: a load failure is a failure, not a skip)
    assert hasattr(lib, "dr_debug_rescale")
    assert b"cfg_rescale is 0 (off) or phi in units of 1 / 10000" in open(_cabi.LIB_PATH, "rb").read()
    assert lib.dr_set_option(None, b"cfg_rescale", 7000) == _cabi.DR_EINVAL
    assert lib.dr_debug_rescale(None, None, None, 1, 1, 0.0, None, None) == _cabi.DR_EINVAL


def test_the_parents_kernels_keep_their_text():
    """The rescaling form is a third instantiation of update_quad and a second argument: UpdateArgs does not grow, tail.hip
    names none of the option's pieces, and the statistics use no floating-point atomic and wait for nobody."""
    csrc = os.path.join(ROOT, "diffroll_amd", "csrc")
    tail = open(os.path.join(csrc, "tail.hip")).read()
    assert "rescale" not in tail.lower()
    kern = open(os.path.join(csrc, "kernels.h")).read()
    upd = kern[kern.index("struct UpdateArgs {"):kern.index("// (mode 5) the half the step reads")]
    assert "rescale" not in upd.lower() and upd.rstrip().endswith("float clamp_lo, clamp_hi;\n};".rstrip())
    # (the loops of the statistics launch live in group_sums.h, which rescale.hip instantiates)
    skel = open(os.path.join(csrc, "group_sums.h")).read()
    hip = open(os.path.join(csrc, "rescale.hip")).read()
    src = hip + open(os.path.join(csrc, "rescale_quad.h")).read() + skel
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    for banned in ("unsafeAtomicAdd", "atomicAdd(", "atomicMax(", "atomicMin(", "while (", "__builtin_amdgcn_s_sleep"):
        assert banned not in code, banned
    assert '#include "group_sums.h"' in hip and "gs_roll<RescaleStat>(a)" in code and "gs_grid<RescaleStat>(a)" in code
    # contraction off in the skeleton: in front of its first function, and in every function
    pragma = "#pragma clang fp contract(off)"
    assert skel.index(pragma) < skel.index("DR_DEVINL") and skel.count(pragma) == skel.count("DR_DEVINL") + 1
    assert code.count("__hip_atomic_fetch_add") == 1      # the ticket, once
    # the rescaled forms of the selection kernels are the text of threshold.hip itself, which test_x0_threshold_cpu.py scans:
    # the unit includes no file of kernel text but itself
    sel = open(os.path.join(csrc, "threshold.hip")).read()
    assert re.findall(r'#include "([^"]+)"', sel) == ["rescale_quad.h", "threshold.hip", "threshold.hip"]
    assert "thresh_roll_rs_kernel" in sel and "thresh_pass_rs_kernel" in sel
    assert not [f for f in os.listdir(csrc) if f.endswith(".inc")]
