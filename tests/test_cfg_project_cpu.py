"""Options "cfg_project" / "cfg_norm" (include/diffroll_amd.h) without a GPU: the properties of the restated coefficients of
tests/project_ref.py in float64 (orthogonality, the bound, the identities and fallbacks), that the inputs of the GPU tests
project at all, and the Python surface (check_cfg_project / check_cfg_norm, hparams.sampling, the CLI, the documents)."""
import os
import re

import numpy as np
import pytest
import torch

from testlib import ATOL

import clip_cases as CC
import project_cases as PC
import project_ref as PR
import thresh_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = CC.S
ZERO, ONE = np.float32(0.0), np.float32(1.0)


def _pair(T, seed=None):
    g = torch.Generator().manual_seed(T if seed is None else seed)
    return 0.3 * torch.randn(2, 1, T, 88, generator=g) + 0.1, 0.4 * torch.randn(2, 1, T, 88, generator=g)


# ---------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("T", [1, 40, 640])
def test_rho_1_leaves_an_update_orthogonal_to_c(T):
    """y' - c = s (d - k c) in float64, before the cast to fp32: |<c, y' - c>| <= 1e-9 |c| |d|."""
    c, u = _pair(T)
    y = PR.guided(c, u, 3.0)
    for norm in (0, 500):
        for b, rows in enumerate(TR.clip_groups(2)):
            N, Scc, Scd, Sdd = PR.group_sums(c, y, rows)
            assert N == T * 88
            k, rho, s, a, bb = PR.parts(10000, norm, 3.0, N, Scc, Scd, Sdd)
            cd, yd = c[b].double().reshape(-1).numpy(), y[b].double().reshape(-1).numpy()
            new = a * cd + bb * yd
            dot = float(np.dot(cd, new - cd))
            assert abs(dot) <= 1e-9 * np.linalg.norm(cd) * np.linalg.norm(yd - cd), (T, norm, b, dot)
            assert abs(float(np.dot(cd, yd - cd)) / float(np.dot(cd, cd)) - k) <= 1e-12 * abs(k)      # k is the share of c in d


@pytest.mark.parametrize("T", [1, 40, 640])
def test_a_binding_r_sets_the_rms_of_the_update(T):
    """rho = 0 and r below the update's rms: the rms of (y' - c) / w equals r to 1e-12 relative, in float64."""
    c, u = _pair(T)
    w = 3.0
    y = PR.guided(c, u, w)
    for b, rows in enumerate(TR.clip_groups(2)):
        sums = PR.group_sums(c, y, rows)
        rms = np.sqrt(sums[3] / sums[0]) / w
        for norm in (500, 1000, int(rms * 10000) - 1):
            r = norm / 10000.0
            assert r < rms
            k, rho, s, a, bb = PR.parts(0, norm, w, *sums)
            cd, yd = c[b].double().reshape(-1).numpy(), y[b].double().reshape(-1).numpy()
            got = np.sqrt(np.mean(((a * cd + bb * yd - cd) / w) ** 2))
            assert abs(got - r) <= 1e-12 * r, (T, norm, got, r)
            assert s < 1.0 and a == 1.0 - s


def test_identities_and_fallbacks():
    c, u = _pair(3, seed=4)
    groups = TR.clip_groups(2)

    def ab(c, u, w, project, norm):
        return PR.group_ab(c, u, w, project, norm, groups)

    y = PR.guided(c, u, 3.0)
    sums = PR.group_sums(c, y, groups[0])
    assert PR.coefficients(0, 100000, 3.0, *sums) == (ZERO, ONE)                  # rho = 0 with a bound that does not bind
    assert PR.coefficients(0, 0, 3.0, *sums) == (ZERO, ONE)
    a, b = PR.coefficients(10000, 100000, 3.0, *sums)
    assert a != ZERO and b == ONE and a.dtype == np.float32 and b.dtype == np.float32
    assert (ab(c, None, 3.0, 10000, 500) == (ZERO, ONE)).all()                   # no u: d = 0
    assert (ab(c, u, 0.0, 10000, 500) == (ZERO, ONE)).all()                      # w = 0: y is c, q = 0 / 0 does not bind
    zero = torch.zeros(2, 1, 3, 88)
    assert (ab(zero, zero, 3.0, 10000, 500) == (ZERO, ONE)).all()                # a zero roll: !(Scc > 0), Sdd = 0
    flat = torch.full((2, 1, 3, 88), 0.75)
    assert (ab(flat, flat, 3.0, 10000, 500) == (ZERO, ONE)).all()                # a constant roll on both sides: d = 0
    got = ab(zero, u, 3.0, 10000, 0)
    assert (got == (ZERO, ONE)).all()                                            # c = 0 alone: k = 0, nothing to remove
    for bad in (float("nan"), float("inf"), float("-inf")):
        cb = c.clone()
        cb[1, 0, 2, 5] = bad
        got = ab(cb, u, 3.0, 10000, 500)
        assert tuple(got[1]) == (ZERO, ONE), bad
        assert tuple(got[0]) == tuple(ab(c, u, 3.0, 10000, 500)[0]) and got[0, 0] != ZERO
        ub = u.clone()
        ub[1, 0, 0, 7] = bad
        assert tuple(ab(c, ub, 3.0, 10000, 500)[1]) == (ZERO, ONE), bad
    assert PR.coefficients(10000, 0, 3.0, 88, 1e-300, 1e300, 1.0) == (ZERO, ONE)  # a not finite in fp32
    # the applied form: the identity pair leaves y bit for bit, any other pair is (a c) + (b y)
    pair = np.array([[0.0, 1.0], [-0.5, 0.75]], dtype=np.float32)
    new = PR.apply(c, y, pair, groups)
    assert torch.equal(new[0], y[0]) and torch.equal(new[1], torch.tensor(-0.5) * c[1] + torch.tensor(0.75) * y[1])


def test_window_groups_share_one_pair_and_count_every_frame_once():
    g = torch.Generator().manual_seed(6)
    c, u = torch.randn(3, 1, 8, 88, generator=g), torch.randn(3, 1, 8, 88, generator=g)
    groups = TR.window_groups(3, 2)
    for mode in (0, 1, 2):
        got = PR.group_ab(c, u, 3.0, 10000, 500, groups, plan=(2, mode))
        assert got.shape == (1, 2) and got[0, 1] < 0.9
    assert PR.group_ab(c, u, 3.0, 10000, 500, TR.window_groups(3, 2, marks=(2,)), plan=(2, 0)).shape == (2, 2)
    cb, yb = PR.blended(c, u, 3.0, groups, (2, 0))
    assert PR.group_sums(cb, yb, groups[0])[0] == (8 + 6 + 6) * 88


# ---------------------------------------------------------------------------------------------- 2. the GPU inputs are active
@pytest.mark.parametrize("sampler", PC.GUIDING)
def test_gpu_chain_cases_are_active(sampler):
    for project, norm in PC.VALUES:
        PC.assert_active(sampler, project, norm)


@pytest.mark.parametrize("name,kw,_", PC.OPTION_CASES, ids=[c[0] for c in PC.OPTION_CASES])
def test_gpu_option_cases_are_active(name, kw, _):
    assert name != "clip-threshold" and "v" not in kw
    roll = PC.assert_active("cfdg_ddpm_x0", *PC.MAIN, **kw)
    # the option beside the projection matters on these inputs: its chain is not the plain projected one
    assert float((roll - PC.reference("cfdg_ddpm_x0", *PC.MAIN)[0]).abs().max()) >= 100 * ATOL
    if "interval" in kw:                              # the steps outside the interval do not guide: no coefficients there
        _, seen = PC.reference("cfdg_ddpm_x0", *PC.MAIN, **kw)
        assert seen and all(kw["interval"][0] <= t <= kw["interval"][1] for t in seen) and len(seen) < PC.N_STEPS


def test_options_off_is_chain_refs_chain():
    import chain_ref as CR
    hp, p, _, x, noise = PC.setup()
    off, seen = PC.reference("cfdg_ddpm_x0", 0, 0)
    assert not seen
    assert torch.equal(off, CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, PC.spec_of("cfdg_ddpm_x0"), noise, PC.N_STEPS, w=PC.W))


# ---------------------------------------------------------------------------------------------- 3. the Python surface
def test_check_cfg_project_and_norm():
    from diffroll_amd.schedule import GUIDING_SAMPLERS, check_cfg_norm, check_cfg_project
    for check in (check_cfg_project, check_cfg_norm):
        for off in (None, 0, False, 0.0):
            assert check(off) == 0 and check(off, "ddim") == 0 and check(off, "ddim", 0.995, 0.7) == 0
    for s in GUIDING_SAMPLERS:
        assert check_cfg_project(1.0, s) == 10000 and check_cfg_project(1, s) == 10000 and check_cfg_project(0.5, s) == 5000
        assert check_cfg_project(0.0001, s) == 1
        assert check_cfg_norm(0.05, s) == 500 and check_cfg_norm(10, s) == 100000 and check_cfg_norm(10.0, s) == 100000
        assert check_cfg_norm(0.0001, s) == 1 and check_cfg_norm(1.5, s) == 15000
    for bad in (1.0001, -0.1, 2, 10000, "1.0", [1.0], True, 0.00001):
        with pytest.raises(ValueError, match=re.escape("cfg_project must be") + ".*" + re.escape(repr(bad))):
            check_cfg_project(bad, "cfdg_ddpm_x0")
    for bad in (10.0001, -0.1, 11, 500, "0.05", [0.05], True, 0.00001):
        with pytest.raises(ValueError, match=re.escape("cfg_norm must be") + ".*" + re.escape(repr(bad))):
            check_cfg_norm(bad, "cfdg_ddpm_x0")
    for s in ("ddpm_x0", "generation_ddpm_x0", "ddim_x0", "ddpm", "ddim", "ddim2ddpm"):
        with pytest.raises(ValueError, match=r"cfg_project = 1.0 needs a sampler that guides"):
            check_cfg_project(1.0, s)
        with pytest.raises(ValueError, match=r"cfg_norm = 0.05 needs a sampler that guides"):
            check_cfg_norm(0.05, s)
    for check, name, value in ((check_cfg_project, "cfg_project", 1.0), (check_cfg_norm, "cfg_norm", 0.05)):
        with pytest.raises(ValueError, match=f"{name} = {value} does not combine with x0_threshold = 0.995"):
            check(value, "cfdg_ddpm_x0", 0.995, None)
        with pytest.raises(ValueError, match=f"{name} = {value} does not combine with cfg_rescale = 0.7"):
            check(value, "cfdg_ddpm_x0", None, 0.7)
        assert check(value, "cfdg_ddpm_x0", 0, 0.0) > 0 and check(value, "cfdg_ddpm_x0", None, False) > 0


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
    assert m.cfg_project() == 0 and m.cfg_norm() == 0
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_project": 1.0, "cfg_norm": 0.05})
    assert m.cfg_project() == 10000 and m.cfg_norm() == 500
    assert m.sampling_options()["cfg_project"] == 10000 and m.sampling_options()["cfg_norm"] == 500
    m.hparams.sampling.cfg_project = None             # read at every use
    assert m.cfg_project() == 0 and m.cfg_norm() == 500
    m.hparams.sampling.cfg_project = 0.5
    m.__dict__["_stride1"] = True                     # one of the reference's single-step methods is running
    assert m.cfg_project() == 0 and m.cfg_norm() == 0
    m.__dict__["_stride1"] = False
    assert m.cfg_project() == 5000
    m.hparams.sampling.cfg_project = 1.5              # refused at use, before the engine is reached
    with pytest.raises(ValueError, match="cfg_project must be"):
        m.engine
    with pytest.raises(ValueError, match="cfg_project must be"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    m.hparams.sampling.cfg_project = 1.0
    m.hparams.sampling.cfg_rescale = 0.7              # both refusals, at use
    with pytest.raises(ValueError, match="cfg_project = 1.0 does not combine with cfg_rescale = 0.7"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    m.hparams.sampling.cfg_rescale = None
    m.hparams.sampling.x0_clip = 1
    assert m.cfg_project() == 10000                   # (the clamp alone combines)
    m.hparams.sampling.x0_threshold = 0.995
    with pytest.raises(ValueError, match="cfg_project = 1.0 does not combine with x0_threshold = 0.995"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    for key, bad in (("cfg_project", 1.3), ("cfg_project", "1.0"), ("cfg_norm", 10.5), ("cfg_norm", 500)):
        with pytest.raises(ValueError, match=f"{key} must be"):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, key: bad})
    for key, value in (("cfg_project", 1.0), ("cfg_norm", 0.05)):
        with pytest.raises(ValueError, match="needs a sampler that guides"):
            _model(sampling={"type": "ddpm_x0", key: value})
        with pytest.raises(ValueError, match=f"{key} = {value} does not combine with cfg_rescale"):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, key: value, "cfg_rescale": 0.7})
        with pytest.raises(ValueError, match=f"{key} = {value} does not combine with x0_threshold"):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, key: value, "x0_clip": 1, "x0_threshold": 0.995})
    for word in ("cfg_project", "cfg_norm"):
        assert word in type(m).sample.__doc__, word


def test_load_from_checkpoint_override(golden_dir):
    """load_from_checkpoint(..., sampling=...) reads both keys through the same validators."""
    from diffroll_amd import ClassifierFreeDiffRoll
    path = os.path.join(golden_dir, "trained_small.ckpt")
    got = ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_project": 1.0, "cfg_norm": 0.05})
    assert got.cfg_project() == 10000 and got.cfg_norm() == 500
    plain = ClassifierFreeDiffRoll.load_from_checkpoint(path)
    assert plain.cfg_project() == 0 and plain.cfg_norm() == 0
    with pytest.raises(ValueError, match="cfg_norm must be"):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_norm": 11})
    with pytest.raises(ValueError, match="cfg_project = 1.0 does not combine with cfg_rescale"):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_project": 1.0, "cfg_rescale": 0.7})


def test_cli():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "task.sampling.w=3", "task.sampling.cfg_project=1.0", "task.sampling.cfg_norm=0.05"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 3, "cfg_project": 1.0, "cfg_norm": 0.05}
    plain = cli.build_config(["task=transcription"])["task"]["sampling"]
    assert "cfg_project" not in plain and "cfg_norm" not in plain
    assert cli.build_config(["task=transcription", "task.sampling.cfg_norm=null"])["task"]["sampling"]["cfg_norm"] is None
    for key, bads in (("cfg_project", ("1.3", "2", "10000", "high", "-0.5")), ("cfg_norm", ("10.5", "500", "high", "-0.5"))):
        for bad in bads:
            with pytest.raises(SystemExit, match=f"task.sampling.{key}"):
                cli.build_config(["task=transcription", f"task.sampling.{key}={bad}"])
    with pytest.raises(SystemExit, match="task.sampling.cfg_project.*needs a sampler that guides"):
        cli.build_config(["task=transcription", "task.sampling.type=ddim", "task.sampling.cfg_project=1.0"])
    with pytest.raises(SystemExit, match="task.sampling.cfg_norm.*does not combine with cfg_rescale"):
        cli.build_config(["task=transcription", "task.sampling.cfg_norm=0.05", "task.sampling.cfg_rescale=0.7"])
    with pytest.raises(SystemExit, match="task.sampling.cfg_project.*does not combine with x0_threshold"):
        cli.build_config(["task=transcription", "task.sampling.cfg_project=1.0", "task.sampling.x0_clip=1", "task.sampling.x0_threshold=0.995"])


# ---------------------------------------------------------------------------------------------- 4. the documents
def test_options_are_public_and_documented():
    from diffroll_amd import _cabi
    from diffroll_amd.engine import _MIRRORED, Engine
    for name in ("cfg_project", "cfg_norm"):
        assert name in _cabi.PUBLIC_OPTIONS and _MIRRORED[name] == 0 and getattr(Engine, name) == 0
        assert f"'{name}'" in Engine.set_option.__doc__ and f"'{name}'" in Engine.holding.__doc__
        assert not name.startswith("guidance")
    assert "dr_debug_project" in _cabi.DEBUG_EXPORTS and callable(Engine.project_stats)
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    begin = re.search(r'"cfg_project"\s+\[0\]', doc)
    assert begin and re.search(r'"cfg_norm"\s+\[0\]', doc)
    flat = re.sub(r"\s*\n \*\s*", " ", doc[begin.start():doc.index("Unknown names")])
    for word in ("1 .. 10000", "1 .. 100000", "Sadat et al. 2024", "without its momentum", "d_i = (double)y_i - (double)c_i",
                 "Scc = sum c_i c_i", "Scd = sum c_i d_i", "Sdd = sum d_i d_i", "k = Scd / Scc", "k = 0.0 when !(Scc > 0)",
                 "rho = (double)cfg_project / 10000.0", "r = (double)cfg_norm / 10000.0", "q = sqrt(Sdd / N) / fabs((double)w)",
                 "if (q > r) s = r / q", "a = (float)((1.0 - s) - s (rho k))", "b = (float)s",
                 "a = 0.0f, b = 1.0f exactly when a or b is not finite", "y' = (a c) + (b y)", "in pitch order", "blocks of 64",
                 "in row, then block order", "no floating-point atomic", "frames [O, T)", "DR_MODE_FUSED_STACK",
                 "keeps its tail kernel", "naming the value", 'beside "x0_threshold"', 'beside "cfg_rescale"', "naming both options",
                 '"sampling_steps"', '"window_break"', '"window_blend"', '"draws"', '"guidance_t_min" / "guidance_t_max"',
                 '"solver_order" / "solver_noise"', '"start_step" / "start_noise"', '"x0_clip"', "all three precisions", "sharding",
                 "captured chain's key", "dr_sample_checked", "INTEGRATION.md 3c"):
        assert word in flat, word
    assert "dr_debug_project(" in open(os.path.join(ROOT, "include", "diffroll_amd_debug.h")).read()
    for doc_name, words in (("README.md", ("cfg_project", "cfg_norm", "profiles/project_kernel_resources.txt", "profiles/project_sweep.txt")),
                            ("INTEGRATION.md", ('"cfg_project"', '"cfg_norm"', "task.sampling.cfg_project", "task.sampling.cfg_norm"))):
        body = open(os.path.join(ROOT, doc_name)).read()
        for word in words:
            assert word in body, (doc_name, word)
    abi = open(os.path.join(ROOT, "diffroll_amd", "csrc", "abi.hip")).read()
    assert '{"cfg_project", &ChainOptions::cfg_project,' in abi and '{"cfg_norm", &ChainOptions::cfg_norm,' in abi      # (their rows of the option table)
    quad = open(os.path.join(ROOT, "diffroll_amd", "csrc", "project_quad.h")).read()
    assert "momentum" in quad and '"cfg_rescale"' in quad      # what is left out, said where the code is


def test_the_built_library_knows_the_options():
    """Without a GPU no engine exists to set the options on.  What can be held: the library exports dr_debug_project, carries
    the options' own refusal texts (a library without them has none), and a null handle is DR_EINVAL, never a crash."""
    from diffroll_amd import _cabi
    if not os.path.exists(_cabi.LIB_PATH):
        pytest.skip("the library is not built (python -m diffroll_amd.build)")
    lib = _cabi.load_library()                        # (built: a load failure is a failure, not a skip)
    assert hasattr(lib, "dr_debug_project")
    blob = open(_cabi.LIB_PATH, "rb").read()
    for text in (b"cfg_project is 0 (off) or rho in units of 1 / 10000", b"cfg_norm is 0 (off) or the rms bound r in units of 1 / 10000",
                 b"do not combine with x0_threshold = %d", b"do not combine with cfg_rescale = %d"):
        assert text in blob, text
    assert lib.dr_set_option(None, b"cfg_project", 10000) == _cabi.DR_EINVAL
    assert lib.dr_set_option(None, b"cfg_norm", 500) == _cabi.DR_EINVAL
    assert lib.dr_debug_project(None, None, None, 1, 1, 0.0, None, None) == _cabi.DR_EINVAL


def test_the_parents_kernels_keep_their_text():
    """The projecting form is a further instantiation of update_quad and a second argument: UpdateArgs does not grow, tail.hip
    names none of the options' pieces, the clamp call lives in project_quad.h, and the statistics use no floating-point
    atomic and wait for nobody."""
    csrc = os.path.join(ROOT, "diffroll_amd", "csrc")
    tail = open(os.path.join(csrc, "tail.hip")).read().lower()
    assert "project_" not in tail and "cfg_" not in tail and "projected" not in tail
    kern = open(os.path.join(csrc, "kernels.h")).read()
    upd = kern[kern.index("struct UpdateArgs {"):kern.index("// (mode 5) the half the step reads")]
    assert "project" not in upd.lower() and upd.rstrip().endswith("float clamp_lo, clamp_hi;\n};".rstrip())
    quad = open(os.path.join(csrc, "project_quad.h")).read()
    assert quad.count("clamp_quad(") == 1 and open(os.path.join(csrc, "update_quad.h")).read().count("clamp_quad(") == 2
    update = open(os.path.join(csrc, "update.hip")).read()
    assert "update_project_kernel" in update
    for word in ("clamp_quad", "clamp_lo", "blend_quad"):
        assert word not in update, word
    hip = open(os.path.join(csrc, "project.hip")).read()
    skel = open(os.path.join(csrc, "group_sums.h")).read()      # the loops of the statistics launch, which project.hip instantiates
    src = hip + quad + skel
    # contraction off throughout: for the whole of project.hip and of the skeleton in front of their first function, and in every
    # function of the two headers (project_quad.h: the frame's sums and their in_y, the coefficients, the record, the update's form)
    pragma = "#pragma clang fp contract(off)"
    assert hip.index(pragma) < hip.index("DR_DEVINL") and quad.count(pragma) == quad.count("DR_DEVINL void") == 5
    assert skel.index(pragma) < skel.index("DR_DEVINL") and skel.count(pragma) == skel.count("DR_DEVINL") + 1
    assert '#include "group_sums.h"' in hip and "gs_roll<ProjectStat>(a)" in hip and "gs_grid<ProjectStat>(a)" in hip
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    for banned in ("unsafeAtomicAdd", "atomicAdd(", "atomicMax(", "atomicMin(", "while (", "__builtin_amdgcn_s_sleep"):
        assert banned not in code, banned
    assert "project_roll_kernel" in code and "project_grid_kernel" in code
    from diffroll_amd import build
    assert "project.hip" in build.SOURCES and any(h.endswith("project_quad.h") for h in build.HEADERS)
