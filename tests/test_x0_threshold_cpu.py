"""Option "x0_threshold" (include/diffroll_amd.h) without a GPU: the restated quantile of tests/thresh_ref.py against
torch.quantile (the definition), its order on ties / zeros / inf / NaN, "inert => identical" in the restatement, that the
inputs of the GPU tests are active or inert as tests/thresh_cases.py claims, and the Python surface (check_x0_threshold,
hparams.sampling.x0_threshold, the CLI, the documents)."""
import os
import re

import pytest
import torch

from testlib import ATOL

import clip_cases as CC
import clip_ref as CL
import thresh_cases as TC
import thresh_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = CC.S
VS = (5000, 9000, 9950, 9999, 10000)


# ---------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("v", VS)
def test_restated_quantile_is_torch_quantile(v):
    """Random rolls and the test network's predictions: rtol 1e-5 - this checks the definition only.  torch.quantile is given
    the fp32 values as float64: in fp32 it rounds the position v (N - 1) / 10000 itself to fp32 (3518.648 has 2.4e-4 between
    neighbours), an error of its own that reaches 2.4e-5 of q at v = 9999 and that the option's integer k / rem does not have."""
    hp, p, _, x, _, spec = CC.setup()
    import chain_ref as CR
    from oracle import diffroll_ref as R
    y_net = CR.prediction(p, hp, "cfdg_ddpm_x0", x, spec, S - 1, 3.0, R.build_embedding(S))
    g = torch.Generator().manual_seed(3)
    for y in (torch.randn(3, 1, 40, 88, generator=g), 2.0 * torch.randn(1, 1, 1, 88, generator=g), y_net):
        for code in (1, 2):
            m, _ = TR.centre(code)
            qs = TR.group_stats(y, code, v, TR.clip_groups(y.shape[0]))
            for b in range(y.shape[0]):
                want = torch.quantile((y[b] - m).abs().reshape(-1).double(), v / 10000.0)
                assert torch.allclose(qs[b, 0].double(), want, rtol=1e-5, atol=0.0), (code, b, float(qs[b, 0]), float(want))


def test_restated_order_on_ties_zeros_inf_and_nan():
    inf, nan = float("inf"), float("nan")
    y = torch.zeros(1, 1, 1, 88)
    q = lambda t, v, code=2: TR.group_stats(t, code, v, TR.clip_groups(1))[0]
    assert q(y, 9950).tolist() == [0.0, 1.0]                       # all equal (and -0 == +0 below)
    y[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, -3.0, 3.0])
    assert float(q(y, 10000)[0]) == 3.0 and float(q(y, 9000)[0]) == 0.0
    # two values, the tie straddling k and k + 1: N = 88, v = 5000 -> num = 435000, k = 43, rem = 5000
    y = torch.cat([torch.full((44,), -1.5), torch.full((44,), 2.5)]).reshape(1, 1, 1, 88)
    assert q(y, 5000).tolist() == [2.0, 2.0]                       # a[43] = 1.5, a[44] = 2.5, f = 0.5
    y = torch.cat([torch.full((45,), -1.5), torch.full((43,), 2.5)]).reshape(1, 1, 1, 88)
    assert q(y, 5000).tolist() == [1.5, 1.5]                       # a[43] = a[44] = 1.5
    y = torch.randn(1, 1, 2, 88, generator=torch.Generator().manual_seed(1))
    y[0, 0, 0, 0], y[0, 0, 1, 5] = inf, -inf
    assert q(y, 10000).tolist() == [inf, inf] and float(q(y, 9000)[0]) < 4.0
    a = q(y, 9999)                                                 # a[k] = a[k + 1] = inf: inf + f (inf - inf) is a NaN, s = r
    assert torch.isnan(a[0]) and float(a[1]) == 1.0
    y[0, 0, 1, 7] = nan                                            # one NaN sorts last
    assert torch.isnan(q(y, 10000)[0]) and float(q(y, 10000)[1]) == 1.0 and float(q(y, 9000)[0]) < 4.0
    assert q(torch.full((1, 1, 1, 88), nan), 9000, 1)[1] == 0.5    # only NaN: s = r
    out, _ = TR.threshold(y, 2, 9000, TR.clip_groups(1))
    assert torch.isnan(out[0, 0, 1, 7]) and float(out[0, 0, 0, 0]) == 1.0 and float(out[0, 0, 1, 5]) == -1.0


def test_window_groups_count_every_canvas_frame_once():
    assert TR.window_groups(3, 2) == [[(0, 0), (1, 2), (2, 2)]]
    assert TR.window_groups(3, 2, marks=(2,)) == [[(0, 0), (1, 2)], [(2, 0)]]
    assert TR.window_groups(6, 2, marks=(2,), draws=2) == [[(0, 0), (1, 2)], [(2, 0)], [(3, 0), (4, 2)], [(5, 0)]]
    hp, p, plan, _, _ = CC.long_case()
    y = torch.randn(plan.n, 1, plan.T, 88, generator=torch.Generator().manual_seed(2))
    import chain_ref as CR
    ym = CR.shared_mean(y, plan)
    assert torch.equal(ym, TR.shared_mean(y, TR.window_groups(plan.n, plan.overlap), plan.stride, plan.overlap))
    canvas = torch.cat([ym[0, 0]] + [ym[b, 0, plan.overlap:] for b in range(1, plan.n)])
    assert canvas.numel() == ((plan.n - 1) * plan.stride + plan.T) * 88 == plan.T_c * 88
    qs = TR.group_stats(ym, 2, 9950, TR.window_groups(plan.n, plan.overlap))
    assert torch.equal(qs, TR.group_stats(canvas.reshape(1, 1, -1, 88), 2, 9950, TR.clip_groups(1)))


# ---------------------------------------------------------------------------------------------- 2. inert => identical, active
@pytest.mark.parametrize("sampler,w,code,v", TC.INERT, ids=[f"{s}-w{w:g}-code{c}-v{v}" for s, w, c, v in TC.INERT])
def test_inert_cases_are_the_clipped_chain(sampler, w, code, v):
    TC.assert_inert(sampler, w, code, v, 20)


@pytest.mark.parametrize("sampler,w,code,v,n", TC.CASES, ids=TC.CASE_IDS)
def test_gpu_cases_are_active(sampler, w, code, v, n):
    for philox in ((False,) if n == 0 else (False, True)):
        TC.assert_active(sampler, w, code, v, n, philox)


@pytest.mark.parametrize("name,kw", TC.OPTION_CASES, ids=[c[0] for c in TC.OPTION_CASES])
def test_gpu_option_cases_are_active(name, kw):
    TC.assert_active(*TC.GUIDED, 20, **kw)


def test_the_issues_figures():
    """cfdg_ddpm_x0, n = 20 on clip_cases.setup(): code 2, w = 3, v = 9950 has q > 1 at all 40 (step, roll) pairs; v = 9000 is
    inert; code 1 has q(|y - 0.5|) > 0.5 everywhere."""
    _, stats, r = TC.reference("cfdg_ddpm_x0", 3.0, 2, 9950, 20)
    qs = torch.cat([s[:, 0] for s in stats.values()])
    assert qs.numel() == 40 and float(qs.min()) > 1.0
    _, stats, _ = TC.reference("cfdg_ddpm_x0", 3.0, 2, 9000, 20)
    assert float(torch.cat([s[:, 0] for s in stats.values()]).max()) <= 1.0
    _, stats, _ = TC.reference("cfdg_ddpm_x0", 0.5, 1, 9000, 20)
    assert float(torch.cat([s[:, 0] for s in stats.values()]).min()) > 0.5


def test_gpu_fused_and_long_cases_are_active():
    for (roll, stats, r), clipped in ((TC.fused_reference(), CC.fused_reference(2)[0]), (TC.long_reference(), CC.long_reference(2)[0])):
        flags = TR.active(stats, r)
        assert flags and all(flags)
        assert float((roll - clipped).abs().max()) >= 100 * ATOL
    hp, p, plan, _, _ = CC.long_case()
    roll, stats, _ = TC.long_reference()
    assert all(s.shape == (1, 2) for s in stats.values())          # one q per step over the recording's canvas
    H, O, T = plan.stride, plan.overlap, plan.T
    for b in range(plan.n - 1):
        assert torch.equal(roll[b, :, H:T], roll[b + 1, :, 0:O]), b


# ---------------------------------------------------------------------------------------------- 3. the Python surface
def test_check_x0_threshold():
    from diffroll_amd.schedule import X0_SAMPLERS, check_x0_threshold
    for off in (None, 0, False, 0.0):
        assert check_x0_threshold(off) == 0 and check_x0_threshold(off, "ddim", None) == 0
    for s in X0_SAMPLERS:
        assert check_x0_threshold(0.995, s, 1) == 9950
        assert check_x0_threshold(0.5, s, True) == 5000 and check_x0_threshold(1, s, 1) == 10000 and check_x0_threshold(1.0, s, 1) == 10000
        assert check_x0_threshold(0.99995, s, 1) == 10000 and check_x0_threshold(0.9, s, 1) == 9000
    for bad in (0.4999, 1.0001, -1, 2, 9950, "0.995", [0.995], True):
        with pytest.raises(ValueError, match=re.escape("x0_threshold must be") + ".*" + re.escape(repr(bad))):
            check_x0_threshold(bad, "cfdg_ddpm_x0", 1)
    for clip in (None, 0, False):
        with pytest.raises(ValueError, match=r"x0_threshold = 0.995 needs x0_clip"):
            check_x0_threshold(0.995, "cfdg_ddpm_x0", clip)
    for s in ("ddpm", "ddim", "ddim2ddpm"):
        with pytest.raises(ValueError, match=r"x0_threshold.*x0_clip.*epsilon"):
            check_x0_threshold(0.995, s, 1)


def _model(**kw):
    from diffroll_amd import ClassifierFreeDiffRoll
    base = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=229, norm_args=[0, 1, "imagewise"],
                residual_layers=2, kernel_size=3, dilation_base=2, dilation_bound=4,
                spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000,
                               center=True, normalized=True, pad_mode="reflect"),
                timesteps=S)
    base.update(kw)
    return ClassifierFreeDiffRoll(**base)


def test_facade_hparams_x0_threshold():
    assert _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "x0_clip": True}).x0_threshold() == 0
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "x0_clip": True, "x0_threshold": 0.995})
    assert m.x0_threshold() == 9950 and m.x0_clip() == 1
    m.hparams.sampling.x0_threshold = None            # read at every use
    assert m.x0_threshold() == 0
    m.hparams.sampling.x0_threshold = 0.9
    m.__dict__["_stride1"] = True                     # one of the reference's single-step methods is running
    assert m.x0_threshold() == 0
    m.__dict__["_stride1"] = False
    assert m.x0_threshold() == 9000
    m.hparams.sampling.x0_clip = 0                    # refused at use, before the engine is reached
    with pytest.raises(ValueError, match="needs x0_clip"):
        m.engine
    with pytest.raises(ValueError, match="needs x0_clip"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    for bad in (0.3, 9950, "0.995"):
        with pytest.raises(ValueError, match="x0_threshold must be"):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "x0_clip": 1, "x0_threshold": bad})
    with pytest.raises(ValueError, match="needs x0_clip"):
        _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "x0_threshold": 0.995})
    with pytest.raises(ValueError, match="epsilon"):
        _model(sampling={"type": "ddim", "x0_threshold": 0.995})


def test_cli_x0_threshold():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "task.sampling.w=3", "task.sampling.x0_clip=1", "task.sampling.x0_threshold=0.995"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 3, "x0_clip": 1, "x0_threshold": 0.995}
    assert "x0_threshold" not in cli.build_config(["task=transcription"])["task"]["sampling"]
    assert cli.build_config(["task=transcription", "task.sampling.x0_threshold=null"])["task"]["sampling"]["x0_threshold"] is None
    for bad in ("0.3", "2", "9950", "high"):
        with pytest.raises(SystemExit, match="task.sampling.x0_threshold"):
            cli.build_config(["task=transcription", "task.sampling.x0_clip=1", f"task.sampling.x0_threshold={bad}"])
    with pytest.raises(SystemExit, match="task.sampling.x0_threshold.*needs x0_clip"):
        cli.build_config(["task=transcription", "task.sampling.x0_threshold=0.995"])
    with pytest.raises(SystemExit, match="task.sampling.x0_threshold.*epsilon"):
        cli.build_config(["task=transcription", "task.sampling.type=ddim", "task.sampling.x0_threshold=0.995"])


def test_load_from_checkpoint_override(golden_dir):
    from diffroll_amd import ClassifierFreeDiffRoll
    path = os.path.join(golden_dir, "trained_small.ckpt")
    m = ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 2.0, "steps": 20, "x0_clip": 1,
                                                                    "x0_threshold": 0.995})
    assert m.x0_threshold() == 9950 and m.x0_clip() == 1
    assert ClassifierFreeDiffRoll.load_from_checkpoint(path).x0_threshold() == 0


# ---------------------------------------------------------------------------------------------- 4. the documents
def test_option_is_public_and_documented():
    from diffroll_amd import _cabi
    from diffroll_amd.engine import _MIRRORED, Engine
    assert "x0_threshold" in _cabi.PUBLIC_OPTIONS and "dr_debug_threshold" in _cabi.DEBUG_EXPORTS
    assert _MIRRORED["x0_threshold"] == 0 and Engine.x0_threshold == 0
    assert "'x0_threshold'" in Engine.set_option.__doc__ and "'x0_threshold'" in Engine.holding.__doc__
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    assert "is not offered" not in text
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    begin = re.search(r'"x0_threshold"\s+\[0\]', doc)
    assert begin
    flat = re.sub(r"\s*\n \*\s*", " ", doc[begin.start():doc.index("Unknown names")])
    for word in ("5000 .. 10000", "9950", '"x0_clip"', "num = value (N - 1)", "a NaN q gives s = r", "bit-identical to the \"x0_clip\" step",
                 "RECORDING'S CANVAS", "frames [O, T)", "DR_MODE_FUSED_STACK", "tail_launches does not move", "naming both", "naming the value",
                 '"sampling_steps"', '"window_overlap"', '"draws"', '"guidance_t_min"', '"solver_order"', '"solver_noise"', '"start_step"',
                 "both precisions", "sharding", "captured chain's key", "dr_sample_checked", "profiles/thresh_sweep.txt", "INTEGRATION.md 3c"):
        assert word in flat, word
    assert "dr_debug_threshold(" in open(os.path.join(ROOT, "include", "diffroll_amd_debug.h")).read()
    for doc_name, words in (("README.md", ("x0_threshold", "profiles/thresh_sweep.txt", "profiles/thresh_kernel_resources.txt")),
                            ("INTEGRATION.md", ('"x0_threshold"', "task.sampling.x0_threshold")), ("DESIGN.md", ('"x0_threshold"',))):
        body = open(os.path.join(ROOT, doc_name)).read()
        assert "thresholding is not offered" not in body, doc_name
        for word in words:
            assert word in body, (doc_name, word)
    if os.path.exists(_cabi.LIB_PATH):               # (built: a load failure is a failure, not a skip)
        lib = _cabi.load_library()
        assert lib.dr_set_option(None, b"x0_threshold", 9950) == _cabi.DR_EINVAL      # a null handle, never a crash
        assert lib.dr_debug_threshold(None, None, None, 1, 1, 0.0, None, None) == _cabi.DR_EINVAL


def test_the_tail_kernel_keeps_its_text():
    """The thresholding form is a second instantiation: UpdateArgs does not grow, tail.hip neither names the option's pieces
    nor includes their header, and the selection uses integer counts only."""
    csrc = os.path.join(ROOT, "diffroll_amd", "csrc")
    tail = open(os.path.join(csrc, "tail.hip")).read()
    assert "thresh" not in tail and "threshold_quad.h" not in tail
    kern = open(os.path.join(csrc, "kernels.h")).read()
    upd = kern[kern.index("struct UpdateArgs {"):kern.index("// (mode 5) the half the step reads")]
    assert "thresh" not in upd.lower() and upd.rstrip().endswith("float clamp_lo, clamp_hi;\n};".rstrip())
    sel = open(os.path.join(csrc, "threshold.hip")).read()
    code = "\n".join(line.split("//")[0] for line in sel.splitlines())
    assert "atomicAdd(&hist" in code and "float*>(a.work" in code
    for banned in ("unsafeAtomicAdd", "atomicAdd((float", "atomicMax((float", "atomicMin((float", "while (", "__builtin_amdgcn_s_sleep"):
        assert banned not in code, banned
