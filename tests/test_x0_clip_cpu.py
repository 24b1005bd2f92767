"""Option "x0_clip" (include/diffroll_amd.h) without a GPU: the restatement tests/clip_ref.py against tests/chain_ref.py
with the option off, the Python surface (check_x0_clip, hparams.sampling.x0_clip, the CLI), the documents, that the inputs
of the GPU tests exercise the bounds they claim, and the two properties a clamped chain has by construction."""
import os
import re

import pytest
import torch

import chain_ref as CR
import clip_cases as CC
import clip_ref as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = CC.S


# ---------------------------------------------------------------------------------------------- 1. code 0 is chain_ref
OFF = [
    ("plain", "cfdg_ddpm_x0", dict(w=3.0)),
    ("interval", "cfdg_ddpm_x0", dict(w=3.0, interval=(60, 140))),
    ("order2-noise", "cfdg_ddpm_x0", dict(w=3.0, order=2, solver_noise=1)),
    ("started", "ddpm_x0", dict(start=CR.visited(S, 20)[7])),
    ("ddim", "cfdg_ddim_x0", dict(w=0.5, trajectory=True)),
]


@pytest.mark.parametrize("name,sampler,kw", OFF, ids=[c[0] for c in OFF])
def test_code_0_is_the_chain_of_chain_ref(name, sampler, kw):
    hp, p, _, x, noise, spec = CC.setup()
    want = CR.sample_chain(p, hp, sampler, x, spec, noise, 20, **kw)
    got, moved = CL.sample_chain(p, hp, sampler, x, spec, noise, 20, code=0, **kw)
    assert torch.equal(got, want)
    assert all(v == (0.0, 0.0) for v in moved.values()) and list(moved) == list(CR.chain_rows(hp, sampler, 20, start=kw.get("start")))


def test_code_0_in_windows_is_the_chain_of_chain_ref():
    hp, p, plan, _, _ = CC.long_case()
    xw, spec, z = CC.long_inputs(4)
    want = CR.sample_chain(p, hp, "cfdg_ddpm_x0", xw, spec, z, 4, w=3.0, plan=plan)
    got, _ = CL.sample_chain(p, hp, "cfdg_ddpm_x0", xw, spec, z, 4, code=0, w=3.0, plan=plan)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- 2. the Python surface
def test_check_x0_clip():
    from diffroll_amd.schedule import X0_SAMPLERS, check_x0_clip
    for off in (None, 0, False):
        assert check_x0_clip(off) == 0 and check_x0_clip(off, "ddim", [0, 1, "imagewise"]) == 0
        assert check_x0_clip(off, "ddpm_x0", [0, 5, "imagewise"]) == 0          # off: the range is not looked at
    for s in X0_SAMPLERS:
        for on in (1, True):
            assert check_x0_clip(on, s, [0, 1, "imagewise"]) == 1
            assert check_x0_clip(on, s, (-1, 1, "framewise")) == 2
            assert check_x0_clip(on, s, [0.0, 1.0]) == 1
    assert check_x0_clip(1) == 1                                                # the released range by default
    for rng in ([0, 2, "imagewise"], [-1, 0, "imagewise"], [1, 0], [0], ["a", 1], None, "01"):
        with pytest.raises(ValueError, match="norm_args"):
            check_x0_clip(1, "cfdg_ddpm_x0", rng)
    with pytest.raises(ValueError, match=r"\[0, 2\]"):                            # ... naming the range
        check_x0_clip(1, "cfdg_ddpm_x0", [0, 2, "imagewise"])
    for s in ("ddpm", "ddim", "ddim2ddpm"):
        with pytest.raises(ValueError, match="epsilon"):
            check_x0_clip(1, s, [0, 1, "imagewise"])
    for bad in (2, 3, -1, 1.0, "1", [1]):
        with pytest.raises(ValueError, match=re.escape(f"x0_clip must be") + ".*" + re.escape(repr(bad))):
            check_x0_clip(bad, "cfdg_ddpm_x0", [0, 1, "imagewise"])


def _model(**kw):
    from diffroll_amd import ClassifierFreeDiffRoll
    base = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=229, norm_args=[0, 1, "imagewise"],
                residual_layers=2, kernel_size=3, dilation_base=2, dilation_bound=4,
                spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000,
                               center=True, normalized=True, pad_mode="reflect"),
                timesteps=S)
    base.update(kw)
    return ClassifierFreeDiffRoll(**base)


def test_facade_hparams_x0_clip():
    assert _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5}).x0_clip() == 0
    assert _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "x0_clip": None}).x0_clip() == 0
    m = _model(sampling={"type": "cfdg_ddim_x0", "w": 3.0, "steps": 10, "solver_order": 2, "x0_clip": True})
    assert m.x0_clip() == 1 and m.solver_order() == 2 and m.sampling_steps() == 10
    assert _model(norm_args=[-1, 1, "imagewise"], sampling={"type": "ddpm_x0", "x0_clip": 1}).x0_clip() == 2
    m.hparams.sampling.x0_clip = 0                    # read at every use
    assert m.x0_clip() == 0
    m.hparams.sampling.x0_clip = 1
    m.__dict__["_stride1"] = True                     # one of the reference's single-step methods is running
    assert m.x0_clip() == 0
    m.__dict__["_stride1"] = False
    assert m.x0_clip() == 1
    m.hparams.sampling.x0_clip = 2                    # ... and refused there, before the engine is reached
    with pytest.raises(ValueError, match="x0_clip"):
        m.engine
    with pytest.raises(ValueError, match="x0_clip"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    m.hparams.sampling.x0_clip = 1
    m.hparams.norm_args[1] = 2                        # a range the engine has no code for: at use too
    with pytest.raises(ValueError, match="norm_args"):
        m.engine
    # at construction
    for bad in (2, -1, "1", 1.5):
        with pytest.raises(ValueError, match="x0_clip"):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "x0_clip": bad})
    with pytest.raises(ValueError, match="norm_args"):
        _model(norm_args=[0, 2, "imagewise"], sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "x0_clip": 1})
    for s in ("ddpm", "ddim", "ddim2ddpm"):
        with pytest.raises(ValueError, match="epsilon"):
            _model(sampling={"type": s, "x0_clip": 1})
        assert _model(sampling={"type": s, "x0_clip": 0}).x0_clip() == 0


def test_cli_x0_clip():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "task.sampling.w=3", "task.sampling.x0_clip=1"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 3, "x0_clip": 1}
    assert cli.build_config(["task=transcription", "task.sampling.x0_clip=true"])["task"]["sampling"]["x0_clip"] is True
    assert cli.build_config(["task=transcription", "task.sampling.x0_clip=null"])["task"]["sampling"]["x0_clip"] is None
    assert cli.build_config(["task=transcription", "task.sampling.x0_clip=0"])["task"]["sampling"]["x0_clip"] == 0
    assert "x0_clip" not in cli.build_config(["task=transcription"])["task"]["sampling"]
    for bad in ("2", "-1", "1.5", "one", "[1]"):
        with pytest.raises(SystemExit, match="task.sampling.x0_clip"):
            cli.build_config(["task=transcription", f"task.sampling.x0_clip={bad}"])
    with pytest.raises(SystemExit, match="task.sampling.x0_clip.*epsilon"):
        cli.build_config(["task=transcription", "task.sampling.type=ddim", "task.sampling.x0_clip=1"])
    with pytest.raises(SystemExit, match="task.sampling.x0_clip.*norm_args"):
        cli.build_config(["task=transcription", "model.args.norm_args=[0,2,'imagewise']", "task.sampling.x0_clip=1"])
    cfg = cli.build_config(["task=transcription", "model.args.norm_args=[-1,1,'imagewise']", "task.sampling.x0_clip=1"])
    assert cfg["task"]["sampling"]["x0_clip"] == 1


def test_load_from_checkpoint_override(golden_dir):
    from diffroll_amd import ClassifierFreeDiffRoll
    path = os.path.join(golden_dir, "trained_small.ckpt")
    m = ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 2.0, "steps": 20, "x0_clip": 1})
    assert m.x0_clip() == 1 and m.sampling_steps() == 20
    assert ClassifierFreeDiffRoll.load_from_checkpoint(path).x0_clip() == 0
    with pytest.raises(ValueError, match="x0_clip"):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "x0_clip": 2})


def test_every_rank_gets_the_option():
    """distributed.py passes nothing per option: every rank calls model.sample on the model it was handed, which syncs
    hparams.sampling.x0_clip into that rank's engine."""
    from diffroll_amd import distributed

    class Rank:
        def __init__(self):
            self.m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "steps": 20, "x0_clip": 1})
            self.calls = []

        def sample(self, x, wav, noise=None, seed=0, first_sample=0, **kw):
            self.calls.append((self.m.x0_clip(), tuple(x.shape), seed, first_sample))
            return x, None

    x, wav, z = torch.zeros(4, 1, 8, 88), torch.zeros(4, 4096), torch.zeros(S, 4, 1, 8, 88)
    ranks = [Rank(), Rank()]
    for r, m in enumerate(ranks):
        distributed.sample_shard(m, x, wav, z, 7, r, 2)
    assert ranks[0].calls == [(1, (2, 1, 8, 88), 7, 0)] and ranks[1].calls == [(1, (2, 1, 8, 88), 7, 2)]


# ---------------------------------------------------------------------------------------------- 3. the documents
def test_option_is_public_and_documented():
    from diffroll_amd import _cabi
    from diffroll_amd.engine import _MIRRORED, Engine
    assert _cabi.DR_ABI_VERSION == 11
    assert "x0_clip" in _cabi.PUBLIC_OPTIONS
    assert _MIRRORED["x0_clip"] == 0 and Engine.x0_clip == 0
    assert "'x0_clip'" in Engine.set_option.__doc__ and "'x0_clip'" in Engine.holding.__doc__
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", text).group(1)) == 11
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    begin = re.search(r'"x0_clip"\s+\[0\]', doc)
    assert begin
    flat = re.sub(r"\s*\n \*\s*", " ", doc[begin.start():doc.index("Unknown names")])        # the entry as running text
    for word in ("[0, 1]", "[-1, 1]", "shared-frame mean", "[lo / c2, hi / c2]", "a NaN stays a NaN", "DR_EINVAL", "naming both",
                 '"sampling_steps"', '"window_overlap"', '"draws"', '"guidance_t_min"', '"solver_order"', '"solver_noise"',
                 '"start_step"', '"start_noise"', "both precisions", "sharding", "captured chain's key", "dr_sample_checked",
                 "INTEGRATION.md 3c"):
        assert word in flat, word
    for doc_name, words in (("README.md", ("x0_clip", "profiles/clip_sweep.txt", "profiles/clip_kernel_resources.txt")),
                            ("INTEGRATION.md", ('"x0_clip"', "task.sampling.x0_clip")), ("DESIGN.md", ('"x0_clip"',))):
        body = open(os.path.join(ROOT, doc_name)).read()
        for word in words:
            assert word in body, (doc_name, word)
    if os.path.exists(_cabi.LIB_PATH):               # (built: a load failure is a failure, not a skip)
        assert _cabi.load_library().dr_set_option(None, b"x0_clip", 1) == _cabi.DR_EINVAL      # a null handle, never a crash


def test_the_clamp_is_written_once_as_compare_and_select():
    """The reading item of the option: y < lo ? lo : (y > hi ? hi : y) keeps a NaN (torch.clamp does), fminf(fmaxf()) would
    turn it into lo.  The arithmetic lives in update_quad.h alone; update_kernel and the tail kernel's part T3 call it."""
    csrc = os.path.join(ROOT, "diffroll_amd", "csrc")
    quad = open(os.path.join(csrc, "update_quad.h")).read()
    body = quad[quad.index("DR_DEVINL void clamp_quad("):]
    body = body[:body.index("}") + 1]
    assert "y[e] < lo ? lo : (y[e] > hi ? hi : y[e])" in body
    assert "fminf" not in body and "fmaxf" not in body
    assert quad.count("clamp_quad(") == 2              # the definition and its one call, in update_quad
    assert quad.index("clamp_quad(a.clamp_lo") < quad.index("if (pred) *pred =")          # the history receives the clamped y
    for unit in ("update.hip", "tail.hip"):
        src = open(os.path.join(csrc, unit)).read()
        assert "update_quad(" in src and "clamp_quad" not in src and "clamp_lo" not in src, unit
    y = torch.tensor([float("nan"), -2.0, 0.25, 2.0])
    out = y.clamp(0.0, 1.0)
    assert torch.isnan(out[0]) and out[1:].tolist() == [0.0, 0.25, 1.0]


# ---------------------------------------------------------------------------------------------- 4. the GPU cases clamp
@pytest.mark.parametrize("sampler,w,code,n", CC.CASES, ids=CC.CASE_IDS)
def test_gpu_cases_exercise_the_clamp(sampler, w, code, n):
    # (the replayed Philox draws of the 200-step chains are held to the same conditions where they are computed anyway: in
    # tests/test_gpu_x0_clip.py, before the engine's roll is looked at)
    for philox in ((False,) if n == 0 else (False, True)):
        CC.assert_exercised(sampler, w, code, n, philox)


@pytest.mark.parametrize("name,kw", CC.OPTION_CASES, ids=[c[0] for c in CC.OPTION_CASES])
def test_gpu_option_cases_exercise_the_clamp(name, kw):
    CC.assert_exercised("cfdg_ddpm_x0", 3.0, 1, 20, **kw)


def test_gpu_fused_case_exercises_the_clamp():
    roll, moved = CC.fused_reference()
    CC.exercised(moved, ("lo", "hi"), roll, CC.fused_reference(0)[0])
    assert CC.in_range(roll, CC.fused_case()[0], 1)


# ---------------------------------------------------------------------------------------------- 5. by construction
def test_windows_shared_frames_are_equal_and_the_roll_is_in_range():
    hp, p, plan, _, _ = CC.long_case()
    roll, moved = CC.long_reference()
    CC.exercised(moved, ("lo", "hi"), roll, CC.long_reference(0)[0])
    H, O, T = plan.stride, plan.overlap, plan.T
    for b in range(plan.n - 1):
        assert torch.equal(roll[b, :, H:T], roll[b + 1, :, 0:O]), b
    assert CC.in_range(roll, hp, 1)
    c2 = CL.last_scale(hp)
    assert float(roll.min()) == 0.0 and float(roll.max()) == float(torch.tensor(1.0) / torch.tensor(c2))      # both bounds are reached
