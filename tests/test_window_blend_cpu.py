"""Option "window_blend" without a GPU: the CPU restatement of tests/blend_ref.py against chain_ref.shared_mean and against
the option's definition, the references of tests/blend_cases.py (do modes 1 and 2 move the roll at all?), the façade's
validator and CLI key, and the documents."""
import os
import re

import pytest
import torch

from testlib import header_functions

import blend_cases as BC
import blend_ref as BR
import chain_ref as CR

from diffroll_amd import cli, longform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-5                                          # the parity bound of the GPU tests
OS = (1, 5, 16)


def windows(O, n=3, T=32, seed=0):
    plan = longform.plan_windows((n - 1) * (T - O) + T, None, T, O)
    assert plan.n == n
    return plan, torch.randn(n, 1, T, 88, generator=torch.Generator().manual_seed(seed + O))


# ---------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("O", OS)
def test_mode_0_is_the_shared_mean_bit_for_bit(O):
    plan, y = windows(O)
    assert torch.equal(BR.blend(y, plan, 0), CR.shared_mean(y, plan))


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("O", OS)
def test_shared_frames_agree_and_the_rest_is_untouched(O, mode):
    plan, y = windows(O)
    out = BR.blend(y, plan, mode)
    H, T = plan.stride, plan.T
    for b in range(plan.n - 1):
        assert torch.equal(out[b, :, H:T], out[b + 1, :, 0:O]), b
    shared = torch.zeros(plan.n, T, dtype=torch.bool)
    shared[:-1, H:] = True
    shared[1:, :O] = True
    assert not shared.all() or O == 16               # (O = T / 2: the middle window has no frame of its own)
    assert torch.equal(out[:, 0][~shared], y[:, 0][~shared])
    assert not torch.equal(out[:, 0][shared], y[:, 0][shared])


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("O", OS)
def test_a_constant_prediction_is_unchanged_bit_for_bit(O, mode):
    plan, _ = windows(O)
    for value in (0.1, -3.7, 1e-30, 16777217.0):
        y = torch.full((plan.n, 1, plan.T, 88), value)
        assert torch.equal(BR.blend(y, plan, mode), y), value


@pytest.mark.parametrize("O", OS)
def test_hand_over_takes_the_nearer_window_and_the_lower_one_the_odd_frame(O):
    plan, y = windows(O)
    out = BR.blend(y, plan, 2)
    H, half = plan.stride, (O + 1) // 2
    for b in range(plan.n - 1):
        for j in range(O):
            want = y[b, :, H + j] if j < half else y[b + 1, :, j]
            assert torch.equal(out[b, :, H + j], want) and torch.equal(out[b + 1, :, j], want), (b, j)
    assert {1: 1, 5: 3, 16: 8}[O] == half            # O odd: the lower window takes the middle frame


@pytest.mark.parametrize("O", OS)
def test_linear_weights_are_the_stated_expression(O):
    plan, y = windows(O)
    out = BR.blend(y, plan, 1)
    H = plan.stride
    for j in range(O):
        wu = torch.tensor(j + 1, dtype=torch.float32) / torch.tensor(O + 1, dtype=torch.float32)
        lo, up = y[0, :, H + j], y[1, :, j]
        assert torch.equal(out[0, :, H + j], lo + wu * (up - lo)), j
        assert 0.0 < float(wu) < 1.0
    # the weights of the two windows are mirror images: wu(j) + wu(O - 1 - j) = 1 up to one rounding
    w = [(j + 1) / (O + 1) for j in range(O)]
    assert all(abs(w[j] + w[O - 1 - j] - 1.0) < 1e-12 for j in range(O))


def test_blend_is_per_recording():
    """break-style batches: windows 0-1 are one recording, window 2 another - nothing blends across the mark."""
    import thresh_ref as TR
    O, T = 5, 32
    y = torch.randn(3, 1, T, 88, generator=torch.Generator().manual_seed(4))
    for mode in (0, 1, 2):
        out = BR.blend_groups(y, TR.window_groups(3, O, marks=(2,)), T - O, O, mode)
        assert torch.equal(out[2], y[2]) and torch.equal(out[1, :, T - O:], y[1, :, T - O:])
        assert torch.equal(out[0, :, T - O:], out[1, :, :O]) and not torch.equal(out[0, :, T - O:], y[0, :, T - O:])


# ---------------------------------------------------------------------------------------------- 2. the GPU cases move
@pytest.mark.parametrize("mode", BC.MODES)
@pytest.mark.parametrize("O", BC.OS)
def test_gpu_cases_move_the_roll_beyond_the_parity_bound(O, mode):
    """A parity test cannot pass by ignoring the option: the references of modes 1 and 2 lie further from mode 0's than the
    bound.  The one exception is by definition: at O = 1 the cross-fade's only weight is (float)1 / (float)2 = 0.5, so mode 1
    IS the mean up to the rounding of lo + 0.5 (up - lo) against 0.5 (lo + up) - asserted as such."""
    base, ref = BC.reference(O, 0), BC.reference(O, mode)
    d = float((ref - base).abs().max())
    print(f"\nO {O} mode {mode}: max |roll - mean's roll| {d:.3e}")
    if (O, mode) == (1, 1):
        assert d < ATOL
    else:
        assert d > 100 * ATOL, d
    # mode 0 of the wrapped chain is chain_ref's own window chain
    hp, p, plan, _, x_T, noise, spec = BC.case(O)
    x = BC.windows_of(x_T.reshape(plan.T_c, 88), plan)
    z = BC.windows_of(noise.reshape(-1, plan.T_c, 88), plan)
    assert torch.equal(base, CR.sample_chain(p, hp, BC.SAMPLER, x, spec, z, 0, w=BC.W, plan=plan))


@pytest.mark.parametrize("mode", BC.MODES)
def test_gpu_option_and_fused_cases_move_the_roll(mode):
    import thresh_ref as TR
    for name in BC.OPTION_CASES:
        d = float((BC.option_reference(name, mode) - BC.option_reference(name, 0)).abs().max())
        assert d > 100 * ATOL, (name, d)
    assert float((BC.break_reference(mode) - BC.break_reference(0)).abs().max()) > 100 * ATOL
    roll, stats, r = BC.thresh_reference(mode)
    assert len(stats) == 4 and all(TR.active(stats, r))          # the inputs threshold at every step
    assert float((roll - BC.thresh_reference(0)[0]).abs().max()) > 100 * ATOL
    assert float((BC.fused_reference(mode) - BC.fused_reference(0)).abs().max()) > 100 * ATOL


# ---------------------------------------------------------------------------------------------- 3. façade and CLI
def test_check_window_blend():
    for value, want in ((None, 0), ("mean", 0), ("linear", 1), ("nearest", 2), (0, 0), (1, 1), (2, 2)):
        assert longform.check_window_blend(value) == want
    for bad in (3, -1, "cosine", "Linear", 1.0, True, False, [1], ""):
        with pytest.raises(ValueError, match="window blend"):
            longform.check_window_blend(bad)


def test_cli_key():
    base = ["task=transcription", "dataset=Custom", "dataset.args.max_segment_samples=null"]
    assert cli.build_config(base)["task"].get("window_blend") is None
    for text, want in (("linear", 1), ("nearest", 2), ("mean", 0), ("2", 2), ("null", 0)):
        cfg = cli.build_config(base + [f"task.window_blend={text}"])
        assert longform.check_window_blend(cfg["task"]["window_blend"]) == want
    for bad in ("cosine", "3", "-1", "true", "1.5"):
        with pytest.raises(SystemExit, match=r"task\.window_blend"):
            cli.build_config(base + [f"task.window_blend={bad}"])


def test_facade_holds_the_option_for_the_call():
    """sample_long / sample_long_batch(blend=) validate first and hold "window_blend" beside "window_overlap"."""
    import inspect
    from diffroll_amd.model import ClassifierFreeDiffRoll as M
    for fn in (M.sample_long, M.sample_long_batch):
        assert inspect.signature(fn).parameters["blend"].default is None
    src = inspect.getsource(M._sample_windows)
    assert re.search(r"eng\.holding\(window_overlap=[^)]*?window_blend=blend", src, re.S)
    for fn in (M.sample_long, M.sample_long_batch):
        assert "check_window_blend(blend)" in inspect.getsource(fn)


# ---------------------------------------------------------------------------------------------- 4. the documents
def test_option_is_public_and_documented():
    from diffroll_amd import _cabi
    from diffroll_amd.engine import _MIRRORED, Engine
    assert "window_blend" in _cabi.PUBLIC_OPTIONS
    assert _MIRRORED["window_blend"] == 0 and Engine.window_blend == 0
    assert "'window_blend'" in Engine.set_option.__doc__ and "'window_blend'" in Engine.holding.__doc__
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    begin = re.search(r'"window_blend"\s+\[0\]', doc)
    assert begin
    flat = re.sub(r"\s*\n \*\s*", " ", doc[begin.start():doc.index('"sampling_steps"   [0]')])      # the entry as running text
    for word in ("0.5f * (y_lo + y_up)", "(float)(j + 1) / (float)(O + 1)", "y_lo + wu * (y_up - y_lo)", "j < (O + 1) / 2 ? y_lo : y_up",
                 "lower first", "bit-identical", '"x0_clip"', '"x0_threshold"', '"solver_order"', '"window_break"', '"draws"',
                 "DR_EINVAL", "captured chain's key", "profiles/blend_sweep.txt", "INTEGRATION.md 3b"):
        assert word in flat, word
    for doc_name, words in (("README.md", ("window_blend", "profiles/blend_sweep.txt", "profiles/blend_kernel_resources.txt")),
                            ("INTEGRATION.md", ('"window_blend"', "task.window_blend")), ("DESIGN.md", ('"window_blend"',))):
        body = open(os.path.join(ROOT, doc_name)).read()
        for word in words:
            assert word in body, (doc_name, word)
    for record in ("blend_kernel_resources.txt", "blend_sweep.txt"):
        assert os.path.exists(os.path.join(ROOT, "profiles", record)), record
    if os.path.exists(_cabi.LIB_PATH):               # (built: a load failure is a failure, not a skip)
        assert _cabi.load_library().dr_set_option(None, b"window_blend", 1) == _cabi.DR_EINVAL      # a null handle, never a crash


def test_abi_stays_at_11_and_30_functions():
    from diffroll_amd import _cabi
    assert _cabi.DR_ABI_VERSION == 11
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", text).group(1)) == 11
    assert len(header_functions()) == 30 and len(_cabi.EXPORTS) == 30


def test_the_blend_is_written_once():
    """update_quad and pred_quad call one blend_quad, lower window first; the kernel units name no mode themselves."""
    csrc = os.path.join(ROOT, "diffroll_amd", "csrc")
    quad = open(os.path.join(csrc, "update_quad.h")).read()
    body = quad[quad.index("DR_DEVINL void blend_quad("):quad.index("// pred (optional)")]
    assert "(float)(j + 1) / (float)(O + 1)" in body and "lo[e] + wu * (up[e] - lo[e])" in body
    assert "j < (O + 1) / 2" in body and "0.5f * (lo[e] + up[e])" in body and "#pragma clang fp contract(off)" in body
    thr = open(os.path.join(csrc, "threshold_quad.h")).read()
    for src, y in ((quad, "x0"), (thr, "y")):
        assert f"blend_quad(win_blend(a), f - win_H(a), (int)(o4 / 22), {y}, yp, {y})" in src
        assert f"blend_quad(win_blend(a), f, (int)(o4 / 22), yp, {y}, {y})" in src
    for unit in ("update.hip", "tail.hip", "threshold.hip"):
        assert "blend_quad" not in open(os.path.join(csrc, unit)).read(), unit
