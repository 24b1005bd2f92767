"""Everything that makes dr_sample's captured chain stale, on one engine: after each event the captured path must compute what
the eager path computes under the new state - a chain captured under the old state is not replayed - and after the event
is undone the first roll comes back bit for bit.  The calls are asynchronous (check=False) and nothing waits between them
except the comparisons at the end of each event, so every capture replaces a chain whose last replay is still on the stream.
Geometry and four-step chain of test_gpu_x0_clip.py::test_inert_option_values_replay_the_captured_chain."""
import pytest
import torch

from testlib import make_model

import clip_cases as CC

pytestmark = pytest.mark.gpu

SAMPLER, W = "cfdg_ddpm_x0", 3.0
SWITCHED = ("fused_stack", "fused_tail", "blocked_accumulation", "fused_stack_xcd", "tune.ksplit_max")


def option(name, value, back):
    return (lambda eng: eng.set_option(name, value)), (lambda eng: eng.set_option(name, back))


def events(m, wav, run):
    """(name, apply, undo): apply and undo take the engine; undo None = apply has put everything back itself"""
    wide = torch.cat([wav, wav])

    def other_clip_count(eng):
        eng.frontend(torch.cat([wav, wav[:1]]), CC.TN, return_spec=False)
        eng.frontend(wav, CC.TN, return_spec=False)

    def twice_the_batch(eng):
        eng.frontend(wide, CC.TN, return_spec=False)
        run(2 * CC.B)
        eng.frontend(wav, CC.TN, return_spec=False)

    def commit_again(eng):
        eng.load_params(dict(m.state_dict()))
        eng.frontend(wav, CC.TN, return_spec=False)

    return [
        ("fused_stack-0",) + option("fused_stack", 0, 1),
        ("fused_stack-2",) + option("fused_stack", 2, 1),
        ("fused_tail-0",) + option("fused_tail", 0, 1),
        ("blocked_accumulation-1",) + option("blocked_accumulation", 1, 2),
        ("fused_stack_xcd-0",) + option("fused_stack_xcd", 0, 1),
        ("tune.ksplit_max-1",) + option("tune.ksplit_max", 1, 16),
        ("precision-bf16x3", lambda eng: eng.set_precision("bf16x3"), lambda eng: eng.set_precision("f32")),
        ("frontend-one-clip-more", other_clip_count, None),
        ("twice-the-batch", twice_the_batch, None),
        ("commit-again", commit_again, None),
    ]


def test_every_staleness_event_captures_again_and_undone_replays_the_first_roll():
    from tools import tuning_env
    if any(tuning_env.is_forced(k) for k in SWITCHED):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp, p, wav, x, _, _ = CC.setup()
    m = make_model(hp, p, sampler=SAMPLER, w=W)
    m.hparams.sampling.steps = 4
    eng = m.engine
    eng.frontend(wav, CC.TN, return_spec=False)
    x_T = x.squeeze(1).to(eng.device).contiguous()

    def run(B=CC.B, use_graph=True):
        x_in = x_T.repeat(B // CC.B, 1, 1).contiguous()
        return eng.sample(SAMPLER, x_in, None, w=W, seed=CC.PHILOX_SEED, use_graph=use_graph, check=False)

    def counts():      # every capture issues launches that one of these counts (captured launches count once, at capture)
        st = eng.launch_state()
        return eng.launch_counts() + (st["stack_launches"], st["tail_launches"])

    c0 = counts()
    first = run()
    assert counts() != c0                             # (the capture was counted: the counters see this chain)
    c1 = counts()
    assert torch.equal(run(), first) and counts() == c1      # ... and a replay is not
    try:
        for name, apply, undo in events(m, wav, run):
            apply(eng)
            before = counts()
            captured, after = run(), counts()
            eager = run(use_graph=False)
            if undo:
                undo(eng)
            back = run()
            assert torch.equal(captured, eager), name
            assert after != before, (name, before)
            assert torch.equal(back, first), name
            eng.finish()
    finally:
        eng.set_option("tune.ksplit_max", 16)         # (process-wide)
