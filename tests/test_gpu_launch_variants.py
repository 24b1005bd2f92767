"""Launch variants that only a shape threshold or an A/B knob reaches, each forced (tests/variant_cases.py: the table, which
tests/test_launch_variants_cpu.py proves reaches what it claims) and held to a twin that must give the same bits, and to the
oracle: the block -> XCD mapping of the per-phase GEMM launches (A), the one-chain 1x1 GEMMs across kernels and channels per
hand-over (B), pwk_kernel<1> against <2> (C), the tail kernel's 64- / 96-frame items (D), every split-K factor (E).  The
twins differ only in which block computes which tile, or in how one fp32 chain is cut into hand-overs - never in the order of
a sum - so every comparison between them is torch.equal; the tolerances against the oracle are those of tests/testlib.py."""
import pytest
import torch

from testlib import ATOL_FWD, ATOL_STEP, make_model, maxdiff
from tuning_pins import pinned

import variant_cases as V

pytestmark = pytest.mark.gpu


def skip_if_forced(cases, *options):
    from tools import tuning_env
    knobs = {k for c in cases for ps in V.pin_sets(c) for k in ps.pins} | {"fused_stack", "blocked_accumulation"} | set(options)
    if any(tuning_env.is_forced(k) for k in knobs):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")


def model_of(c):
    return make_model(V.hp_of(c), V.params(c), sampler=c.sampler, w=V.W, precision=c.precision)


def evaluate(m, c):
    """one forward() and one reverse step"""
    wav, x, z, t, _ = V.inputs(c)
    out, _ = m(x, wav, t)
    step, _ = m.reverse_diffusion(x, wav, V.STEP_T, noise=z)
    return out.cpu(), step.cpu()


def per_phase(m, c, pins):
    with pinned(m.engine, V.with_defaults(pins)):
        m.engine.set_option("fused_stack", 0)
        return evaluate(m, c)


def same_bits(a, b, what, names=("forward", "step")):
    for name, u, v in zip(names, a, b):
        assert torch.equal(u, v), (*what, name, "max |difference| = %.3e" % maxdiff(u, v))


def near_oracle(got, c, what):
    ref = V.reference(c)
    d = [maxdiff(g, r) for g, r in zip(got, ref)]
    print(*what, "vs oracle:", " ".join("%.2e" % v for v in d))
    assert d[0] <= ATOL_FWD, (*what, "forward", d[0])
    assert d[1] <= ATOL_STEP, (*what, "step", d[1])


MAPPINGS = (("xcd_n=1", {"tune.xcd_n": 1}), ("xcd_model=0", {"tune.xcd_model": 0}), ("traffic model", {}))


@pytest.mark.parametrize("c", V.CASES_A, ids=V.case_id)
def test_xcd_mapping_twins(c):
    """A: under every pin set, mapping 1 (tune.xcd_n = 1: the M tiles of a frame tile on one XCD; with split-K the K slices
    too) = mapping 0, as are the two rules that choose between them; mapping 0 is within the tolerances of the oracle"""
    skip_if_forced([c], "tune.xcd_n", "tune.xcd_model")
    m = model_of(c)
    for ps in V.pin_sets(c):
        base = per_phase(m, c, dict(ps.pins, **{"tune.xcd_n": 0}))
        for label, extra in MAPPINGS:
            same_bits(per_phase(m, c, dict(ps.pins, **extra)), base, (c.name, ps.label, label))
        near_oracle(base, c, (c.name, ps.label))


@pytest.mark.parametrize("c", V.CASES_B, ids=V.case_id)
def test_one_chain_pointwise_twins(c):
    """B: the 1x1 residual / skip GEMM keeps one k-ordered chain per output in pw_kernel (64 .. 160-frame blocks) and in the
    LDS-staged gemm_kernel (64- / 128-frame blocks, 32 / 64 / 128 channels per hand-over - tune.one_ks = 4 on 128-frame
    blocks falls back to 64): all the same bits"""
    skip_if_forced([c])
    m = model_of(c)
    sets = V.pin_sets(c)
    base = per_phase(m, c, sets[0].pins)
    for ps in sets[1:]:
        same_bits(per_phase(m, c, ps.pins), base, (c.name, ps.label, "against " + sets[0].label))
    near_oracle(base, c, (c.name, sets[0].label))


@pytest.mark.parametrize("channels", sorted({c.C for c in V.CASES_C}))
def test_pwk_kernel_widths_are_twins(channels):
    """C: pwk_kernel<1> = pwk_kernel<2> (the same per-wave K quarter, ((p0 + p1) + p2) + p3) with 1 / 2 / 3 K slabs per wave,
    from one frame to four ragged 32-frame tiles, in the full launch and the last layer's skip half; forward() with per-sample
    steps (the epilogue's row selection) and a guided step, each within the tolerances of the oracle"""
    cases = [c for c in V.CASES_C if c.C == channels]
    skip_if_forced(cases)
    m = model_of(cases[0])
    for c in cases:
        one, two = (per_phase(m, c, ps.pins) for ps in V.pin_sets(c))
        same_bits(two, one, (c.name, "pwk_kernel<2> against <1>"))
        near_oracle(one, c, (c.name, "pwk_kernel<1>"))
        near_oracle(two, c, (c.name, "pwk_kernel<2>"))


@pytest.mark.parametrize("c", V.CASES_D, ids=V.case_id)
def test_tail_item_width_twins(c):
    """D: a 3-step guided chain on the fused stack with the tail kernel's next-step first-layer conv on 64-frame items, on
    96-frame items, without the tail kernel, and on per-phase launches of the same flavours: the same roll, bit for bit"""
    skip_if_forced([c], "fused_tail")
    m = model_of(c)
    eng = m.engine
    wav, x, _, _, noise = V.inputs(c)
    t4_1, t4_3 = V.pin_sets(c)
    twin = {k: v for k, v in t4_1.pins.items() if k != "tune.tail_t4"}
    rolls = []
    for label, pins, stack, tail in ((t4_1.label, t4_1.pins, 2, 1), (t4_3.label, t4_3.pins, 2, 1), ("fused_tail=0", twin, 2, 0),
                                     ("per-phase", twin, 0, 1)):
        with pinned(eng, V.with_defaults(pins), restore=("fused_stack", "fused_tail")):
            eng.set_option("fused_stack", stack)
            eng.set_option("fused_tail", tail)
            eng.stack_status()
            t0, s0 = eng.tail_launches, eng.stack_launches
            roll = m.sample(x, wav, noise=noise)[0].cpu()
            assert eng.stack_status()[0] == 0, (c.name, label, "a group barrier timed out")
            assert (eng.tail_launches > t0) == (stack == 2 and tail == 1), (c.name, label, eng.tail_launches - t0)
            assert (eng.stack_launches > s0) == (stack == 2), (c.name, label)
        rolls.append((label, roll))
    for label, roll in rolls[1:]:
        same_bits((roll,), (rolls[0][1],), (c.name, label, "against " + rolls[0][0]), names=("chain",))
    d = maxdiff(rolls[0][1], V.reference(c)[0])
    print(c.name, "chain vs oracle: %.2e" % d)
    assert d <= ATOL_STEP, (c.name, d)


@pytest.mark.parametrize("c", V.CASES_E, ids=V.case_id)
def test_split_k_factors(c):
    """E: the conv cut 2 / 4 / 8 / 16 times in K (and 4 times by the tune.ksplit_blocks cap): each factor within the tolerances of
    the oracle - a slice that is consistently wrong repeats perfectly - and repeatable bit for bit"""
    skip_if_forced([c])
    m = model_of(c)
    for ps in V.pin_sets(c):
        first = per_phase(m, c, ps.pins)
        same_bits(per_phase(m, c, ps.pins), first, (c.name, ps.label, "second run"))
        near_oracle(first, c, (c.name, ps.label))
