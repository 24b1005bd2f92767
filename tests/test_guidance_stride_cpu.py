"""Option "guidance_stride" without a GPU: the refresh rule against tables written out by hand (tests/stride_ref.py and, through
a compiled stand-alone harness, stride_step / guided_ordinal of csrc/chain_tables.h), the planner's shapes of refresh and reuse
steps (csrc/launch_plan.h), the restated chains the GPU tests compare with (tests/stride_cases.py) shown to reuse - and to be
closer to the guided chain than the chain that drops guidance at the same steps - the Python surface - validator, facade,
checkpoint override, CLI - the documents, the built library and the structural facts of the new kernel's text."""
import os
import re
import shutil
import struct
import subprocess

import pytest
import torch

from testlib import ATOL, S

import chain_ref as CR
import stride_cases as SC
import stride_ref as SR
from facade_fakes import clip, facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V20 = [199, 189, 178, 168, 157, 147, 136, 126, 115, 105, 94, 84, 73, 63, 52, 42, 31, 21, 10, 0]
# the steps that refresh, written out by hand: 20 visited steps, every one guided
REFRESH_20 = {2: [199, 178, 157, 136, 115, 94, 73, 52, 31, 10, 0],      # k = 0, 2, .., 18 and step 0 (k = 19)
              3: [199, 168, 136, 105, 73, 42, 10, 0],                   # k = 0, 3, .., 18 and step 0
              4: [199, 157, 115, 73, 31, 0],                            # k = 0, 4, .., 16 and step 0
              64: [199, 0]}                                             # k = 0 and step 0
# ... 200 steps (t = 199 - k): how many refresh, and the evaluations of one roll's chain
REFRESH_200 = {2: (101, 301), 3: (68, 268), 4: (51, 251), 64: (5, 205)}
# ... under the interval [60, 140] (guided: 136 .. 63, k = 0 .. 7; step 0 does not guide), and from a start step
REFRESH_INTERVAL = {2: [136, 115, 94, 73], 3: [136, 105, 73], 4: [136, 94], 64: [136]}
REFRESH_START_168 = {2: [168, 147, 126, 105, 84, 63, 42, 21, 0], 3: [168, 136, 105, 73, 42, 10, 0], 4: [168, 126, 84, 42, 0], 64: [168, 0]}
REFRESH_START_105_INTERVAL = {2: [105, 84, 63], 3: [105, 73], 4: [105, 63], 64: [105]}


# ---------------------------------------------------------------------------------------------- 1. the refresh rule
def refreshing(sched):
    return [t for t, what in sched if what == "refresh"]


@pytest.mark.parametrize("n", [2, 3, 4, 64])
def test_refresh_rule_matches_the_tables(n):
    assert CR.visited(S, 20) == V20
    sched = SR.schedule(V20, n, S)
    assert refreshing(sched) == REFRESH_20[n] and all(what != "unguided" for _, what in sched)
    assert sched[0] == (199, "refresh") and sched[-1] == (0, "refresh")          # the first guided step, and step 0
    full = SR.schedule(CR.visited(S, 0), n, S)
    assert (len(refreshing(full)), SR.evaluations(full)) == REFRESH_200[n]
    assert full[0] == (199, "refresh") and full[-1] == (0, "refresh")
    inter = SR.schedule(V20, n, S, interval=(60, 140))
    assert refreshing(inter) == REFRESH_INTERVAL[n]
    assert [t for t, what in inter if what == "unguided"] == [199, 189, 178, 168, 157, 147, 52, 42, 31, 21, 10, 0]
    assert refreshing(SR.schedule(V20, n, S, start=168)) == REFRESH_START_168[n]
    started = SR.schedule(V20, n, S, interval=(60, 140), start=105)
    assert refreshing(started) == REFRESH_START_105_INTERVAL[n] and started[0] == (105, "refresh")
    # off, w = 0 and a sampler that does not guide: nothing reuses
    for off in (SR.schedule(V20, 0, S), SR.schedule(V20, 1, S)):
        assert refreshing(off) == V20
    assert all(what == "unguided" for _, what in SR.schedule(V20, n, S, w=0.0) + SR.schedule(V20, n, S, guiding=False))


def test_evaluation_counts_of_the_issue():
    """A 200-step guided chain: 400 evaluations off, 251 at stride 4 (50 refreshes and the last step's); at stride 2 the rule
    gives 301 - 100 refreshes and the last step's, k = 199."""
    full = CR.visited(S, 0)
    assert SR.evaluations(SR.schedule(full, 0, S)) == 400
    assert SR.evaluations(SR.schedule(full, 2, S)) == 301 and SR.evaluations(SR.schedule(full, 4, S)) == 251


# ---------------------------------------------------------------------------------------------- 2. stride_step and the planner
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
            } else if (cmd == "str") {      // str VALID SAMPLER B T t | SAMPLER B T t START_STEP LO HI W_ZERO N
                dr::StrideKey k;
                dr::GuidanceInterval g;
                int valid = 0, sampler = 0, B = 0, T = 0, t = 0, start = 0, wz = 0, n = 0;
                in >> valid >> k.sampler >> k.B >> k.T >> k.t >> sampler >> B >> T >> t >> start >> g.lo >> g.hi >> wz >> n;
                k.valid = valid != 0;
                const dr::StrideVerdict v = dr::stride_step(k, sampler, B, T, t, steps, start, g, steps.S(), wz != 0, n);
                const int out[3] = {(int)v.what, v.expect, v.k};
                fwrite(out, 4, 3, stdout);
            } else if (cmd == "plan") {     // plan NB n_cond B LO HI W_ZERO t next_t REUSE_NOW REUSE_NEXT (-1 -1: the defaults)
                dr::GuidanceInterval g;
                int NB = 0, nc = 0, B = 0, wz = 0, t = 0, nt = 0, rn = 0, rx = 0;
                in >> NB >> nc >> B >> g.lo >> g.hi >> wz >> t >> nt >> rn >> rx;
                const dr::StepShapes p = rn < 0 ? dr::plan_step(NB, nc, B, g, steps.S(), wz != 0, t, nt)
                                                : dr::plan_step(NB, nc, B, g, steps.S(), wz != 0, t, nt, rn != 0, rx != 0);
                const int out[3] = {p.now.NB * 4 + p.now.n_cond * 2 + (int)p.now.dual, p.next.NB * 4 + p.next.n_cond * 2 + (int)p.next.dual,
                                    (int)dr::stride_refreshes(rn, rx, t)};
                fwrite(out, 4, 3, stdout);
            } else return 1;
        }
        return 0;
    }
"""
REFRESHES, REUSES, REFUSED = 0, 1, 2      # dr::StrideStep


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("stride_step")
    src = d / "stride_step_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "stride_step_driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def ask(driver, lines):
    r = subprocess.run([driver], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return [struct.unpack_from("<iii", r.stdout, 12 * i) for i in range(len(r.stdout) // 12)]


def test_stride_rule_of_dr_step(driver):
    key, call, none = "1 1 2 40", "1 2 40", "0 -1 0 0 -1"
    whole, inter = "0 -1 0", "60 140 0"
    cases = [
        # a respaced chain, every step guides, stride 2: the even ordinals and step 0 refresh, whatever is held
        (f"{none} {call} 199 -1 {whole} 2", (REFRESHES, 199, 0)),
        (f"{key} 178 {call} 199 -1 {whole} 2", (REFRESHES, 199, 0)),
        (f"{none} {call} 178 -1 {whole} 2", (REFRESHES, 178, 2)),
        (f"{none} {call} 0 -1 {whole} 2", (REFRESHES, 0, 19)),              # step 0: ordinal 19, refreshes all the same
        (f"{key} 199 {call} 189 -1 {whole} 2", (REUSES, 189, 1)),
        (f"{key} 21 {call} 10 -1 {whole} 3", (REFRESHES, 10, 18)),
        (f"{key} 178 {call} 168 -1 {whole} 2", (REUSES, 168, 3)),
        (f"{key} 199 {call} 168 -1 {whole} 2", (REFUSED, 189, 3)),          # a reuse that skips steps,
        (f"{key} 189 {call} 189 -1 {whole} 2", (REFUSED, 178, 1)),          # repeats its own,
        (f"{none} {call} 189 -1 {whole} 2", (REFUSED, 199, 1)),             # or has no state: the first guided step is expected
        (f"{key} 199 2 2 40 189 -1 {whole} 2", (REFUSED, 199, 1)),          # another sampler,
        (f"{key} 199 1 3 40 189 -1 {whole} 2", (REFUSED, 199, 1)),          # batch
        (f"{key} 199 1 2 41 189 -1 {whole} 2", (REFUSED, 199, 1)),          # or frame count
        (f"{key} 0 {call} 189 -1 {whole} 2", (REFUSED, 199, 1)),            # behind step 0 nothing follows
        # stride 4: three reuses behind a refresh, each following the one before
        (f"{key} 199 {call} 189 -1 {whole} 4", (REUSES, 189, 1)),
        (f"{key} 189 {call} 178 -1 {whole} 4", (REUSES, 178, 2)),
        (f"{key} 178 {call} 168 -1 {whole} 4", (REUSES, 168, 3)),
        (f"{key} 168 {call} 157 -1 {whole} 4", (REFRESHES, 157, 4)),
        (f"{key} 199 {call} 178 -1 {whole} 4", (REFUSED, 189, 2)),
        # off: every guided step refreshes
        (f"{none} {call} 189 -1 {whole} 0", (REFRESHES, 189, 1)),
        (f"{none} {call} 189 -1 {whole} 1", (REFRESHES, 189, 1)),
        # under the interval [60, 140] the ordinals start at the first step inside it
        (f"{none} {call} 136 -1 {inter} 2", (REFRESHES, 136, 0)),
        (f"{key} 136 {call} 126 -1 {inter} 2", (REUSES, 126, 1)),
        (f"{none} {call} 115 -1 {inter} 2", (REFRESHES, 115, 2)),
        (f"{key} 73 {call} 63 -1 {inter} 2", (REUSES, 63, 7)),
        (f"{none} {call} 126 -1 {inter} 2", (REFUSED, 136, 1)),
        (f"{key} 136 {call} 105 -1 {inter} 2", (REFUSED, 126, 3)),
        (f"{key} 63 {call} 52 -1 {inter} 2", (REFUSED, 136, -1)),           # (a caller's error: 52 does not guide)
        # from a start step the ordinals start there
        (f"{none} {call} 168 168 {whole} 2", (REFRESHES, 168, 0)),
        (f"{key} 168 {call} 157 168 {whole} 2", (REUSES, 157, 1)),
        (f"{none} {call} 147 168 {whole} 2", (REFRESHES, 147, 2)),
        (f"{none} {call} 199 168 {whole} 2", (REFUSED, 168, -1)),           # above the start: not this chain's
        (f"{none} {call} 105 105 {inter} 2", (REFRESHES, 105, 0)),
        (f"{key} 105 {call} 94 105 {inter} 2", (REUSES, 94, 1)),
        (f"{none} {call} 136 105 {inter} 2", (REFUSED, 105, -1)),
    ]
    got = ask(driver, ["steps 200 20"] + [f"str {c}" for c, _ in cases])
    assert len(got) == len(cases)
    for (c, want), g in zip(cases, got):
        assert g == want, (c, g)


@pytest.mark.parametrize("n", [2, 3, 4, 64])
def test_the_engines_rule_is_the_tables(driver, n):
    """stride_step over every visited step, the state held at the step before: a refresh where the hand-written table says so,
    a reuse elsewhere - 20 steps whole, under the interval, from a start step; 200 steps counted."""
    key, call = "1 1 2 40", "1 2 40"

    def verdicts(steps, start, interval, table_of_guided):
        lines = [f"str {key} {p} {call} {t} {start} {interval} 0 {n}" for p, t in zip([-1] + table_of_guided[:-1], table_of_guided)]
        return lines

    guided_whole, guided_inter = V20, [t for t in V20 if 60 <= t <= 140]
    guided_start = V20[V20.index(168):]
    lines = ["steps 200 20"] + verdicts(V20, -1, "0 -1", guided_whole) + verdicts(V20, -1, "60 140", guided_inter) + \
        verdicts(V20, 168, "0 -1", guided_start)
    got = ask(driver, lines)
    want = [(t, REFRESH_20[n]) for t in guided_whole] + [(t, REFRESH_INTERVAL[n]) for t in guided_inter] + \
        [(t, REFRESH_START_168[n]) for t in guided_start]
    assert len(got) == len(want)
    for (t, table), g in zip(want, got):
        assert g[0] == (REFRESHES if t in table else REUSES) and g[1] == t, (t, g)
    full = list(range(199, -1, -1))
    got = ask(driver, ["steps 200 0"] + verdicts(full, -1, "0 -1", full))
    assert [g[2] for g in got] == list(range(200)) and sum(g[0] == REFRESHES for g in got) == REFRESH_200[n][0]
    assert all(g[0] in (REFRESHES, REUSES) for g in got)


def test_planner_gives_a_reuse_step_B_evaluations(driver):
    """plan_step (csrc/launch_plan.h): NB = 4, n_cond = 2, B = 2.  A refresh step is the 2 B dual step, a reuse step the B
    conditional one - now and as the successor a tail kernel primes for; the unguided step behind the interval and the old
    eight-argument call are unchanged."""
    dual, cond = 4 * 4 + 2 * 2 + 1, 2 * 4 + 2 * 2
    lines = ["steps 200 20",
             "plan 4 2 2 0 -1 0 199 189 0 1",       # refresh, then reuse
             "plan 4 2 2 0 -1 0 189 178 1 0",       # reuse, then refresh
             "plan 4 2 2 0 -1 0 189 178 1 1",       # reuse, then reuse (stride > 2)
             "plan 4 2 2 0 -1 0 199 189 -1 -1",     # the old call: guided, guided
             "plan 4 2 2 0 -1 0 199 189 0 0",       # ... and the defaults spelled out
             "plan 4 2 2 60 140 0 147 136 0 0",     # the unguided step in front of the interval primes a refresh: the first guided step
             "plan 4 2 2 60 140 0 63 52 1 0",       # the last guided step, a reuse; the unguided step behind the interval
             "plan 4 2 2 60 140 0 52 42 0 0",       # unguided steps keep their shape whatever the flags say ...
             "plan 4 2 2 60 140 0 52 42 1 1",
             "plan 4 2 2 0 -1 1 199 189 1 1",       # ... and so does w = 0
             "plan 2 2 2 0 -1 0 199 189 1 1",       # ... and a sampler that does not guide
             "plan 4 2 2 0 -1 0 0 -1 0 0"]          # the last step: no successor
    got = ask(driver, lines)
    assert [g[:2] for g in got] == [(dual, cond), (cond, dual), (cond, cond), (dual, dual), (dual, dual), (cond, dual), (cond, cond),
                                    (cond, cond), (cond, cond), (cond, cond), (cond, cond), (dual, 0)]
    # stride_refreshes(n, k, t) by the same driver (its last word: n = REUSE_NOW, k = REUSE_NEXT, t)
    rule = ask(driver, [f"plan 4 2 2 0 -1 0 {t} -1 {n} {k}" for n, k, t in ((2, 0, 5), (2, 1, 5), (2, 1, 0), (3, 3, 7), (3, 4, 7), (64, 63, 9),
                                                                            (64, 64, 9), (1, 5, 9), (0, 5, 9))])
    assert [g[2] for g in rule] == [1, 0, 1, 1, 0, 0, 1, 1, 1]


# ---------------------------------------------------------------------------------------------- 3. the chains the GPU tests use
def test_stride_0_and_1_are_chain_refs_chain():
    hp, p, _, x, noise = SC.setup()
    for sampler in ("cfdg_ddpm_x0", "cfdg_ddim_x0"):
        ref = CR.sample_chain(p, hp, sampler, x, SC.spec_of(sampler), noise, SC.N_STEPS, w=SC.W)
        assert torch.equal(SC.reference(sampler, 0)[0], ref)
        assert torch.equal(SR.sample_chain(p, hp, sampler, x, SC.spec_of(sampler), noise, SC.N_STEPS, w=SC.W, guidance_stride=1)[0], ref)
    ref = CR.sample_chain(p, hp, "cfdg_ddpm_x0", x, SC.spec_of("cfdg_ddpm_x0"), noise, SC.N_STEPS, w=SC.W, interval=(60, 140), order=2)
    assert torch.equal(SC.reference("cfdg_ddpm_x0", 0, interval=(60, 140), order=2)[0], ref)


@pytest.mark.parametrize("sampler", SC.GUIDING)
def test_the_cases_bite(sampler):
    """20 steps, stride 2: the strided roll is at least 100 ATOL from the guided chain's, and its rms distance from it is under
    half that of the chain that skips guidance at the reuse steps (measured when the option was designed: 0.23, 0.23, 0.23).
    Strides 3 and 4 and the variant that reuses a stale unconditional prediction are printed as a record only."""
    full = SC.reference(sampler, 0)[0]
    roll = SC.assert_active(sampler, 2)
    skip = SC.reference(sampler, 2, variant="skip")[0]
    d, ds = SC.rms(roll - full), SC.rms(skip - full)
    print(f"\n{sampler} 20 steps stride 2: rms |reuse d - guided| {d:.3e}  |skip - guided| {ds:.3e}  ratio {d / ds:.3f}  (roll rms {SC.rms(full):.3f})")
    for n in (2, 3, 4):
        du = SC.rms(SC.reference(sampler, n, variant="u")[0] - full)
        dn, dsn = SC.rms(SC.reference(sampler, n)[0] - full), SC.rms(SC.reference(sampler, n, variant="skip")[0] - full)
        print(f"  stride {n}: reuse d {dn:.3e}  skip {dsn:.3e}  stale u {du:.3e}")
    assert float((roll - full).abs().max()) >= 100 * ATOL
    assert d < 0.5 * ds, (d, ds)


def test_the_200_step_chain_bites_too():
    """cfdg_ddpm_x0, every step of the 200, stride 2 (measured when the option was designed: ratio 0.05)."""
    full = SC.reference("cfdg_ddpm_x0", 0, n=0)[0]
    roll, sched = SC.reference("cfdg_ddpm_x0", 2, n=0)
    skip = SC.reference("cfdg_ddpm_x0", 2, n=0, variant="skip")[0]
    d, ds = SC.rms(roll - full), SC.rms(skip - full)
    print(f"\ncfdg_ddpm_x0 200 steps stride 2: rms |reuse d - guided| {d:.3e}  |skip - guided| {ds:.3e}  ratio {d / ds:.3f}")
    assert SR.evaluations(sched) == 301
    assert float((roll - full).abs().max()) >= 100 * ATOL and d < 0.5 * ds, (d, ds)


@pytest.mark.parametrize("stride", SC.STRIDES)
@pytest.mark.parametrize("sampler", SC.GUIDING)
def test_gpu_chain_cases_are_active(sampler, stride):
    SC.assert_active(sampler, stride)
    SC.assert_active(sampler, stride, philox=True)


@pytest.mark.parametrize("name,kw,_", SC.OPTION_CASES, ids=[c[0] for c in SC.OPTION_CASES])
def test_gpu_option_cases_are_active(name, kw, _):
    SC.assert_active("cfdg_ddpm_x0", SC.MAIN, **kw)
    sched = SC.reference("cfdg_ddpm_x0", SC.MAIN, **kw)[1]
    if "interval" in kw:                              # the ordinals start at the first step inside the interval
        want = REFRESH_INTERVAL[2] if kw["interval"][0] == 60 else [136, 115, 94, 73, 52, 31, 10, 0]
        assert [t for t, what in sched if what == "refresh"] == want
    if kw.get("start"):
        assert sched[0] == (SC.start_step(), "refresh")


# ---------------------------------------------------------------------------------------------- 4. the Python surface
def test_check_guidance_stride():
    from diffroll_amd.schedule import GUIDING_SAMPLERS, STRIDE_PARTNERS, check_guidance_stride
    for off in (None, 0, 1):
        assert check_guidance_stride(off) == 0 and check_guidance_stride(off, "ddim") == 0
        assert check_guidance_stride(off, "cfdg_ddpm_x0", cfg_rescale=0.7) == 0
    for s in GUIDING_SAMPLERS:
        assert check_guidance_stride(2, s) == 2 and check_guidance_stride(64, s) == 64 and check_guidance_stride(3, s, cfg_rescale=None) == 3
    for bad in (-1, 65, 100, 2.0, 0.5, "2", [2], True, False):
        with pytest.raises(ValueError, match=re.escape("guidance_stride must be") + ".*" + re.escape(repr(bad))):
            check_guidance_stride(bad, "cfdg_ddpm_x0")
    for s in ("ddpm_x0", "generation_ddpm_x0", "ddim_x0", "ddpm", "ddim", "ddim2ddpm"):
        with pytest.raises(ValueError, match=r"guidance_stride = 2 needs a sampler that guides"):
            check_guidance_stride(2, s)
    assert STRIDE_PARTNERS == ("x0_threshold", "cfg_rescale", "cfg_project", "cfg_norm", "cfg_momentum")
    for other, theirs in (("x0_threshold", 0.995), ("cfg_rescale", 0.7), ("cfg_project", 1.0), ("cfg_norm", 0.05), ("cfg_momentum", -0.5)):
        with pytest.raises(ValueError, match=f"guidance_stride = 2 does not combine with {other} = {theirs!r}"):
            check_guidance_stride(2, "cfdg_ddpm_x0", **{other: theirs})
        assert check_guidance_stride(2, "cfdg_ddpm_x0", **{other: None}) == 2 and check_guidance_stride(2, "cfdg_ddpm_x0", **{other: 0}) == 2


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
    assert m.guidance_stride() == 0
    m = _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "guidance_stride": 2})
    assert m.guidance_stride() == 2 and m.sampling_options()["guidance_stride"] == 2
    m.hparams.sampling.guidance_stride = None         # read at every use
    assert m.guidance_stride() == 0
    m.hparams.sampling.guidance_stride = 1            # 1 is off
    assert m.guidance_stride() == 0
    m.hparams.sampling.guidance_stride = 4
    m.__dict__["_stride1"] = True                     # one of the reference's single-step methods is running
    assert m.guidance_stride() == 0
    m.__dict__["_stride1"] = False
    assert m.guidance_stride() == 4
    m.hparams.sampling.guidance_stride = 65           # refused at use, before the engine is reached
    with pytest.raises(ValueError, match="guidance_stride must be"):
        m.engine
    with pytest.raises(ValueError, match="guidance_stride must be"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    m.hparams.sampling.guidance_stride = 2
    for key, value in (("cfg_rescale", 0.7), ("cfg_project", 1.0), ("cfg_norm", 0.05)):
        setattr(m.hparams.sampling, key, value)
        with pytest.raises(ValueError, match=f"guidance_stride = 2 does not combine with {key} = {value!r}"):
            m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
        setattr(m.hparams.sampling, key, None)
    m.hparams.sampling.cfg_project, m.hparams.sampling.cfg_momentum = 1.0, -0.5
    with pytest.raises(ValueError, match="guidance_stride = 2 does not combine with cfg_project = 1.0"):
        m.engine
    m.hparams.sampling.cfg_project, m.hparams.sampling.cfg_momentum = None, None
    m.hparams.sampling.x0_clip = 1
    assert m.guidance_stride() == 2                   # (the clamp combines)
    m.hparams.sampling.x0_threshold = 0.995
    with pytest.raises(ValueError, match="guidance_stride = 2 does not combine with x0_threshold = 0.995"):
        m.sample(torch.zeros(1, 1, 8, 88), torch.zeros(1, 4096))
    m.hparams.sampling.x0_threshold = None
    m.hparams.sampling.update(guidance_interval=[60, 140], solver_order=2, solver_noise=1, steps=20, strength=0.5, draws=2)
    assert m.guidance_stride() == 2                   # (everything else combines)
    for bad in (65, -1, "2", 2.0, True):
        with pytest.raises(ValueError, match="guidance_stride must be"):
            _model(sampling={"type": "cfdg_ddpm_x0", "w": 0.5, "guidance_stride": bad})
    with pytest.raises(ValueError, match="needs a sampler that guides"):
        _model(sampling={"type": "ddpm_x0", "guidance_stride": 2})
    with pytest.raises(ValueError, match="does not combine with cfg_rescale"):
        _model(sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "guidance_stride": 2, "cfg_rescale": 0.7})
    assert "guidance_stride" in type(m).sample.__doc__


def test_the_option_is_set_once_and_not_again_across_calls():
    """The facade on the recording engine (tests/facade_fakes.py): the first call sets the option, later calls with the same
    hparams set nothing, a change of the key sets the new value once, None sets 0."""
    m, eng = facade("cfdg_ddpm_x0")
    wav, x, _, z = clip(2, 8)
    m.hparams.sampling.guidance_stride = 2
    m.sample(x, wav, noise=z)
    first = eng.talk()
    assert [c for c in first if c[0] == "set_option"] == [("set_option", "guidance_stride", 2)] and eng.guidance_stride == 2
    assert first.index(("set_option", "guidance_stride", 2)) < [c[0] for c in first].index("sample")      # in front of the chain
    m.sample(x, wav, noise=z)
    m.sample(x, wav, seed=3)
    assert not [c for c in eng.talk() if c[0] == "set_option"]
    m.hparams.sampling.guidance_stride = 4
    m.sample(x, wav, noise=z)
    assert [c for c in eng.talk() if c[0] == "set_option"] == [("set_option", "guidance_stride", 4)]
    m.hparams.sampling.guidance_stride = None
    m.sample(x, wav, noise=z)
    assert [c for c in eng.talk() if c[0] == "set_option"] == [("set_option", "guidance_stride", 0)]
    m.hparams.sampling.guidance_stride = 1            # 1 is 0 to the engine: nothing is set
    m.sample(x, wav, noise=z)
    assert not [c for c in eng.talk() if c[0] == "set_option"]
    plain, eng2 = facade("cfdg_ddpm_x0")
    plain.sample(x, wav, noise=z)
    assert not [c for c in eng2.talk() if c[0] == "set_option" and c[1] == "guidance_stride"]


def test_load_from_checkpoint_override(golden_dir):
    from diffroll_amd import ClassifierFreeDiffRoll
    path = os.path.join(golden_dir, "trained_small.ckpt")
    got = ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "guidance_stride": 2})
    assert got.guidance_stride() == 2
    assert ClassifierFreeDiffRoll.load_from_checkpoint(path).guidance_stride() == 0
    with pytest.raises(ValueError, match="guidance_stride must be"):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "guidance_stride": 65})
    with pytest.raises(ValueError, match="guidance_stride = 2 does not combine with cfg_project"):
        ClassifierFreeDiffRoll.load_from_checkpoint(path, sampling={"type": "cfdg_ddpm_x0", "w": 3.0, "cfg_project": 1.0, "guidance_stride": 2})


def test_cli():
    from diffroll_amd import cli
    cfg = cli.build_config(["task=transcription", "task.sampling.w=3", "task.sampling.guidance_stride=2"])
    assert cfg["task"]["sampling"] == {"type": "cfdg_ddpm_x0", "w": 3, "guidance_stride": 2}
    assert "guidance_stride" not in cli.build_config(["task=transcription"])["task"]["sampling"]
    assert cli.build_config(["task=transcription", "task.sampling.guidance_stride=null"])["task"]["sampling"]["guidance_stride"] is None
    assert cli.build_config(["task=inpainting", "task.sampling.guidance_stride=4", "task.sampling.steps=50"])["task"]["sampling"]["guidance_stride"] == 4
    for bad in ("65", "-1", "2.5", "two"):
        with pytest.raises(SystemExit, match="task.sampling.guidance_stride"):
            cli.build_config(["task=transcription", f"task.sampling.guidance_stride={bad}"])
    with pytest.raises(SystemExit, match="task.sampling.guidance_stride.*needs a sampler that guides"):
        cli.build_config(["task=transcription", "task.sampling.type=ddim", "task.sampling.guidance_stride=2"])
    with pytest.raises(SystemExit, match="task.sampling.guidance_stride.*does not combine with cfg_rescale"):
        cli.build_config(["task=transcription", "task.sampling.guidance_stride=2", "task.sampling.cfg_rescale=0.7"])
    with pytest.raises(SystemExit, match="task.sampling.guidance_stride.*does not combine with cfg_norm"):
        cli.build_config(["task=transcription", "task.sampling.guidance_stride=2", "task.sampling.cfg_norm=0.05"])


# ---------------------------------------------------------------------------------------------- 5. the documents
def test_option_is_public_and_documented():
    from diffroll_amd import _cabi
    from diffroll_amd.engine import _MIRRORED, Engine
    from testlib import header_functions
    name = "guidance_stride"
    assert name in _cabi.PUBLIC_OPTIONS and _MIRRORED[name] == 0 and getattr(Engine, name) == 0
    assert f"'{name}'" in Engine.set_option.__doc__ and f"'{name}'" in Engine.holding.__doc__
    assert _cabi.DR_ABI_VERSION == 11 and len(_cabi.PRECISIONS) == 4
    text = open(os.path.join(ROOT, "include", "diffroll_amd.h")).read()
    assert int(re.search(r"#define DR_ABI_VERSION (\d+)", text).group(1)) == 11
    assert len(header_functions()) == len(_cabi.EXPORTS) == 30
    doc = text[text.index('"fused_stack"'):text.index("int dr_set_option(")]
    begin = re.search(r'"guidance_stride"\s+\[0\]', doc)
    assert begin
    flat = re.sub(r"\s*\n \*\s*", " ", doc[begin.start():doc.index("Unknown names")])
    for word in ("0 or 1 (off), or 2 .. 64", "Lv et al. 2024", "Castillo et al. 2023", "k % n == 0 or when it is step t == 0",
                 "always refreshes", "d = y - c", "y = c + d", "no contraction", "one rounding", "written by the element's own thread",
                 "bit for bit, the roll of the same step with the option off", "B evaluations", 'the clamp of "x0_clip"',
                 "the solver's extrapolation and its history", "the last step", "CARRIES THE WEIGHT", "never each other's state",
                 "one state per roll", "no memset, no host help, every replay restarts by itself", "csrc/stride.hip",
                 "DR_MODE_FUSED_STACK", "keep the tail kernel and every bit", "DR_ESTATE naming the step expected next", "dr_sample",
                 'a change of "guidance_stride" itself', '"x0_threshold", "cfg_rescale", "cfg_project", "cfg_norm" or "cfg_momentum"',
                 "a sampler that does not guide", "naming the two options", "stating the range", "captured chain's key",
                 "0 and 1 are one value", "byte-identical", "Nothing is known about quality", "INTEGRATION.md 3c"):
        assert word in flat, word
    for doc_name, words in (("README.md", ("guidance_stride", "profiles/stride_sweep.txt", "profiles/stride_kernel_resources.txt",
                                           "profiles/stride_margins.txt", "Nothing is known about quality")),
                            ("INTEGRATION.md", ('"guidance_stride"', "task.sampling.guidance_stride=2")),
                            ("DESIGN_HISTORY.md", ("guidance_stride",))):
        body = open(os.path.join(ROOT, doc_name)).read()
        for word in words:
            assert word in body, (doc_name, word)
    abi = open(os.path.join(ROOT, "diffroll_amd", "csrc", "abi.hip")).read()
    assert '{"guidance_stride", &ChainOptions::guid_stride, 0, 64,' in abi and "stride_step(" in abi      # (its row of the option table)


def test_the_built_library_knows_the_option():
    """Without a GPU no engine exists to set the option on: that it accepts 0, 1, 2 and 64 and refuses -1, 65 and each
    forbidden partner is held on the GPU (tests/test_gpu_guidance_stride.py).  What can be held here: the library carries the
    option's own refusal texts (a library without it has none), and a null handle is DR_EINVAL, never a crash."""
    from diffroll_amd import _cabi
    if not os.path.exists(_cabi.LIB_PATH):
        pytest.skip("the library is not built (python -m diffroll_amd.build)")
    lib = _cabi.load_library()                        # (built: a load failure is a failure, not a skip)
    blob = open(_cabi.LIB_PATH, "rb").read()
    for text in (b"guidance_stride is 0 or 1 (off) or the stride n, 2 .. 64", b"guidance_stride = %d does not combine with %s = %d",
                 b"guidance_stride = %d reuses the guidance update of a sampler that guides",
                 b"reuses no stored guidance update - the step expected next is %d"):
        assert text in blob, text
    assert lib.dr_set_option(None, b"guidance_stride", 2) == _cabi.DR_EINVAL
    assert _cabi.DR_ABI_VERSION == 11


def test_the_new_kernels_text_and_the_parents():
    """The stride form is a further instantiation of update_quad and a second argument: UpdateArgs does not grow, tail.hip and
    update.hip learn nothing, contraction is off in the new files, which use no atomic and wait for nobody."""
    csrc = os.path.join(ROOT, "diffroll_amd", "csrc")
    for unit in ("tail.hip", "update.hip", "momentum.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert "guidance_stride" not in text and "StrideUpd" not in text and "stride_quad" not in text, unit
    kern = open(os.path.join(csrc, "kernels.h")).read()
    upd = kern[kern.index("struct UpdateArgs {"):kern.index("// (mode 5) the half the step reads")]
    assert "guidance_stride" not in upd and upd.rstrip().endswith("float clamp_lo, clamp_hi;\n};".rstrip())
    quad = open(os.path.join(csrc, "stride_quad.h")).read()
    hip = open(os.path.join(csrc, "stride.hip")).read()
    assert "struct StrideUpd {" in quad and "float* d;" in quad and "int reuse;" in quad
    assert "DR_DEVINL void form_quad(const UpdateArgs& a, const StrideUpd& su," in quad
    assert quad.count("clamp_quad(") == 1 and "clamp_quad" not in hip and "pred_quad(uc, i4, c)" in quad
    pragma = "#pragma clang fp contract(off)"
    assert hip.index(pragma) < hip.index("__global__") and quad.count(pragma) == quad.count("DR_DEVINL void") == 1
    code = "\n".join(line.split("//")[0] for line in (hip + quad).splitlines())
    for banned in ("unsafeAtomicAdd", "atomicAdd(", "atomicMax(", "atomicMin(", "while (", "__builtin_amdgcn_s_sleep", "fmaf("):
        assert banned not in code, banned
    assert re.search(r"void update_stride_kernel\(const UpdateArgs a, const StrideUpd su\) \{[^}]*update_quad\(a, i4, &y, su\)", code)
    plan = open(os.path.join(csrc, "plan.hip")).read()
    assert "launch_update_stride(u, StrideUpd{e->stride_d, reuse ? 1 : 0}, st)" in plan and "!stage.stride" in plan
    from diffroll_amd import build
    assert "stride.hip" in build.SOURCES and any(h.endswith("stride_quad.h") for h in build.HEADERS)
