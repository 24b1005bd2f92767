"""The fused residual-stack kernel (one persistent launch for all residual layers, group barriers between the
phases) against one launch per phase: same device code, same MFMA order, same epilogue arithmetic, so the
results must be BIT-IDENTICAL - any stale read across workgroups (the hazard of an in-launch hand-off) would show
as a difference.  Both are separately held to the oracle by tests/test_gpu_parity.py; here the fused path is
forced (fused_stack = 2) over launch geometries it would not be chosen for, so ragged tiles, multi-tile clips
(halo exchange inside a group), tiles straddling the residual / skip halves (C = 64, 192), per-sample steps and
both block mappings are covered."""
import os

import numpy as np
import pytest
import torch

from oracle import diffroll_ref as R
from testlib import make_model

pytestmark = pytest.mark.gpu


def _run_both(m, fn, xcds=(1, 0)):
    eng = m.engine
    eng.set_option("fused_stack", 0)
    ref = fn()
    outs = []
    for xcd in xcds:
        eng.set_option("fused_stack", 2)
        eng.set_option("fused_stack_xcd", xcd)
        eng.stack_status()
        n0 = eng.stack_launches
        out = fn()
        flag, _ = eng.stack_status()
        assert flag == 0, "a group barrier of the fused kernel timed out"
        outs.append((xcd, out, eng.stack_launches - n0))
    eng.set_option("fused_stack", 1)
    eng.set_option("fused_stack_xcd", 1)
    return ref, outs


@pytest.mark.parametrize("ni", ["1", "2", "2b", "5b", "1s", "2s", "2sb"])
def test_fused_stack_is_bit_identical_to_per_phase_launches(ni):
    """All cases of tests/fused_cases.py for one block flavour, in a child process whose per-phase kernels are
    pinned to the flavours the fused kernel is built from (tune.* options, tools/tuning_env.py).  "2b" = the
    128-frame flavour with blocked accumulation requested (option blocked_accumulation = 2: other instantiations); "5b" = the
    160-frame flavour of the 640-frame geometries (blocked accumulation only; per-phase twin: gemm_kernel<5> + pw_kernel<5>);
    "1s" / "2s" / "2sb" = the split-bf16 flavours (precision="bf16x3": S3 hand-offs, LDS-staged 1x1 phases, no tail
    kernel; "2sb": 128-frame blocks with blocked accumulation)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    blocked = "b" in ni
    s3 = "s" in ni
    ni = int(ni[0])
    from tools import tuning_env
    env = tuning_env.env_with(tune__ksplit_max=1, tune__tile=3200 + ni, tune__pw_nw=5 if ni == 5 else 2 * ni, tune__stack_fl=ni,
                              blocked_accumulation=2 if blocked else 1)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "fused_cases.py"), str(ni)] + (["bf16x3"] if s3 else []), env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("FUSED_CASES ")][-1]
    for rec in json.loads(line[len("FUSED_CASES "):]):
        assert rec["vs_oracle"] <= 1e-5, rec                       # the pair is right, not just equal
        for run in rec["runs"]:
            assert run["timed_out"] == 0 and run["launches"] >= 1, rec
            assert run["kernel"] == f"stack_kernel<{ni}>", rec
            assert run["equal"], rec
            if run.get("chain"):      # whole chains: the tail kernel ran (or, switched off, did not)
                # (an evaluation that needs several fused launches - sample chunks - keeps the separate tail launches)
                # (DR_TEST_TUNE="fused_tail=0" - a forced-mode run of the suite - only changes the DEFAULT: runs that set the option carry "tail")
                env_off = "tail" not in run and tuning_env.forced("fused_tail", 1) == 0
                want_tail = run.get("tail", 1) == 1 and rec["runs"][0]["launches"] == 1 and not env_off and not s3
                assert (run["tail_launches"] >= 1) == want_tail, rec


def test_fused_stack_with_per_sample_steps_and_whole_chain():
    """forward() with a (B,) step tensor of differing entries (the step-embedding row is selected per sample inside
    the fused kernel's 1x1 epilogues), and a whole captured chain (graph replay re-uses the in-kernel re-armed
    counters: three replays, identical rolls)."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=128, residual_layers=4, kernel_size=9, timesteps=10)
    p = R.synthetic_params(hp, seed=77)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    torch.manual_seed(8)
    B, Tn = 8, 100
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    steps = torch.tensor([0, 9, 3, 3, 7, 1, 5, 2])
    # (in this process the per-phase launches pick their own kernel flavours - split-K, 16x16 MFMA tiles - so the
    # agreement here is fp32 round-off, not bitwise; the two block mappings of the fused kernel ARE bitwise equal)
    ref, outs = _run_both(m, lambda: m(x, wav, steps)[0])
    for xcd, out, launches in outs:
        assert launches >= 1 and float((out - ref).abs().max()) <= 2e-6, xcd
    assert torch.equal(outs[0][1], outs[1][1])
    noise = torch.randn(hp["timesteps"], B, 1, Tn, 88)
    ref, outs = _run_both(m, lambda: m.sample(x, wav, noise=noise)[0], xcds=(1,))
    assert float((outs[0][1] - ref).abs().max()) <= 5e-6
    with torch.no_grad():
        want = R.sample_chain(p, hp, "cfdg_ddpm_x0", x, wav, noise, w=0.5)
    assert float((outs[0][1].cpu() - want).abs().max()) <= 1e-5
    m.engine.set_option("fused_stack", 2)
    a = m.sample(x, wav, seed=4)[0]
    b = m.sample(x, wav, seed=4)[0]
    c = m.sample(x, wav, seed=4)[0]
    assert torch.equal(a, b) and torch.equal(a, c)
    assert m.engine.stack_status()[0] == 0


def test_fused_stack_soak_under_uneven_load():
    """Hand-offs are only trustworthy when tested with the consumers' caches warm and the chip unevenly loaded: the
    same evaluation 40 times in a row (L1 / L2 hold the previous round's g / hd at the very same addresses), half
    of them with a second stream hammering HBM with copies - every result must be bit-identical to the per-phase
    reference."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_layers=3, timesteps=6)            # full width: 8 M tiles
    p = R.synthetic_params(hp, seed=5)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5)
    torch.manual_seed(3)
    B, Tn = 12, 125                                       # 24 evaluations: 192 of 256 CUs, the rest idle (uneven)
    wav = 0.1 * torch.randn(B, Tn * 512)
    x = torch.randn(B, 1, Tn, 88)
    z = torch.randn(B, 1, Tn, 88)
    eng = m.engine
    eng.set_option("fused_stack", 0)
    per_phase = m.reverse_diffusion(x, wav, 2, noise=z)[0]
    eng.set_option("fused_stack", 2)
    # (in THIS process the per-phase launches may split K - the narrow output projection does - so they agree with
    # the fused step to fp32 round-off; bitwise identity with pinned flavours is the test above.  The reference every
    # repetition must reproduce bit for bit is the fused step's own first, quiet, result.)
    ref = m.reverse_diffusion(x, wav, 2, noise=z)[0]
    assert float((ref - per_phase).abs().max()) <= 2e-6
    side = torch.cuda.Stream()
    big = torch.empty(64 << 20, device="cuda")
    # mapping 1: every group inside one XCD (plain stores, shared L2); mapping 0: groups span all XCDs, so every
    # hand-off is write-through stores + loads that must not hit a stale line in ANOTHER XCD's L2
    for xcd in (1, 0):
        eng.set_option("fused_stack_xcd", xcd)
        for it in range(40):
            if it % 2:
                with torch.cuda.stream(side):
                    for _ in range(4):
                        big.copy_(big.flip(0))
            out = m.reverse_diffusion(x, wav, 2, noise=z)[0]
            assert torch.equal(out, ref), (xcd, it)
        torch.cuda.synchronize()
        assert eng.stack_status()[0] == 0
    eng.set_option("fused_stack_xcd", 1)
    eng.set_option("fused_stack", 1)


# (what happens when a group barrier can NOT complete - bounded spins, the flag, dr_finish, the re-run on the per-phase
# kernels - is covered by tests/test_gpu_r3.py)


@pytest.mark.parametrize("flavour,args", [("2", ["--T", "500", "--reps", "200"]),
                                          ("1", ["--T", "250", "--reps", "200"]),
                                          ("2", ["--T", "640", "--reps", "200"]),                    # five 128-frame tiles per clip: 40-block groups
                                          ("2", ["--T", "500", "--chain", "6", "--reps", "40"]),     # chains: the tail kernel too
                                          ("1", ["--T", "250", "--chain", "6", "--reps", "40"]),
                                          ("5", ["--T", "640", "--reps", "200"]),                    # four 160-frame tiles per clip: 32-block groups
                                          ("5", ["--T", "640", "--k", "15", "--reps", "60"]),        # BASELINE config 5: halo 56 frames
                                          ("5", ["--T", "640", "--chain", "6", "--reps", "40"])])    # ... with the tail kernel (96-frame T4 items)
def test_cross_xcd_handoffs_of_a_deep_net_are_bitwise_repeatable(flavour, args):
    """tools/xcd_stress.py: the full-depth (15-layer) full-width net with 32- / 64-block groups, block mapping 0 (every
    group spread over all eight XCDs: every hand-off crosses XCDs, and the X tiles of a conv phase arrive from memory
    instead of the local L2) against mapping 1, bit for bit, >= 200 persistent launches per flavour (128-, 64- and 160-frame
    blocks; whole chains bring the tail kernel in).  This is the class of test that exposed the missing
    wait before the LDS-DMA hand-over barrier in round 3 (25 % of the runs of the then 160-frame flavour)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from tools import tuning_env
    env = tuning_env.env_with(tune__stack_fl=int(flavour))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "xcd_stress.py")] + args, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2000:])
    assert "RESULT ok" in r.stdout, r.stdout[-2000:]
    assert f"stack_kernel<{flavour}>" in r.stdout, r.stdout[-500:]


def test_fused_chain_soak_is_bitwise_repeatable_at_the_bench_geometries():
    """tools/fused_soak.py: 6 captured 200-step chains each at BASELINE config 2 (128-frame blocks), config 3 (64-frame
    blocks) and the reference's 640-frame shipping geometry (config 6: 160-frame blocks) - 3 x 1200 fused + tail launches -
    must give bit-identical rolls, without a barrier time-out."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for cfg in ("2", "3", "6"):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "fused_soak.py"), "--chains", "6", "--config", cfg],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (cfg, r.stdout[-1500:], r.stderr[-2000:])
        assert "mismatching chains 0, barrier time-outs 0" in r.stdout, r.stdout[-1000:]


def test_split_k_determinism_soak():
    """tools/determinism_soak.py: 64 shape / seed / precision combinations of small launches (split-K through the
    workspace: write-through partials, tickets, the last arriver's ordered re-read), every 10-step chain run twice with
    the same seed: bit-identical."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "determinism_soak.py"), "64"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2000:])
    assert "every chain bitwise repeatable" in r.stdout, r.stdout[-500:]


def test_handoff_litmus_plain_stores_across_xcds_are_caught():
    """Why the in-launch hand-offs are written the way they are, as a failing experiment: a LITMUS build (-DDR_FAULT=2) stores
    g / hd with plain stores even when a group's blocks sit on different XCDs.  The XCDs' L2s are not coherent with each
    other, so the consumers (sc1 loads: L1 bypassed, their own L2 or memory) then read lines the producer's L2 never wrote
    back - and tools/xcd_stress.py, which compares block mapping 0 (groups spread over all XCDs) with mapping 1 (a group
    inside one XCD, where plain stores ARE sufficient), must see different rolls.  The production build passes the same
    comparison bit for bit (test above): relaxed agent-scope counters + s_waitcnt vmcnt(0) order the hand-off, the sc1
    write-through is what makes the data visible, and nothing weaker than it is.  (The missing-wait race of round 3 has its
    own litmus build, -DDR_FAULT=1: probabilistic - tools/gpu_soak.sh runs it, DESIGN.md section 5 has the counts.)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from diffroll_amd import build
    lib = build.build(verbose=False, variant="fault2")
    from tools import tuning_env
    env = tuning_env.env_with(dict(os.environ, DR_LIB=lib), tune__stack_fl=2)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "xcd_stress.py"), "--T", "500", "--reps", "12"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2000:])
    assert "mapping 1 repeatable: True" in r.stdout, r.stdout[-2000:]      # inside one XCD plain stores are fine ...
    assert "RESULT FAIL" in r.stdout, r.stdout[-2000:]                     # ... across XCDs they are not


@pytest.mark.parametrize("accumulation", ["single_chain", "blocked"])
def test_fused_tail_on_and_off_give_the_same_bits_with_natural_tile_selection(accumulation):
    """at the bench geometry (16 guided clips x 125 frames) the first step of a chain - and every step with
    fused_tail = 0 - runs layer 0's shared conv as a per-phase launch on 64-frame tiles (256 blocks: what the cost model
    picks), the later steps run it inside the tail kernel.  Under accumulation='single_chain' (blocked_accumulation = 1:
    the 128-frame stack keeps one chain per output) both must contract as ONE chain (GemmArgs::nofold64 / TailArgs::fold
    = 0), under the default both in 32-channel blocks: the header's claim that fused_tail only changes the launch count."""
    from tools import tuning_env
    if tuning_env.is_forced("blocked_accumulation") or tuning_env.is_forced("fused_tail") or tuning_env.is_forced("fused_stack"):
        pytest.skip("DR_TEST_TUNE pins the options this test switches")
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=512, residual_layers=3, kernel_size=9, timesteps=6)
    p = R.synthetic_params(hp, seed=11)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, accumulation=accumulation)
    g = torch.Generator().manual_seed(12)
    B, Tn = 16, 125
    wav = 0.1 * torch.randn(B, Tn * 512, generator=g)
    x = torch.randn(B, 1, Tn, 88, generator=g)
    noise = torch.randn(6, B, 1, Tn, 88, generator=g)
    eng = m.engine
    # (split-K off: the narrow projections behind the stack - M = 88 / 512 rows - would otherwise be cut in K through the
    # workspace when they run as launches of their own, which is a different summation order from the tail kernel's by
    # design; the option is process-wide, hence the restore)
    eng.set_option("tune.ksplit_max", 1)
    try:
        t0 = eng.tail_launches
        with_tail, _ = m.sample(x, wav, noise=noise)
        assert eng.tail_launches > t0                              # the tail kernel is what ran
        eng.set_option("fused_tail", 0)
        t1 = eng.tail_launches
        without, _ = m.sample(x, wav, noise=noise)
        assert eng.tail_launches == t1
    finally:
        eng.set_option("tune.ksplit_max", 16)
    assert torch.equal(with_tail, without)
    with torch.no_grad():
        ref = R.sample_chain(p, hp, "cfdg_ddpm_x0", x, wav, noise, w=0.5)
    assert float((with_tail.cpu() - ref).abs().max()) <= 1e-5


def test_set_precision_failure_leaves_the_engine_usable(monkeypatch):
    """dr_set_precision commits the mode only after the split-bf16 packings exist, and a commit
    made AFTER the switch rebuilds them before the next launch (check_ready) - no launch ever sees null packings."""
    hp = dict(R.DEFAULT_HP)
    hp.update(residual_channels=128, residual_layers=2, kernel_size=9, timesteps=4)
    p = R.synthetic_params(hp, seed=5)
    m = make_model(hp, p, sampler="cfdg_ddpm_x0", w=0.5, precision="bf16x3")
    g = torch.Generator().manual_seed(2)
    wav = 0.1 * torch.randn(2, 40 * 512, generator=g)
    x = torch.randn(2, 1, 40, 88, generator=g)
    noise = torch.randn(4, 2, 1, 40, 88, generator=g)
    a, _ = m.sample(x, wav, noise=noise)
    # new weights while the split precision is on: the re-commit drops the packings, the next call rebuilds them
    p2 = R.synthetic_params(hp, seed=6)
    m.load_state_dict(p2)
    b, _ = m.sample(x, wav, noise=noise)
    with torch.no_grad():
        ref = R.sample_chain(p2, hp, "cfdg_ddpm_x0", x, wav, noise, w=0.5)
    assert float((b.cpu() - ref).abs().max()) <= 1e-5 and not torch.equal(a, b)
