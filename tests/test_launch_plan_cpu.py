"""csrc/launch_plan.h without a GPU: the launch plan of one network evaluation (fused residual stack or one launch per
phase, block flavour, sample chunks, tail kernel) and the per-phase tiles, compiled into a small C++ driver and pinned
at the bench.py configurations' per-GPU shapes - at full depth (C = 512, L = 15) and at the two-layer depth of
test_gpu_parity's 640-frame family.  The full-depth expectations are what the kernel-trace records in profiles/ show ran."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
    #include <cstdio>
    #include <cstring>
    #include <string>
    #include "launch_plan.h"
    int main() {
        char line[512];
        while (fgets(line, sizeof line, stdin)) {
            dr::NetShape s{};
            dr::PlanKnobs k;
            int tsel = 0, offered = 0, used = 0;
            if (sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d%n", &s.NB, &s.n_cond, &s.bmod, &s.T, &s.Cp, &s.L, &s.K,
                       &s.max_dil, &s.prec, &s.n_cus, &s.fuse, &s.opt_blocked, &s.opt_tail, &tsel, &offered, &used) < 15) {
                printf("bad line\n");
                return 1;
            }
            s.has_tsel = tsel; s.tail_offered = offered;
            char name[32];
            long value;
            int n = 0;
            for (const char* p = line + used; sscanf(p, " %31[a-z_0-9]=%ld%n", name, &value, &n) == 2; p += n) {
                const std::string f = name;
                if (f == "tile") k.tile = (int)value;
                else if (f == "pw") k.pw = (int)value;
                else if (f == "pw_nw") k.pw_nw = (int)value;
                else if (f == "pwk") k.pwk = (int)value;
                else if (f == "ksplit_max") k.ksplit_max = (int)value;
                else if (f == "ksplit_blocks") k.ksplit_blocks = value;
                else if (f == "stack3") k.stack3 = (int)value;
                else if (f == "stack_fl") k.stack_fl = (int)value;
                else if (f == "xcd_n") k.xcd_n = (int)value;
                else if (f == "xcd_model") k.xcd_model = (int)value;
                else if (f == "tail_t4") k.tail_t4 = (int)value;
                else if (f == "one_ks") k.one_ks = (int)value;
                else { printf("unknown knob %s\n", name); return 1; }
            }
            const dr::NetPlan p = dr::plan_network(s, k);
            // the per-phase tiles run_network would launch: layer 0's conv (a guided pair's shared contraction or not), a
            // later layer's conv at the largest dilation, the 1x1 residual/skip GEMM and the last layer's skip half
            const int MT = s.Cp / 64, first = s.Cp / 128;
            const bool wide32 = s.opt_blocked >= 2;
            const dr::Tile c0 = p.dual0 ? dr::pick_tile(k, MT, s.bmod, s.T, s.K, 1, s.prec, dr::EPI_GATE, false, wide32)
                                        : dr::pick_tile(k, MT, s.NB, s.T, s.K, 1, s.prec, dr::EPI_GATE, true, wide32);
            const dr::Tile cl = dr::pick_tile(k, MT, s.NB, s.T, s.K, s.max_dil, s.prec, dr::EPI_GATE, true, wide32);
            const dr::Tile pw = dr::pick_pointwise_tile(k, MT, s.NB, s.T, s.prec);
            const dr::Tile half = dr::pick_pointwise_tile(k, MT - first, s.NB, s.T, s.prec, s.Cp / 32);
            printf("%d %d %d %d %d %d %d %d %d,%d %d,%d %d,%d %d,%d\n", p.stack_fl, p.stack_chunks, p.stack_from, (int)p.dual0,
                   (int)p.fold, (int)p.fused_step, (int)p.use_tail, p.mode, c0.flavor, c0.n, cl.flavor, cl.n, pw.flavor, pw.n,
                   half.flavor, half.n);
        }
        return 0;
    }
"""

MODES = {1: "per_phase", 2: "fused_stack", 3: "fused_stack+tail"}
FULL = dict(Cp=512, L=15, max_dil=8, n_cus=256)       # C = 512, L = 15, dilations 1 / 2 / 4 / 8 (base 2, bound 4), 256 CUs
SHALLOW = dict(Cp=512, L=2, max_dil=2, n_cus=256)     # residual_layers = 2: dilations 1 / 2

# bench.py CONFIGS at their per-GPU shape: (NB, n_cond, bmod, T, K) of one network evaluation as run_step issues it
# (classifier-free guidance: 2B evaluations of B inputs, the first B conditional; generation: B unconditional ones)
CONFIGS = {
    1: (2, 1, 1, 125, 9),        # cfdg_ddpm_x0, B = 1
    2: (32, 16, 16, 125, 9),     # cfdg_ddpm_x0, B = 16
    3: (16, 0, 16, 125, 9),      # generation_ddpm_x0, B = 16
    4: (32, 16, 16, 125, 9),     # inpainting_ddpm_x0, B = 16
    5: (8, 4, 4, 640, 15),       # cfdg_ddpm_x0, B = 4, k = 15
    6: (8, 4, 4, 640, 9),        # cfdg_ddpm_x0, B = 4
    7: (16, 0, 16, 640, 9),      # generation_ddpm_x0, B = 16
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("launch_plan")
    src = d / "launch_plan_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "launch_plan_driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def plans(driver, cases):
    """cases: dicts of NetShape fields (+ knobs=...); returns one dict per case"""
    lines = []
    for c in cases:
        s = dict(prec=0, fuse=1, opt_blocked=2, opt_tail=1, has_tsel=0, tail_offered=1)
        s.update(c)
        knobs = " ".join(f"{k}={v}" for k, v in s.pop("knobs", {}).items())
        fields = ("NB", "n_cond", "bmod", "T", "Cp", "L", "K", "max_dil", "prec", "n_cus", "fuse", "opt_blocked", "opt_tail",
                  "has_tsel", "tail_offered")
        lines.append(" ".join(str(int(s[f])) for f in fields) + " " + knobs)
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = []
    for got in r.stdout.splitlines():
        v = got.split()
        tile = lambda t: tuple(int(x) for x in t.split(","))
        out.append(dict(stack_fl=int(v[0]), chunks=int(v[1]), stack_from=int(v[2]), dual0=bool(int(v[3])), fold=bool(int(v[4])),
                        fused_step=bool(int(v[5])), use_tail=bool(int(v[6])), mode=MODES[int(v[7])], conv0=tile(v[8]),
                        conv=tile(v[9]), pw=tile(v[10]), pw_half=tile(v[11])))
    assert len(out) == len(cases)
    return out


def config(n, depth=FULL, **kw):
    NB, n_cond, bmod, T, K = CONFIGS[n]
    return dict(depth, NB=NB, n_cond=n_cond, bmod=bmod, T=T, K=K, **kw)


def fused(fl, chunks, frm, mode):
    return dict(stack_fl=fl, chunks=chunks, stack_from=frm, mode=mode)


PER_PHASE = dict(stack_fl=0, stack_from=-1, mode="per_phase", use_tail=False)      # (chunks: unused)


def check(got, want, what):
    assert {k: got[k] for k in want} == want, (what, got)


# profiles/r06_kernel_stats_cfg*.txt (and r06_kernel_stats.txt for config 2): the fused flavour and chunking that ran
FULL_DEPTH = {
    1: PER_PHASE,
    2: dict(fused(2, 1, 1, "fused_stack+tail"), fold=True, dual0=True),
    3: fused(1, 1, 0, "fused_stack+tail"),
    4: dict(fused(2, 1, 1, "fused_stack+tail"), fold=True, dual0=True),
    5: fused(5, 1, 1, "fused_stack+tail"),
    6: fused(5, 1, 1, "fused_stack+tail"),
    7: fused(5, 2, 0, "fused_stack"),                # 2800 stack launches for 1400 evaluations, no tail kernel
}


def test_bench_configs_at_full_depth(driver):
    got = plans(driver, [config(n) for n in FULL_DEPTH])
    for (n, want), g in zip(FULL_DEPTH.items(), got):
        check(g, want, n)


def test_config1_per_phase_tiles(driver):
    """config 1 (one guided clip): gemm_kernel<1, 1, EPI_GATE, 0, 1> for every conv (the shared first-layer contraction
    included) and pwk_kernel<1> for every 1x1, the last layer's skip half too"""
    g, = plans(driver, [config(1)])
    assert g["dual0"] and g["conv0"] == (0, 1) and g["conv"] == (0, 1), g
    assert g["pw"] == (3, 1) and g["pw_half"] == (3, 1), g


def test_640_frame_family_at_two_layers(driver):
    """the seven geometries of test_gpu_parity's 640-frame test (residual_layers = 2), with its expectations; the two
    it does not assert are pinned at what the planner chooses"""
    cases = [  # (NB, n_cond, bmod, T, K), expected
        ((8, 4, 4, 640, 9), fused(5, 1, 1, "fused_stack+tail")),        # B = 4 guided, k = 9
        ((8, 4, 4, 640, 15), fused(5, 1, 1, "fused_stack+tail")),       # ... k = 15
        ((8, 0, 8, 640, 9), fused(5, 1, 0, "fused_stack+tail")),        # 8 generation evaluations
        ((16, 0, 16, 640, 9), fused(5, 2, 0, "fused_stack")),           # two chunks of 8: no tail kernel
        ((8, 4, 4, 600, 9), fused(5, 1, 1, "fused_stack+tail")),        # ragged last tile
        ((4, 2, 2, 640, 9), PER_PHASE),                                 # half the chip: split-K per-phase launches
        ((3, 3, 3, 800, 9), PER_PHASE),                                 # 3 conditional evaluations of 5 tiles
    ]
    got = plans(driver, [dict(SHALLOW, NB=s[0], n_cond=s[1], bmod=s[2], T=s[3], K=s[4]) for s, _ in cases])
    for (s, want), g in zip(cases, got):
        check(g, want, s)


def test_without_the_160_frame_flavour_configs_5_to_7_run_per_phase(driver):
    """tune.stack_fl = -5 (profiles/r06_stack160_ab.txt: mode per_phase, gemm_kernel<EPI_GATE> launches)"""
    got = plans(driver, [config(n, knobs=dict(stack_fl=-5)) for n in (5, 6, 7)])
    for n, g in zip((5, 6, 7), got):
        check(g, PER_PHASE, n)


def test_fused_stack_off_is_per_phase_everywhere(driver):
    for depth in (FULL, SHALLOW):
        for n, g in zip(CONFIGS, plans(driver, [config(n, depth, fuse=0) for n in CONFIGS])):
            check(g, PER_PHASE, (n, depth["L"]))


def test_fused_stack_2_fuses_where_it_fits(driver):
    """fused_stack = 2 skips the cost comparison and the part-filled-chip rule: config 1 fuses too"""
    want = dict(FULL_DEPTH)
    want[1] = fused(1, 1, 1, "fused_stack+tail")
    for (n, w), g in zip(want.items(), plans(driver, [config(n, fuse=2) for n in want])):
        check(g, w, n)


def test_split_bf16_has_no_tail_kernel(driver):
    """prec = 1 (bf16x3) at config 2: the split-bf16 stack flavour, but the fused step is fp32 only"""
    g, = plans(driver, [config(2, prec=1)])
    check(g, dict(fused(2, 1, 1, "fused_stack"), fused_step=False), 2)
    g, = plans(driver, [config(2, prec=1, knobs=dict(stack3=0))])
    check(g, PER_PHASE, "stack3=0")


def test_per_sample_steps_or_no_offer_means_no_tail(driver):
    """dr_forward_steps (per-sample steps) and dr_forward (no TailPlan offered) keep the fused stack, never the tail"""
    for n in (2, 3, 5, 6):
        a, b = plans(driver, [config(n, has_tsel=1), config(n, tail_offered=0)])
        check(a, dict(stack_fl=FULL_DEPTH[n]["stack_fl"], fused_step=False, use_tail=False, mode="fused_stack"), (n, "tsel"))
        check(b, dict(stack_fl=FULL_DEPTH[n]["stack_fl"], fused_step=True, use_tail=False, mode="fused_stack"), (n, "no offer"))


def test_single_chain_128_frame_stack_does_not_fold(driver):
    """blocked_accumulation = 1: the 128-frame flavour keeps one chain per output (and the 160-frame one is not offered)"""
    a, b = plans(driver, [config(2, opt_blocked=1), config(3, opt_blocked=1)])
    check(a, dict(stack_fl=2, fold=False), 2)
    check(b, dict(stack_fl=1, fold=True), 3)
