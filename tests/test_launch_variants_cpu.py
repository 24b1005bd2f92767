"""tests/variant_cases.py without a GPU: every case x pin set of the table reaches the kernel variant it claims, on
csrc/launch_plan.h compiled into a small C++ driver (as tests/test_launch_plan_cpu.py does) - the forced tile is feasible and
taken, the block -> XCD mapping is 1 under tune.xcd_n = 1, plan_ksplit gives the claimed factor, the 1x1 is pwk_kernel of
the claimed width in the full launch and in the last layer's skip half, the tail kernel's item width and the channels per
hand-over are the forced ones (or the stated fall-back).  No case is excluded: a case the planner does not take where it
claims is a failure of the table.  And the three decisions that moved into launch_plan.h (pick_xcd_mapping, pick_one_ks,
tail_t4_width) against a literal restatement of the launchers' former rules, over a grid."""
import itertools
import os
import shutil
import subprocess

import pytest

import variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
    #include <cstdio>
    #include <cstring>
    #include <string>
    #include "launch_plan.h"
    using namespace dr;
    static bool knobs(const char* p, PlanKnobs& k) {
        char name[32];
        long value;
        int n = 0;
        for (; sscanf(p, " %31[a-z_0-9]=%ld%n", name, &value, &n) == 2; p += n) {
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
            else { printf("unknown knob %s\n", name); return false; }
        }
        return true;
    }
    // one per-phase launch as launch_tiled (plan.hip) and the launchers (gemm.hip) carry it out:
    // flavour, n, M tiles, frame tiles, frames per block, mapping, split-K factor, slabs per hand-over
    static void launch(const PlanKnobs& k, Tile t, int MT, int NB, int T, int taps, int kchunks, int prec, int epi) {
        const int BN = t.flavor == 0 ? gemm_block_frames(t.n) : 32 * t.n;
        const int NT = NB * ((T + BN - 1) / BN);
        int KS = 0, ksplit = 1;
        if (t.flavor == 0) {
            KS = prec ? (taps == 1 && kchunks % 4 == 0 ? 4 : 1) : pick_one_ks(taps, kchunks, t.n, epi, k.one_ks);
            ksplit = plan_ksplit(k, (long)MT * NT, kchunks / KS, kchunks, taps, t.n, prec, SK_WS_FLOATS, SK_CNT_N).ks;
        } else if (t.flavor == 1) {
            KS = taps == 1 ? 2 : 1;
        }
        const int xcd = t.flavor == 3 ? 0 : pick_xcd_mapping(k, MT, NT, BN, kchunks, taps);      // (pwk_kernel has one mapping)
        printf(" %d,%d,%d,%d,%d,%d,%d,%d", t.flavor, t.n, MT, NT, BN, xcd, ksplit, KS);
    }
    int main() {
        char line[512];
        while (fgets(line, sizeof line, stdin)) {
            PlanKnobs k;
            int used = 0;
            if (!strncmp(line, "net ", 4)) {
                NetShape s{};
                int tsel = 0, offered = 0;
                if (sscanf(line + 4, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d%n", &s.NB, &s.n_cond, &s.bmod, &s.T, &s.Cp, &s.L, &s.K,
                           &s.max_dil, &s.prec, &s.n_cus, &s.fuse, &s.opt_blocked, &s.opt_tail, &tsel, &offered, &used) < 15) return 1;
                s.has_tsel = tsel; s.tail_offered = offered;
                if (!knobs(line + 4 + used, k)) return 1;
                const NetPlan p = plan_network(s, k);
                const int MT = s.Cp / 64, first = s.Cp / 128, kc = s.Cp / 32;
                const bool wide32 = s.opt_blocked >= 2;
                // the tail kernel's item width, where the tail kernel runs the successor's shared first-layer conv
                const int t4 = p.use_tail && p.dual0 ? tail_t4_width(p.fold, k.tail_t4, true, MT, s.T, stack_tile_frames(p.stack_fl)) : 0;
                printf("%d %d %d %d %d %d %d", p.stack_fl, p.stack_chunks, (int)p.dual0, (int)p.fold, (int)p.use_tail, p.mode, t4);
                // the per-phase launches of run_network (plan.hip: launch_conv, launch_res_skip)
                if (p.dual0) launch(k, pick_tile(k, MT, s.bmod, s.T, s.K, 1, s.prec, EPI_GATE, false, wide32), MT, s.bmod, s.T, s.K, kc, s.prec, EPI_GATE);
                else launch(k, pick_tile(k, MT, s.NB, s.T, s.K, 1, s.prec, EPI_GATE, true, wide32), MT, s.NB, s.T, s.K, kc, s.prec, EPI_GATE);
                launch(k, pick_tile(k, MT, s.NB, s.T, s.K, s.max_dil, s.prec, EPI_GATE, true, wide32), MT, s.NB, s.T, s.K, kc, s.prec, EPI_GATE);
                const Tile pw = pick_pointwise_tile(k, MT, s.NB, s.T, s.prec);
                launch(k, pw, MT, s.NB, s.T, 1, kc, s.prec, EPI_RES_SKIP);
                const Tile half = pick_pointwise_tile(k, MT - first, s.NB, s.T, s.prec, kc);
                if (pw.flavor >= 2 && half.flavor == pw.flavor) launch(k, half, MT - first, s.NB, s.T, 1, kc, s.prec, EPI_RES_SKIP);
                else printf(" -");
                printf("\n");
            } else if (!strncmp(line, "xcd ", 4)) {
                int MT, NT, BN, kc, taps;
                if (sscanf(line + 4, "%d %d %d %d %d%n", &MT, &NT, &BN, &kc, &taps, &used) < 5 || !knobs(line + 4 + used, k)) return 1;
                printf("%d\n", pick_xcd_mapping(k, MT, NT, BN, kc, taps));
            } else if (!strncmp(line, "ks ", 3)) {
                int taps, kc, NI, epi, forced;
                if (sscanf(line + 3, "%d %d %d %d %d", &taps, &kc, &NI, &epi, &forced) < 5) return 1;
                const int KS = pick_one_ks(taps, kc, NI, epi, forced);
                printf("%d %zu\n", KS, gemm_lds_bytes(NI, KS, taps, 1, 0, epi));
            } else if (!strncmp(line, "t4 ", 3)) {
                int fold, forced, dual, MT, T, BN;
                if (sscanf(line + 3, "%d %d %d %d %d %d", &fold, &forced, &dual, &MT, &T, &BN) < 6) return 1;
                printf("%d\n", tail_t4_width(fold, forced, dual, MT, T, BN));
            } else {
                printf("bad line\n");
                return 1;
            }
        }
        return 0;
    }
"""

EPI_PLAIN, EPI_GATE, EPI_RES_SKIP = 0, 3, 4
PREC = {"f32": 0, "bf16x3": 1}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("launch_variants")
    src = d / "launch_variants_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "launch_variants_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def ask(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def knob_text(pins):
    return " ".join(f"{k[len('tune.'):]}={v}" for k, v in pins.items())


def net_line(c, ev, pins, fuse=0):
    NB, n_cond, bmod, tsel = V.evaluations(c)[ev]
    # (blocked accumulation, option "fused_tail" on; the tail kernel is offered to the steps of a chain)
    fields = (NB, n_cond, bmod, c.T, c.C, c.L, c.k, V.max_dil(c), PREC[c.precision], V.N_CUS, fuse, 2, 1, int(tsel), int(c.group == "D"))
    return "net " + " ".join(str(f) for f in fields) + " " + knob_text(pins)


def parse_net(text):
    v = text.split()
    plan = dict(stack_fl=int(v[0]), chunks=int(v[1]), dual0=int(v[2]), fold=int(v[3]), use_tail=int(v[4]), mode=int(v[5]), t4=int(v[6]))
    names = ("flavour", "n", "MT", "NT", "BN", "xcd", "ksplit", "ks")
    launches = {}
    for name, item in zip(V.LAUNCHES, v[7:]):
        launches[name] = None if item == "-" else dict(zip(names, (int(x) for x in item.split(","))))
    assert len(launches) == 4
    return plan, launches


def every_run():
    for c in V.CASES:
        for ps in V.pin_sets(c):
            for ev in V.evaluations(c):
                yield c, ps, ev


def test_the_table_is_the_issue_s():
    """the cases and pin sets, counted: a case dropped from the table would otherwise go unnoticed"""
    count = {g: sum(len(V.pin_sets(c)) for c in V.CASES if c.group == g) for g in "ABCDE"}
    assert count == {"A": 3 * 18 + 4 + 2, "B": 4 * 10, "C": 15 * 2, "D": 4 * 2, "E": 5 + 1}, count
    assert [c.name for c in V.CASES if c.group == "C"][:5] == ["C-C128-B1-T1", "C-C128-B2-T31", "C-C128-B1-T33", "C-C128-B3-T65", "C-C128-B2-T97"]
    for c in V.CASES:
        assert c.T <= 200 and c.steps <= 6 and c.L <= 3, c
        for ps in V.pin_sets(c):
            assert set(ps.pins) <= set(V.DEFAULTS), ps


def test_every_case_reaches_the_variant_it_claims(driver):
    runs = list(every_run())
    # per-phase kernels are the subject of groups A, B, C and E (fused_stack = 0); group D's twins are checked below
    got = ask(driver, [net_line(c, ev, ps.pins) for c, ps, ev in runs])
    got1 = ask(driver, [net_line(c, ev, dict(ps.pins, **{"tune.xcd_n": 1})) for c, ps, ev in runs])
    got0 = ask(driver, [net_line(c, ev, dict(ps.pins, **{"tune.xcd_n": 0})) for c, ps, ev in runs])
    checked = 0
    for (c, ps, ev), text, text1, text0 in zip(runs, got, got1, got0):
        plan, launches = parse_net(text)
        _, launches1 = parse_net(text1)
        _, launches0 = parse_net(text0)
        what = (c.name, ps.label, ev)
        assert plan["stack_fl"] == 0 and plan["mode"] == 1, what                  # one launch per phase
        assert plan["dual0"] == int(ev == "step" and V.guided(c)), what
        for name in V.LAUNCHES:
            want, g, g1, g0 = V.claim(c, ps, ev, name), launches[name], launches1[name], launches0[name]
            if want is None:
                assert g is None, (what, name, g)
                continue
            assert g is not None, (what, name, "no launch of its own")
            assert (g["flavour"], g["n"]) == (g1["flavour"], g1["n"]) == (g0["flavour"], g0["n"]), (what, name)      # the mapping knob changes nothing else
            assert g["ksplit"] == g1["ksplit"] == g0["ksplit"], (what, name)
            assert g0["xcd"] == 0, (what, name)
            if "tile" in want:
                assert (g["flavour"], g["n"]) == want["tile"], (what, name, g)
            if "flavour" in want:
                assert g["flavour"] == want["flavour"], (what, name, g)
            if "ksplit" in want:
                assert g["ksplit"] == want["ksplit"], (what, name, g)
            if "ks" in want:
                assert g["ks"] == want["ks"], (what, name, g)
            if "xcd1" in want:
                assert g1["xcd"] == want["xcd1"], (what, name, g1)
            if c.group == "A" and g["flavour"] != 3:
                # the batch of 8 makes the frame tiles a multiple of 8 at every block width: mapping 1 wherever a launch has
                # more than one M tile
                assert g["NT"] % 8 == 0 and g1["xcd"] == int(g["MT"] > 1), (what, name, g1)
            checked += 1
    assert checked >= 4 * len(runs) - sum(1 for c, ps, ev in runs for n in V.LAUNCHES if V.claim(c, ps, ev, n) is None)


def test_group_a_covers_mapping_1_with_split_k_and_every_kernel(driver):
    """what group A is for, counted over its runs under tune.xcd_n = 1: mapping 1 on gemm_kernel at all four widths with
    split-K factors > 1, on gemm16_kernel at both widths and on pw_kernel at all four; and where tune.xcd_model = 0 decides
    differently from the traffic model"""
    runs = [(c, ps, ev) for c, ps, ev in every_run() if c.group == "A"]
    got1 = ask(driver, [net_line(c, ev, dict(ps.pins, **{"tune.xcd_n": 1})) for c, ps, ev in runs])
    seen = set()
    for text in got1:
        for g in parse_net(text)[1].values():
            if g and g["xcd"] == 1:
                seen.add((g["flavour"], g["n"], g["ksplit"] > 1))
    for n in (1, 2, 3, 5):
        assert (0, n, True) in seen and (0, n, False) in seen, (n, sorted(seen))
    for n in (3, 5):
        assert (1, n, False) in seen, (n, sorted(seen))
    for n in (2, 3, 4, 5):
        assert (2, n, False) in seen, (n, sorted(seen))
    # the two traffic rules: a weight matrix that fits an XCD's L2 reduces the model to the old rule (8 w + x < w + 8 x <=> x > w),
    # so on the small networks the xcd_model twin of the GPU test only holds the knob to "changes no result"; the full-width
    # case is the one whose convs the rules map differently
    model = ask(driver, [net_line(c, ev, ps.pins) for c, ps, ev in runs])
    old = ask(driver, [net_line(c, ev, dict(ps.pins, **{"tune.xcd_model": 0})) for c, ps, ev in runs])
    for (c, ps, ev), a, b in zip(runs, model, old):
        if c.name != V.A_RULES_DIFFER:
            assert a == b, (c.name, ps.label, ev)
            continue
        new_rule, old_rule = parse_net(a)[1], parse_net(b)[1]
        for name in ("conv0", "conv"):
            assert (new_rule[name]["xcd"], old_rule[name]["xcd"]) == (0, 1), (c.name, ps.label, ev, name)
        assert new_rule["pw"]["xcd"] == old_rule["pw"]["xcd"] == 1
    picked = {g["xcd"] for text in model for g in parse_net(text)[1].values() if g and g["flavour"] != 3}
    assert picked == {0, 1}              # the unforced rule takes both mappings in this group: the convs 0, the 1x1 GEMMs 1


def test_group_c_is_pwk_kernel_in_all_three_loop_shapes(driver):
    """K slabs per wave 1 / 2 / 3 (the K loop's remainder-only, pair-only and pair + remainder shapes), in the full launch
    and the skip half (whose M tiles start at mt0 > 0), at both widths; unforced, only some of these shapes are pwk at all"""
    runs = [(c, ps, ev) for c, ps, ev in every_run() if c.group == "C"]
    seen = set()
    for (c, ps, ev), text in zip(runs, ask(driver, [net_line(c, ev, ps.pins) for c, ps, ev in runs])):
        _, launches = parse_net(text)
        for name in ("pw", "half"):
            g = launches[name]
            assert g and g["flavour"] == 3, (c.name, ps.label, ev, name)
            assert g["MT"] == (c.C // 64 if name == "pw" else c.C // 64 - c.C // 128)
            seen.add((c.C // 128, g["n"], name))
    assert seen == set(itertools.product((1, 2, 3), (1, 2), ("pw", "half")))
    # width 2 is not what the planner takes by itself at any of these shapes but the largest: the forcing is needed
    natural = ask(driver, [net_line(c, ev, {}) for c, ps, ev in runs])
    widths = {parse_net(t)[1]["pw"]["n"] for t in natural if parse_net(t)[1]["pw"]["flavour"] == 3}
    assert 1 in widths


def test_group_d_runs_the_tail_kernel_at_the_forced_item_width(driver):
    """fused_stack = 2 with the flavour pinned: one fused launch + the tail kernel, whose next-step first-layer conv takes the
    forced item width (blocked accumulation: the 96-frame body exists); fused_stack = 0 under the same pins: the per-phase
    twins test_gpu_fused.py compares with - gemm_kernel of the flavour's width unsplit, pw_kernel of the matching width"""
    for c in (c for c in V.CASES if c.group == "D"):
        for ps in V.pin_sets(c):
            f = ps.info["fl"]
            fused, = ask(driver, [net_line(c, "step", ps.pins, fuse=2)])
            plan, _ = parse_net(fused)
            assert plan["stack_fl"] == f and plan["chunks"] == 1 and plan["use_tail"] and plan["dual0"] and plan["fold"], (c.name, plan)
            assert plan["mode"] == 3 and plan["t4"] == ps.info["t4"], (c.name, ps.label, plan)
            per_phase, = ask(driver, [net_line(c, "step", ps.pins, fuse=0)])
            plan, launches = parse_net(per_phase)
            assert plan["mode"] == 1
            for name in ("conv0", "conv"):
                assert (launches[name]["flavour"], launches[name]["n"], launches[name]["ksplit"]) == (0, f, 1), (c.name, name)
            for name in ("pw", "half"):
                assert (launches[name]["flavour"], launches[name]["n"]) == (2, ps.info["pw_nw"]), (c.name, name)
        # unforced, T4's width is one of the two: the table's cases reach the other only through the knob
        free, = ask(driver, [net_line(c, "step", {k: v for k, v in ps.pins.items() if k != "tune.tail_t4"}, fuse=2)])
        assert parse_net(free)[0]["t4"] in (1, 3)


def test_one_ks_falls_back_where_it_does_not_fit_or_divide(driver):
    """the finding behind the fix: tune.one_ks = 4 on the 128-frame residual / skip launch asked for 196608 bytes of LDS and
    the launch failed; now the unforced 64 channels stand.  And 6 K slabs (C = 192) ignore a forced 4."""
    q = [(1, 4, 2, EPI_RES_SKIP, 4), (1, 4, 2, EPI_RES_SKIP, 0), (1, 4, 1, EPI_RES_SKIP, 4), (1, 4, 2, EPI_PLAIN, 4),
         (1, 6, 1, EPI_RES_SKIP, 4), (1, 6, 1, EPI_RES_SKIP, 1), (1, 6, 2, EPI_RES_SKIP, 0), (9, 4, 1, EPI_GATE, 4)]
    got = [tuple(int(x) for x in t.split()) for t in ask(driver, ["ks " + " ".join(map(str, a)) for a in q])]
    assert [g[0] for g in got] == [2, 2, 4, 4, 2, 1, 2, 1], got
    assert all(g[1] <= 160 * 1024 for g in got), got
    assert 2 * 8 * 4 * 128 * 16 + 32 * 128 * 16 == 196608 > 160 * 1024


# ---------------------------------------------------------------------------------------------------------------------
# the refactor changed nothing: the three moved decisions against the launchers' former rules, restated literally
# ---------------------------------------------------------------------------------------------------------------------
def old_xcd(MT, NT, BN, kchunks, taps, xcd_n=-1, xcd_model=1):
    wbytes = 4.0 * 128.0 * MT * 32.0 * kchunks * taps
    xbytes = 4.0 * float(NT) * BN * 32.0 * kchunks
    if MT <= 1 or NT % 8 != 0:
        return 0
    if xcd_n >= 0:
        return xcd_n
    if not xcd_model:
        return 1 if xbytes > wbytes else 0
    l2, cus_per_xcd = 4.0 * 1024 * 1024, 32.0
    conc = max(1.0, cus_per_xcd / MT)
    rounds1 = 1.0 if wbytes <= l2 else max(1.0, (NT / 8.0) / conc)
    cost1 = 8.0 * rounds1 * wbytes + xbytes
    panel = wbytes / MT
    rounds0 = 1.0 if panel <= l2 else float(MT * NT + 255) / 256      # (the launcher's cast binds before its division: no floor)
    cost0 = rounds0 * wbytes + 8.0 * xbytes
    return 1 if cost1 < cost0 else 0


def old_ks(taps, kchunks, NI, epi):
    KS = 1 if taps != 1 else (4 if kchunks % 4 == 0 else (2 if kchunks % 2 == 0 else 1))
    if epi == EPI_RES_SKIP and NI == 2 and KS == 4:
        KS = 2
    return KS


def old_t4(fold, forced, dual, MT, T, BN):
    tps = (T + BN - 1) // BN
    pair_blocks = (2 if dual else 1) * MT * tps
    n64, n96 = MT * ((T + 63) // 64), MT * ((T + 95) // 96)
    c64, c96 = (n64 + pair_blocks - 1) // pair_blocks * 64, (n96 + pair_blocks - 1) // pair_blocks * 96
    return 3 if fold and forced != 1 and (c96 < c64 or forced == 3) else 1


def test_moved_mapping_rule_is_the_launchers_former_rule(driver):
    grid = list(itertools.product((1, 2, 3, 6, 8, 16), (1, 7, 8, 16, 24, 40, 64, 160, 320, 1024), (64, 96, 128, 160),
                                  (1, 3, 4, 6, 8, 16, 33), (1, 3, 9, 15)))
    for extra, kw in (("", {}), ("xcd_model=0", dict(xcd_model=0)), ("xcd_n=0", dict(xcd_n=0)), ("xcd_n=1", dict(xcd_n=1))):
        got = ask(driver, ["xcd %d %d %d %d %d %s" % (g + (extra,)) for g in grid])
        want = [str(old_xcd(*g, **kw)) for g in grid]
        assert got == want, (extra, [g for g, a, b in zip(grid, got, want) if a != b][:5])
        if not extra:
            assert set(got) == {"0", "1"}


def block_frames(NI):
    return 32 * NI if NI in (3, 5) else 64 * NI


def test_moved_ks_rule_is_the_launchers_former_rule(driver):
    grid = list(itertools.product((1, 3, 9, 15), range(1, 34), (1, 2, 3, 5), (0, 1, 2, 3, 4, 5, 6)))
    got = [int(t.split()[0]) for t in ask(driver, ["ks %d %d %d %d 0" % g for g in grid])]
    assert got == [old_ks(*g) for g in grid]
    # a forced value, as before, where it divides the K slabs of a 1x1 - and now only where it fits as well
    for forced in (1, 2, 4):
        got = [tuple(int(x) for x in t.split()) for t in ask(driver, ["ks %d %d %d %d %d" % (g + (forced,)) for g in grid])]
        for g, (ks, lds) in zip(grid, got):
            taps, kchunks, NI, epi = g
            fits = 2 * 8 * forced * block_frames(NI) * 16 + (32 * block_frames(NI) * 16 if epi == EPI_RES_SKIP else 0) <= 160 * 1024
            assert ks == (forced if taps == 1 and kchunks % forced == 0 and fits else old_ks(*g)), (g, forced, ks)
            assert NI > 2 or lds <= 160 * 1024, (g, forced, lds)      # (1x1 GEMMs exist on 64- / 128-frame blocks)


def test_moved_t4_rule_is_the_launchers_former_rule(driver):
    grid = list(itertools.product((0, 1), (0, 1, 3), (0, 1), (1, 2, 3, 6, 8), (1, 63, 64, 65, 95, 96, 97, 125, 161, 200, 600, 640),
                                  (64, 128, 160)))
    got = [int(t) for t in ask(driver, ["t4 %d %d %d %d %d %d" % g for g in grid])]
    assert got == [old_t4(*g) for g in grid]
    free = {w for g, w in zip(grid, got) if g[0] == 1 and g[1] == 0}
    assert free == {1, 3}
