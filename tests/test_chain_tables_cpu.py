"""csrc/chain_tables.h without a GPU: the engine's own visited steps, respaced and solver coefficient rows, start position,
history rule of dr_step under solver order 2 and per-window table, compiled into a small C++ driver and held to
tests/chain_ref.py (the independent numpy restatement), diffroll_amd.schedule and brute-force statements in Python.  The
driver is handed the committed fp32 tables the engine is handed (diffroll_amd.schedule.sampler_coef_tables)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import diffroll_ref as R

import chain_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# One command per input line; every answer is a count followed by that many 32-bit words on stdout.
DRIVER = r"""
    #include <cstdint>
    #include <cstdio>
    #include <iostream>
    #include <sstream>
    #include <string>
    #include "chain_tables.h"
    static void put(const void* p, size_t words) {
        const uint32_t n = (uint32_t)words;
        fwrite(&n, 4, 1, stdout);
        fwrite(p, 4, words, stdout);
    }
    int main() {
        std::vector<float> coef;
        dr::ChainSteps steps;
        std::string line, cmd;
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            in >> cmd;
            if (cmd == "groups") {
                const int g = dr::STACK_GROUPS;
                put(&g, 1);
            } else if (cmd == "coef") {            // coef FILE S: the committed (DR_COEF_FAMILIES, S, 5) table
                std::string path; int S = 0;
                in >> path >> S;
                coef.assign((size_t)DR_COEF_FAMILIES * S * 5, 0.f);
                FILE* f = fopen(path.c_str(), "rb");
                if (!f || fread(coef.data(), 4, coef.size(), f) != coef.size()) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 1; }
                fclose(f);
            } else if (cmd == "steps") {           // steps S n: count, at(-1 .. count), position(-1 .. S), successor(-1 .. S)
                int S = 0, n = 0;
                in >> S >> n;
                steps = dr::ChainSteps(S, n);
                std::vector<int> out{steps.count(), (int)steps.respaced()};
                for (int i = -1; i <= steps.count(); ++i) out.push_back(steps.at(i));
                for (int t = -1; t <= S; ++t) out.push_back(steps.position(t));
                for (int t = -1; t <= S; ++t) out.push_back(steps.successor(t));
                put(out.data(), out.size());
            } else if (cmd == "respaced") {
                const std::vector<float> tab = dr::respaced_table(coef, steps);
                put(tab.data(), tab.size());
            } else if (cmd == "solver") {          // solver ORDER NOISE
                int order = 0, noise = 0;
                in >> order >> noise;
                const std::vector<float> tab = dr::solver_table(coef, steps, order, noise);
                put(tab.data(), tab.size());
            } else if (cmd == "start") {           // start START_STEP
                int ts = 0;
                in >> ts;
                const dr::StartPosition p = dr::start_position(steps, ts);
                const int out[3] = {p.pos, p.above, p.below};
                put(out, 3);
            } else if (cmd == "hist") {            // hist VALID SAMPLER B T t | SAMPLER B T t START_STEP
                dr::HistoryKey k;
                int valid = 0, sampler = 0, B = 0, T = 0, t = 0, start = 0;
                in >> valid >> k.sampler >> k.B >> k.T >> k.t >> sampler >> B >> T >> t >> start;
                k.valid = valid != 0;
                const dr::HistoryVerdict v = dr::history_step(k, sampler, B, T, t, steps, start);
                const int out[2] = {(int)v.what, v.expect};
                put(out, 2);
            } else if (cmd == "win") {             // win B DRAWS STRIDE marks...
                int B = 0, draws = 1, stride = 0, m = 0;
                in >> B >> draws >> stride;
                std::vector<int> marks;
                while (in >> m) marks.push_back(m);
                const dr::WindowTable tab = dr::window_table(marks, B, draws, stride);
                put(tab.w, (size_t)B);
            } else {
                fprintf(stderr, "unknown command %s\n", cmd.c_str());
                return 1;
            }
        }
        return 0;
    }
"""

STARTS, CONTINUES, REFUSED = 0, 1, 2      # dr::HistoryStep
GRID = [(S, n) for S in (50, 200, 1000) for n in sorted({0, 2, 3, 4, 7, 20, 50, S - 1, S})]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("chain_tables")
    src = d / "chain_tables_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "chain_tables_driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diffroll_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def ask(driver, lines, dtype=np.int32):
    """one array per answering command (coef answers nothing)"""
    r = subprocess.run([driver], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out, pos = [], 0
    while pos < len(r.stdout):
        n, = struct.unpack_from("<I", r.stdout, pos)
        out.append(np.frombuffer(r.stdout, dtype=dtype, count=n, offset=pos + 4))
        pos += 4 + 4 * n
    assert len(out) == sum(1 for ln in lines if not ln.startswith("coef"))
    return out


_tables = {}


def committed(S):
    if S not in _tables:
        _tables[S] = CR.committed(dict(R.DEFAULT_HP, timesteps=S))
    return _tables[S]


@pytest.fixture(scope="module")
def coef_files(tmp_path_factory):
    """S -> file of the committed (5, S, 5) fp32 table"""
    d = tmp_path_factory.mktemp("chain_tables_coef")
    out = {}
    for S in (50, 200, 1000):
        out[S] = str(d / f"coef_{S}.bin")
        np.ascontiguousarray(committed(S), dtype="<f4").tofile(out[S])
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulps(a, b):
    """distance in fp32 units in the last place (the ordered integer image of the bit patterns)"""
    def key(x):
        i = bits(x).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------- steps
def test_steps_are_the_restated_and_the_facades(driver):
    from diffroll_amd.schedule import respaced_steps
    got = ask(driver, [f"steps {S} {n}" for S, n in GRID])
    for (S, n), g in zip(GRID, got):
        want = CR.visited(S, n)
        assert want == respaced_steps(S, n)
        count, respaced = int(g[0]), int(g[1])
        assert count == len(want) and respaced == (n not in (0, S)), (S, n)
        at, rest = g[2:2 + count + 2], g[2 + count + 2:]
        position, successor = rest[:S + 2], rest[S + 2:]
        assert len(successor) == S + 2
        assert at[0] == -1 and at[-1] == -1 and list(at[1:-1]) == want, (S, n)       # -1 past either end
        pos = {t: i for i, t in enumerate(want)}
        assert list(position) == [-1] + [pos.get(t, -1) for t in range(S)] + [-1], (S, n)
        nxt = dict(zip(want, want[1:]))
        assert list(successor) == [-1] + [nxt.get(t, -1) for t in range(S)] + [-1], (S, n)


# ---------------------------------------------------------------------------------------------- respaced rows
def test_respaced_rows_are_bit_equal_to_the_restatement(driver, coef_files):
    """Guaranteed, not measured: only + - x / sqrt in IEEE double on both sides, and one rounding to fp32."""
    lines = []
    for S in (50, 200, 1000):
        lines.append(f"coef {coef_files[S]} {S}")
        for S2, n in GRID:
            if S2 == S:
                lines += [f"steps {S} {n}", "respaced"]
    got = ask(driver, lines, np.uint32)[1::2]
    for (S, n), g in zip(GRID, got):
        tab, steps = committed(S), CR.visited(S, n)
        want = tab.copy()                      # unvisited steps and stride-1 steps: the committed rows
        derived = 0
        for t, rows in CR.rows_for(tab, steps).items():
            derived += not np.array_equal(bits(rows), bits(tab[:, t, :]))
            want[:, t, :] = rows
        assert derived == sum(1 for t, tp in zip(steps, steps[1:]) if tp != t - 1), (S, n)      # (what is compared are derived rows)
        assert np.array_equal(g.reshape(5, S, 5), bits(want)), (S, n)


# ---------------------------------------------------------------------------------------------- solver rows
def test_solver_rows_are_within_one_ulp_of_the_restatement(driver, coef_files, monkeypatch):
    """1 ulp: log / exp / expm1 are below 1 ulp in double in libm and in numpy, the other operations are exact-rounded,
    and both sides round to fp32 once - a double result that differs in its last places rounds to the same or to the
    neighbouring fp32.  The number of rows that are not bit-identical is printed (0 where libm and numpy agree)."""
    monkeypatch.setattr(CR, "committed", lambda hp: committed(int(hp["timesteps"])))      # (solver_rows builds it per call)
    variants = [(1, 0), (2, 0), (1, 1), (2, 1)]
    lines = []
    for S in (50, 200, 1000):
        lines.append(f"coef {coef_files[S]} {S}")
        for S2, n in GRID:
            if S2 == S:
                lines.append(f"steps {S} {n}")
                lines += [f"solver {o} {z}" for o, z in [(0, 0), (0, 1)] + variants]
    got = iter(ask(driver, lines))
    rows_seen = rows_differ = 0
    for S, n in GRID:
        next(got)
        steps = CR.visited(S, n)
        A = committed(S)[0, :, 2]
        for _ in range(2):                     # order 0: all zero, whatever the noise option says
            g = next(got)
            assert len(g) == 2 * S * 5 and not g.any(), (S, n)
        for order, noise in variants:
            tab = next(got).view(np.float32).reshape(2, S, 5)
            want = CR.solver_rows(dict(R.DEFAULT_HP, timesteps=S), n, order, noise)
            assert sorted(want, reverse=True) == steps
            d = ulps(tab[0, steps], np.stack([want[t] for t in steps]))
            assert d.max() <= 1, (S, n, order, noise, [steps[i] for i in np.nonzero(d.max(1) > 1)[0]])
            rows_seen += len(steps)
            rows_differ += int(d.any(1).sum())
            unvisited = np.setdiff1d(np.arange(S), steps)
            assert not bits(tab[:, unvisited]).any(), (S, n, order, noise)
            assert np.array_equal(bits(tab[0, 0]), bits([0, 0, A[0], 0, 0])), (S, n, order, noise)
            # column 3: 0 at the first position, for the step into 0 and under order 1 - and nowhere else under order 2
            c = tab[0, :, 3]
            assert c[steps[0]] == 0 and c[steps[-2]] == 0 and c[0] == 0, (S, n, order, noise)
            if order == 1:
                assert not bits(c).any(), (S, n, noise)
            else:
                assert (c[steps[1:-2]] > 0).all(), (S, n, noise)
            # column 4 is the step's sigma: only the stochastic form has one
            assert (tab[0, steps[:-1], 4] > 0).all() if noise else not bits(tab[0, :, 4]).any(), (S, n, order)
            # rows [S, 2 S): the same rows as a chain's first step
            first = tab[0].copy()
            first[:, 3] = 0
            assert np.array_equal(bits(tab[1]), bits(first)), (S, n, order, noise)
    print(f"solver rows compared: {rows_seen}, not bit-identical to chain_ref.solver_rows: {rows_differ}")


# ---------------------------------------------------------------------------------------------- start position
def test_start_position(driver):
    cases = [(S, n, ts) for S, n in GRID if S != 1000 for ts in range(-1, S)]
    lines, last = [], None
    for S, n, ts in cases:
        if (S, n) != last:
            lines.append(f"steps {S} {n}")
            last = (S, n)
        lines.append(f"start {ts}")
    got = [g for g in ask(driver, lines) if len(g) == 3]
    assert len(got) == len(cases)
    for (S, n, ts), g in zip(cases, got):
        steps = CR.visited(S, n)
        if ts < 0:
            assert list(g) == [0, -1, -1]
        elif ts in steps:
            assert list(g) == [steps.index(ts), -1, -1], (S, n, ts)
        else:
            assert list(g) == [-1, min(t for t in steps if t > ts), max(t for t in steps if t < ts)], (S, n, ts)
    # the neighbours today's message names
    _, g = ask(driver, ["steps 200 20", "start 100"])
    assert list(g) == [-1, 105, 94]


# ---------------------------------------------------------------------------------------------- history rule
def test_history_rule_of_dr_step(driver):
    steps = CR.visited(200, 20)
    assert steps[:4] == [199, 189, 178, 168]
    key = "1 1 2 40"                          # a valid history of sampler 1, B = 2, T = 40 ...
    call = "1 2 40"
    cases = [
        (f"0 -1 0 0 -1 {call} 199 -1", (STARTS, 199)),              # the chain's first step, nothing held
        (f"{key} 178 {call} 199 -1", (STARTS, 199)),                # ... and whatever is held
        (f"0 -1 0 0 -1 {call} 168 168", (STARTS, 168)),             # the step "start_step" names
        (f"{key} 199 {call} 168 168", (STARTS, 168)),
        (f"{key} 199 {call} 189 -1", (CONTINUES, 189)),             # the successor of the step held
        (f"{key} 189 {call} 178 -1", (CONTINUES, 178)),
        (f"{key} 168 {call} 157 168", (CONTINUES, 157)),            # a started chain goes on
        (f"{key} 10 {call} 0 -1", (CONTINUES, 0)),                  # the step into 0
        (f"{key} 199 {call} 178 -1", (REFUSED, 189)),               # a wrong t: a step skipped,
        (f"{key} 189 {call} 189 -1", (REFUSED, 178)),               # repeated,
        (f"{key} 189 {call} 188 -1", (REFUSED, 178)),               # or not visited
        (f"{key} 199 2 2 40 189 -1", (REFUSED, 199)),               # another sampler,
        (f"{key} 199 1 3 40 189 -1", (REFUSED, 199)),               # batch
        (f"{key} 199 1 2 41 189 -1", (REFUSED, 199)),               # or frame count
        (f"0 1 2 40 199 {call} 189 -1", (REFUSED, 199)),            # an invalid key
        (f"{key} 100 {call} 94 -1", (REFUSED, 199)),                # a key whose step the chain does not visit
    ]
    got = ask(driver, ["steps 200 20"] + [f"hist {c}" for c, _ in cases])[1:]
    for (c, want), g in zip(cases, got):
        assert tuple(g) == want, c
    # every step: t continues exactly the history of its predecessor
    full = ask(driver, ["steps 50 0"] + [f"hist {key} {k} {call} {t} -1" for k in range(1, 50) for t in range(49)])[1:]
    for (k, t), g in zip(((k, t) for k in range(1, 50) for t in range(49)), full):
        assert tuple(g) == ((CONTINUES if t == k - 1 else REFUSED), k - 1), (k, t)


# ---------------------------------------------------------------------------------------------- window table
def test_window_table_is_the_brute_force_statement(driver):
    """window j of draw d: (d * stride + #{marks <= j}, j - the last mark <= j, or j) - stride: "draw_stride", or the
    recordings of one draw"""
    G, = ask(driver, ["groups"])[0]
    assert G == 512
    cases = []
    for draws in (1, 3):
        for n in (2, 5, 6, 64, G // draws):
            B = n * draws
            for marks in ([], [1], [3, 4], [n - 1], [1, 3, 4, n - 1]):
                marks = sorted(set(marks))
                if marks and marks[-1] >= n:
                    continue
                for stride in (0, 7):
                    cases.append((B, draws, stride, marks))
    assert max(c[0] for c in cases) == G
    got = ask(driver, ["win %d %d %d %s" % (B, D, s, " ".join(map(str, m))) for B, D, s, m in cases], np.uint32)
    for (B, D, stride, marks), g in zip(cases, got):
        n = B // D
        eff = stride if stride > 0 else len(marks) + 1
        want = []
        for d in range(D):
            for j in range(n):
                below = [m for m in marks if m <= j]
                want.append(((d * eff + len(below)) << 16) | (j - (below[-1] if below else 0)))
        assert list(g) == want, (B, D, stride, marks)
