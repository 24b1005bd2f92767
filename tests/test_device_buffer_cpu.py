"""csrc/device_buffer.h without a GPU: the owning device buffer of the host runtime compiled against a stub
hip/hip_runtime.h that counts live allocations, logs every malloc / memset / free and can fail the next allocation.  A small
C++ driver is fed commands; after each one it prints the result, the buffer's state and what the stub saw."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = r"""
    #pragma once
    #include <cstddef>
    #include <cstdlib>
    #include <cstring>
    #include <map>
    #include <string>
    enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
    namespace stub {
    inline std::map<void*, int>& ids() { static std::map<void*, int> m; return m; }      // live block -> id
    inline int next_id = 1, fail_next = 0;
    inline std::string log;
    inline int id(const void* p) { auto it = ids().find(const_cast<void*>(p)); return it == ids().end() ? 0 : it->second; }
    inline void note(const std::string& ev) { log += (log.empty() ? "" : " ") + ev; }
    }
    inline hipError_t hipMalloc(void** p, size_t bytes) {
        if (stub::fail_next) { stub::fail_next = 0; *p = nullptr; stub::note("malloc:fail"); return hipErrorOutOfMemory; }
        *p = malloc(bytes);
        memset(*p, 0xAB, bytes);
        stub::ids()[*p] = stub::next_id++;
        stub::note("malloc#" + std::to_string(stub::id(*p)) + ":" + std::to_string(bytes));
        return hipSuccess;
    }
    inline hipError_t hipMemset(void* p, int v, size_t bytes) {
        memset(p, v, bytes);
        stub::note("memset#" + std::to_string(stub::id(p)) + ":" + std::to_string(bytes));
        return hipSuccess;
    }
    inline hipError_t hipFree(void* p) {
        stub::note("free#" + std::to_string(stub::id(p)));
        stub::ids().erase(p);
        free(p);
        return hipSuccess;
    }
"""

DRIVER = r"""
    #include <cstdio>
    #include <cstring>
    #include <utility>
    #include "device_buffer.h"
    int main() {
        drh::DevBuf<float> a, b;
        char line[128], cmd[32];
        while (fgets(line, sizeof line, stdin)) {
            long n = 0, zero = 0;
            if (sscanf(line, "%31s %ld %ld", cmd, &n, &zero) < 1) continue;
            stub::log.clear();
            int rc = 0, fits = -1, byte0 = -1;
            if (!strcmp(cmd, "ensure")) {
                rc = (int)a.ensure((size_t)n, zero != 0);
                if (a) byte0 = ((const unsigned char*)(float*)a)[0];
            }
            else if (!strcmp(cmd, "fits")) fits = a.fits((size_t)n);
            else if (!strcmp(cmd, "fail")) stub::fail_next = 1;
            else if (!strcmp(cmd, "move")) b = std::move(a);               // a -> b
            else if (!strcmp(cmd, "back")) a = drh::DevBuf<float>(std::move(b));  // b -> a (move construction)
            else if (!strcmp(cmd, "reset")) a.reset();
            else if (!strcmp(cmd, "scope")) { drh::DevBuf<float> c; (void)c.ensure((size_t)n, false); }
            else { printf("unknown command %s\n", cmd); return 1; }
            // rc | a: id size | b: id size | fits | first byte | live blocks | stub log
            printf("%d | %d %zu | %d %zu | %d | %d | %zu | %s\n", rc, stub::id((float*)a), a.size(), stub::id((float*)b), b.size(),
                   fits, byte0, stub::ids().size(), stub::log.c_str());
        }
        a.reset(); b.reset();
        printf("live %zu\n", stub::ids().size());
        return 0;
    }
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("device_buffer")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(STUB)
    src = d / "device_buffer_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "device_buffer_driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(d), "-I", os.path.join(ROOT, "diffroll_amd", "csrc"),
           str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def run(driver, steps):
    """steps: (command, "rc | a id size | b id size | fits | first byte | live | stub log") after each command"""
    r = subprocess.run([driver], input="".join(c + "\n" for c, _ in steps), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == len(steps) + 1
    for (c, want), got in zip(steps, lines):
        assert [f.strip() for f in got.split("|")] == [f.strip() for f in want.split("|")], (c, got, want)
    assert lines[-1] == "live 0"          # the destructors (and resets) returned every block


def test_ensure_keeps_the_block_while_it_fits(driver):
    run(driver, [
        ("fits 1",       "0 | 0 0  | 0 0 | 0  | -1  | 0 | "),                      # an empty buffer fits nothing
        ("ensure 100 0", "0 | 1 100 | 0 0 | -1 | 171 | 1 | malloc#1:400"),
        ("fits 100",     "0 | 1 100 | 0 0 | 1  | -1  | 1 | "),
        ("fits 101",     "0 | 1 100 | 0 0 | 0  | -1  | 1 | "),
        ("ensure 100 1", "0 | 1 100 | 0 0 | -1 | 171 | 1 | "),                      # fits: same block, not cleared again
        ("ensure 40 1",  "0 | 1 100 | 0 0 | -1 | 171 | 1 | "),                      # grow-only: a smaller request keeps it
    ])


def test_growth_frees_the_old_block_before_allocating(driver):
    run(driver, [
        ("ensure 100 0", "0 | 1 100 | 0 0 | -1 | 171 | 1 | malloc#1:400"),
        ("ensure 101 0", "0 | 2 101 | 0 0 | -1 | 171 | 1 | free#1 malloc#2:404"),  # never two blocks at once
        ("reset",        "0 | 0 0   | 0 0 | -1 | -1  | 0 | free#2"),
    ])


def test_zero_fill_only_when_asked_and_at_least_16_bytes(driver):
    run(driver, [
        ("ensure 1 1",   "0 | 1 1  | 0 0 | -1 | 0   | 1 | malloc#1:16 memset#1:16"),
        ("ensure 8 0",   "0 | 2 8  | 0 0 | -1 | 171 | 1 | free#1 malloc#2:32"),
        ("ensure 9 1",   "0 | 3 9  | 0 0 | -1 | 0   | 1 | free#2 malloc#3:36 memset#3:36"),
        ("reset",        "0 | 0 0  | 0 0 | -1 | -1  | 0 | free#3"),
        ("ensure 0 0",   "0 | 4 0  | 0 0 | -1 | 171 | 1 | malloc#4:16"),
    ])


def test_failed_allocation_leaves_the_buffer_empty(driver):
    run(driver, [
        ("ensure 10 0",  "0 | 1 10 | 0 0 | -1 | 171 | 1 | malloc#1:40"),
        ("fail",         "0 | 1 10 | 0 0 | -1 | -1  | 1 | "),
        ("ensure 20 1",  "2 | 0 0  | 0 0 | -1 | -1  | 0 | free#1 malloc:fail"),   # error returned, old block gone
        ("fits 0",       "0 | 0 0  | 0 0 | 0  | -1  | 0 | "),
        ("ensure 20 1",  "0 | 2 20 | 0 0 | -1 | 0   | 1 | malloc#2:80 memset#2:80"),
    ])


def test_move_leaves_the_source_empty(driver):
    run(driver, [
        ("ensure 10 0",  "0 | 1 10 | 0 0  | -1 | 171 | 1 | malloc#1:40"),
        ("move",         "0 | 0 0  | 1 10 | -1 | -1  | 1 | "),
        ("ensure 5 0",   "0 | 2 5  | 1 10 | -1 | 171 | 2 | malloc#2:20"),
        ("move",         "0 | 0 0  | 2 5  | -1 | -1  | 1 | free#1"),                # move assignment frees the target's block
        ("back",         "0 | 2 5  | 0 0  | -1 | -1  | 1 | "),
    ])


def test_destructor_frees(driver):
    run(driver, [
        ("scope 64",     "0 | 0 0  | 0 0 | -1 | -1  | 0 | malloc#1:256 free#1"),
        ("ensure 3 0",   "0 | 2 3  | 0 0 | -1 | 171 | 1 | malloc#2:16"),
    ])
