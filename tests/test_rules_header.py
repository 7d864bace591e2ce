"""cal_amd/csrc/rules.hpp -- the one statement of the rules libcalhip.so and libcalhost.so share -- is plain C++: a program
that includes nothing else builds under g++ with warnings as errors and no HIP include path, and the rules give their fixed
vectors."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "rules.hpp"

#include <stdio.h>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    using namespace cal;
    CHECK(splitmix64(0ull) == 0xE220A8397B1DCDAFull);

    const float inf = __builtin_inff();
    const float ladder[5] = {-inf, -1.f, 0.f, 1.f, inf};
    for (int i = 0; i + 1 < 5; ++i) CHECK(score_key(ladder[i]) < score_key(ladder[i + 1]));
    CHECK(score_key(-0.f) == score_key(0.f));
    CHECK(score_key(__builtin_nanf("")) < score_key(-inf));

    int64_t lo, m;
    const int64_t down[2] = {5, -3}, wide[2] = {-2, 99}, empty[2] = {7, 7};
    seg_clamp(down, 0, 10, lo, m);
    CHECK(lo == 5 && m == 0);
    seg_clamp(wide, 0, 10, lo, m);
    CHECK(lo == 0 && m == 10);
    seg_clamp(empty, 0, 10, lo, m);
    CHECK(lo == 7 && m == 0);

    CHECK(sel_count(10, 3, 0.5, -1) == 5);                    // ratio * m an integer: no rounding up
    CHECK(sel_count(10, 3, 0.5000001, -1) == 6);              // just above: the next one
    CHECK(sel_count(10, 3, 0.5, 15) == 10);                   // k > m
    CHECK(sel_count(10, 3, 0.5, -2) == 3);                    // the ground-truth count

    MotifPlan q;
    const int64_t triangle[6] = {0, 1, 2, 1, 2, 0}, path[4] = {0, 1, 1, 2}, apart[4] = {0, 2, 1, 3};
    CHECK(motif_plan(triangle, 3, 0, 3, 0, 3, q) && q.k == 3 && q.edges == 3);
    CHECK(motif_plan(path, 2, 0, 2, 0, 3, q) && q.k == 3 && q.edges == 2);
    CHECK(motif_node(q, 0) == 1 && motif_parent(q, 1) == 0 && motif_parent(q, 2) == 0);   // the middle node first
    CHECK(!motif_plan(apart, 2, 0, 2, 0, 4, q));              // two disjoint edges
    CHECK(!motif_plan(path, 2, 0, 0, 0, 0, q));               // no node
    CHECK(!motif_plan(path, 2, 0, 2, 0, 9, q));               // too many nodes
    if (!failures) printf("rules ok\n");
    return failures ? 1 : 0;
}
"""


def test_rules_header_is_plain_cxx_and_gives_its_vectors(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the shared rules cannot be checked")
    src = tmp_path / "rules_check.cpp"
    exe = tmp_path / "rules_check"
    src.write_text(PROGRAM)
    cmd = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "cal_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "rules ok", r.stdout + r.stderr
