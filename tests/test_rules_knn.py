"""The nearest-neighbour rules of cal_amd/csrc/rules.hpp -- key packing with its -0 / NaN / clamp rule, eligibility and k', the
zero-norm rule, the vote count with its lowest-class majority, the chunk plan -- give their fixed vectors in a plain g++ program,
as tests/test_rules_header.py checks the older rules."""
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
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    // the key: distance first, then the row; -0 and negative residues are +0, everything non-finite is +inf
    CHECK(knn_key(0.f, 7u) == 7ull);
    CHECK(knn_key(-0.f, 7u) == 7ull && knn_key(-1e-7f, 7u) == 7ull);
    CHECK(knn_key(1.f, 0u) == 0x3F80000000000000ull);
    CHECK(knn_key(nan, 3u) == knn_key(inf, 3u) && knn_key(-inf, 3u) == knn_key(inf, 3u));
    CHECK(knn_key(inf, 3u) == 0x7F80000000000003ull && knn_key(inf, 0x7FFFFFFFu) < kKnnNone);
    const float ladder[5] = {0.f, 1e-30f, 0.5f, 3e38f, inf};
    for (int i = 0; i + 1 < 5; ++i) CHECK(knn_key(ladder[i], 0x7FFFFFFFu) < knn_key(ladder[i + 1], 0u));
    CHECK(knn_key(0.5f, 4u) < knn_key(0.5f, 5u));                    // ties: the lower row
    CHECK(knn_key_dist(knn_key(0.25f, 9u)) == 0.25f && knn_key_idx(knn_key(0.25f, 9u)) == 9);
    CHECK(knn_key_dist(knn_key(nan, 9u)) == inf);

    // distances
    CHECK(knn_dist<float>(0, 2.f, 5.f, 3.f) == 1.f && knn_dist<double>(0, 2.0, 5.0, 3.0) == 1.0);
    CHECK(knn_dist<float>(1, 4.f, 9.f, 6.f) == 0.f && knn_dist<float>(1, 4.f, 9.f, -6.f) == 2.f);
    CHECK(knn_dist<float>(1, 0.f, 9.f, 0.f) == 1.f && knn_dist<double>(1, 4.0, 0.0, 0.0) == 1.0);      // a zero row
    CHECK(knn_clamp(knn_dist<float>(0, 1.f, 1.f, 1.0000001f)) == 0.f);

    // eligibility and k'
    CHECK(knn_eligible(3, -1) && knn_eligible(3, 4) && !knn_eligible(3, 3));
    CHECK(knn_count(5, 10, -1) == 5 && knn_count(5, 10, 3) == 5 && knn_count(5, 5, 3) == 4 && knn_count(5, 5, 5) == 5);
    CHECK(knn_count(5, 4, -1) == 4 && knn_count(1, 1, 0) == 0);

    // votes
    CHECK(knn_votes_for(0, 2) && knn_votes_for(1, 2) && !knn_votes_for(2, 2) && !knn_votes_for(-1, 2));
    const int32_t tie[4] = {1, 2, 2, 0}, flat[3] = {0, 0, 0}, last[3] = {0, 1, 3};
    CHECK(knn_majority(tie, 4) == 1 && knn_majority(flat, 3) == 0 && knn_majority(last, 3) == 2);

    // the chunk plan: an override is taken as it is; the plan covers the compute units and keeps multiples of 32
    CHECK(knn_chunk_rows(128, 8000, 32) == 32 && knn_chunk_rows(128, 8000, 4096) == 4096);
    CHECK(knn_chunk_rows(8000, 8000, 0) == 4000 && knn_chunks(8000, 4000) == 2);                       // 250 query blocks x 2
    CHECK(knn_chunk_rows(128, 8000, 0) == 128 && knn_chunks(8000, 128) == 63);                         // 4 blocks x 63 chunks
    CHECK(knn_chunk_rows(1, 1, 0) == 32 && knn_chunks(1, 32) == 1);
    CHECK(knn_chunk_rows(1, 1000, 0) == 32 && knn_chunks(1000, 32) == 32);                             // no more chunks than pieces
    CHECK(knn_chunk_rows(33, 1000, 0) % 32 == 0 && knn_chunks(1000, knn_chunk_rows(33, 1000, 0)) <= 32);
    if (!failures) printf("rules ok\n");
    return failures ? 1 : 0;
}
"""


def test_knn_rules_give_their_vectors(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the shared rules cannot be checked")
    src = tmp_path / "rules_knn_check.cpp"
    exe = tmp_path / "rules_knn_check"
    src.write_text(PROGRAM)
    cmd = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "cal_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "rules ok", r.stdout + r.stderr
