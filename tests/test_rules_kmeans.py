"""The k-means rules of cal_amd/csrc/rules.hpp -- the key and its lower-centroid tie rule, the -1 rule, the superblock plan, the
mean with its empty-cluster rule, the seeded initial rows -- restated in plain Python and checked against a plain g++ program, as
tests/test_rules_knn.py checks the nearest-neighbour rules."""
import os
import shutil
import struct
import subprocess

import pytest

from cal_amd.concepts import seed_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
MAX_SPANS = 512


# ---- the rules in plain Python ---------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def py_seed_rows(n, k, seed):
    out, x = [], seed & M64
    while len(out) < k:
        x = splitmix64(x)
        if x % n not in out:
            out.append(x % n)
    return out


def py_span(n, span_rows):
    if span_rows > 0 and span_rows % 128 == 0:
        return span_rows
    pieces = (n + 127) // 128
    return max(1, (pieces + MAX_SPANS - 1) // MAX_SPANS) * 128


def py_spans(n, span):
    return (n + span - 1) // span


def py_key(d, c):
    if d != d or d in (float("inf"), float("-inf")):
        d = float("inf")
    elif not d > 0:
        d = 0.0
    return (struct.unpack("<I", struct.pack("<f", d))[0] << 32) | c


SEEDS = [(10, 10, 1), (1000, 16, 0), (2_000_000, 64, 7), (5, 3, 2 ** 63 + 11), (64, 64, 123456789), (1, 1, 9)]
SPANS = [(1, 0), (127, 0), (128, 0), (129, 0), (65536, 0), (65537, 0), (2_000_000, 0), (2 ** 31 - 1, 0), (1000, 128), (1000, 256),
         (1000, 100), (5, 1280)]
KEYS = [(0.0, 7), (-0.0, 7), (-1e-7, 7), (1.0, 0), (0.5, 4), (0.5, 5), (float("inf"), 3), (float("nan"), 3), (3e38, 63)]

PROGRAM = r"""
#include "rules.hpp"

#include <stdio.h>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main(int argc, char** argv) {
    using namespace cal;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    // the key is knn_key: distance first, the LOWER centroid on equal distances; -0 and residues are +0, non-finite is +inf
    CHECK(kmeans_key(0.5f, 4u) < kmeans_key(0.5f, 5u) && kmeans_key(0.5f, 63u) < kmeans_key(0.75f, 0u));
    CHECK(kmeans_key(-0.f, 7u) == 7ull && kmeans_key(-1e-7f, 7u) == 7ull && kmeans_key(nan, 3u) == kmeans_key(inf, 3u));
    CHECK(kmeans_key(1.f, 2u) == knn_key(1.f, 2u));
    CHECK(knn_clamp(knn_dist<float>(0, 1.f, 1.f, 1.0000001f)) == 0.f);                     // the distance goes through the clamp
    // a row whose best key carries +inf is assigned -1
    CHECK(kmeans_assignable(kmeans_key(3e38f, 63u)) && !kmeans_assignable(kmeans_key(inf, 0u)) && !kmeans_assignable(kmeans_key(nan, 5u)));
    CHECK(kmeans_cluster(kmeans_key(2.f, 9u)) == 9 && kmeans_cluster(kmeans_key(inf, 9u)) == -1 && kmeans_cluster(kmeans_key(0.f, 0u)) == 0);
    // the mean: one rounded division; an empty cluster keeps its centroid's bits
    CHECK(kmeans_mean(10.f, 4, 99.f) == 2.5f && kmeans_mean(1.f, 3, 0.f) == 1.f / 3.f);
    const float kept = kmeans_mean(123.f, 0, -0.f);
    CHECK(float_bits(kept) == 0x80000000u && kmeans_mean(0.f, 0, 7.f) == 7.f);
    CHECK(kmeans_add(1.f, 2.f) == 3.f && kmeans_add(16777216.f, 1.f) == 16777216.f);      // plain fp32 additions
    CHECK(kKmMaxK == 64 && kKmMaxH == 256 && kKmTile == 128 && kKmMaxSpans == 512);
    // the partials workspace at the limits stays in the tens of MB
    CHECK(kKmMaxSpans * kKmMaxK * kKmMaxH * 4 == 32ll << 20);
    for (int i = 1; i + 1 < argc; i += 2) {
        if (argv[i][0] == 's') {                                      // s N span_rows -> span spans
            long long n, sr;
            sscanf(argv[i + 1], "%lld,%lld", &n, &sr);
            const int64_t span = kmeans_span(n, sr);
            printf("span %lld %lld\n", (long long)span, (long long)kmeans_spans(n, span));
        } else if (argv[i][0] == 'r') {                               // r N,K,seed -> the rows
            long long n, k;
            unsigned long long seed;
            sscanf(argv[i + 1], "%lld,%lld,%llu", &n, &k, &seed);
            int64_t out[64];
            kmeans_seed_rows(n, k, seed, out);
            printf("rows");
            for (int j = 0; j < k; ++j) printf(" %lld", (long long)out[j]);
            printf("\n");
        } else {                                                      // k bits,c -> the key
            unsigned int bits, c;
            sscanf(argv[i + 1], "%u,%u", &bits, &c);
            float d;
            memcpy(&d, &bits, 4);
            printf("key %llu\n", (unsigned long long)kmeans_key(d, c));
        }
    }
    if (!failures) printf("rules ok\n");
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the shared rules cannot be checked")
    d = tmp_path_factory.mktemp("rules_kmeans")
    src, exe = d / "rules_kmeans_check.cpp", d / "rules_kmeans_check"
    src.write_text(PROGRAM)
    cmd = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "cal_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("rules ok"), r.stdout + r.stderr
    return r.stdout.strip().splitlines()[:-1]


def test_kmeans_rules_give_their_vectors(program):
    assert _run(program, []) == []


def test_seed_rows_are_bit_equal_to_the_restatement(program):
    args = []
    for n, k, seed in SEEDS:
        args += ["r", "%d,%d,%d" % (n, k, seed)]
    lines = _run(program, args)
    for (n, k, seed), line in zip(SEEDS, lines):
        want = py_seed_rows(n, k, seed)
        assert [int(v) for v in line.split()[1:]] == want
        assert seed_rows(n, k, seed) == want and len(set(want)) == k and all(0 <= r < n for r in want)


def test_span_plan_is_the_restatement(program):
    args = []
    for n, sr in SPANS:
        args += ["s", "%d,%d" % (n, sr)]
    lines = _run(program, args)
    for (n, sr), line in zip(SPANS, lines):
        span = py_span(n, sr)
        assert [int(v) for v in line.split()[1:]] == [span, py_spans(n, span)]
        assert span % 128 == 0 and (sr or py_spans(n, span) <= MAX_SPANS)
        assert sr or span == 128 or py_spans(n, span - 128) > MAX_SPANS                 # the smallest such multiple


def test_keys_are_the_restatement(program):
    args = []
    for d, c in KEYS:
        args += ["k", "%d,%d" % (struct.unpack("<I", struct.pack("<f", d))[0], c)]
    lines = _run(program, args)
    for (d, c), line in zip(KEYS, lines):
        assert int(line.split()[1]) == py_key(d, c)
