"""The surrogate rules of cal_amd/csrc/rules.hpp -- membership with its control row and per-sample invert, the pivot rule at its
edge, the status precedence, the one-player rule, the operations every sum is made of -- checked in a plain g++ program against
their restatement in Python, as tests/test_rules_kmeans.py checks the k-means rules."""
import math
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# key rows of 4 elements, and (row, elem, thresh, invert) -> member
KEY = [[0, 1, 2, -1], [3, 3, 0, 7]]
MEMBER = [(0, 0, 0, 0), (0, 0, 1, 0), (0, 3, 0, 0), (0, 2, 2, 0), (0, 2, 3, 0), (0, 2, 3, 1), (1, 1, 3, 0), (1, 1, 3, 1), (1, 1, 4, 0),
          (-1, 0, -5, 0), (-1, 0, -5, 1), (2, 1, 0, 1), (2, 1, 0, 0), (1, 3, 1 << 40, 0), (1, 3, -(1 << 40), 1)]
# (d_j, A_jj) -> good
PIVOT = [(1.0, 1.0), (2.0 ** -30, 1.0), (2.0 ** -30 * (1 + 2.0 ** -52), 1.0), (0.0, 0.0), (0.0, 1.0), (-1e-14, 1.0), (3e-14, 1.0),
         (0.025, 1.0), (2.0 ** -41, 2.0 ** -10), (2.0 ** -40, 2.0 ** -10), (2.0 ** -39, 2.0 ** -10), (1e8, 1e18), (1e-9, 1e18),
         (float("nan"), 1.0), (1.0, float("nan")), (2.0 ** -70, 2.0 ** -40)]


def py_member(row, elem, th, inv):
    if not 0 <= row < len(KEY):
        return True
    return (KEY[row][elem] < th) != bool(inv)


def py_pivot(dj, ajj):
    return dj > ajj * 2.0 ** -30


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


PROGRAM = r"""
#include "rules.hpp"

#include <stdio.h>
#include <stdlib.h>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static double from_bits(const char* s) {
    const unsigned long long u = strtoull(s, nullptr, 10);
    double d;
    memcpy(&d, &u, 8);
    return d;
}

int main(int argc, char** argv) {
    using namespace cal;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const int32_t key[8] = {0, 1, 2, -1, 3, 3, 0, 7};
    CHECK(kSurrogateMaxDim == 128 && kSurrogateMaxPlayers == 127);
    CHECK(sur_dim(5, 0) == 5 && sur_dim(5, 1) == 6 && sur_dim(0, 1) == 1 && sur_dim(127, 1) == kSurrogateMaxDim);
    // status: too many players, then a bad sample, then rank-deficient
    CHECK(sur_status(false, false, false) == 0 && sur_status(false, false, true) == 1 && sur_status(true, false, false) == 2);
    CHECK(sur_status(false, true, false) == 3 && sur_status(true, true, true) == 2 && sur_status(false, true, true) == 3);
    // one player in mode 0 is defined, not solved
    CHECK(sur_one_player(1, 0) && !sur_one_player(1, 1) && !sur_one_player(2, 0) && !sur_one_player(0, 0));
    // samples and players the fit can use
    CHECK(sur_sample_ok(0.5, 1.0) && sur_sample_ok(-3.0, 0.0) && !sur_sample_ok(nan, 1.0) && !sur_sample_ok(inf, 1.0));
    CHECK(!sur_sample_ok(0.5, -1e-300) && !sur_sample_ok(0.5, inf) && !sur_sample_ok(0.5, nan) && sur_sample_ok(1.7976931348623157e308, 1.0));
    CHECK(sur_player_ok(0, 4) && sur_player_ok(3, 4) && !sur_player_ok(4, 4) && !sur_player_ok(-1, 4) && !sur_player_ok(0, 0));
    // y, ridge on the players' entries only
    CHECK(sur_y(0.75, 0.25, 0) == 0.5 && sur_y(0.75, 0.25, 1) == 0.75);
    CHECK(sur_ridge(2.0, 0.5, 0, 3) == 2.5 && sur_ridge(2.0, 0.5, 2, 3) == 2.5 && sur_ridge(2.0, 0.5, 3, 3) == 2.0);
    // a multiply-add is ONE rounding: 1 + 2^-53 * 2^-53 ... fma(a, a, -1) of a = 1 + 2^-30 keeps the 2^-60 a product would lose
    const double a = 1.0 + 0x1p-30;
    CHECK(sur_rhs_add(-1.0, a, a) == 0x1p-29 + 0x1p-60 && sur_sub(1.0, a, a) == -(0x1p-29 + 0x1p-60));
    CHECK(sur_gram_add(1.0, 0x1p-53) == 1.0 && sur_gram_add(0.0, 0.0) == 0.0);
    CHECK(sur_sq_add(0.0, 2.0, 3.0) == 18.0 && sur_sq_add(1.0, 0.5, -2.0) == 3.0);
    CHECK(sur_sqrt(2.0) * sur_sqrt(2.0) == 2.0000000000000004 && sur_div(1.0, 3.0) == 0.3333333333333333);
    // the constraint: x - u (sum x - Delta) / sum u; with it the corrected values sum to Delta
    CHECK(sur_correct(1.0, 0.5, 3.0, 2.0, 1.0) == 0.5 && sur_correct(2.0, 1.5, 3.0, 2.0, 1.0) == 0.5);
    // r2: NaN where the values do not vary
    CHECK(sur_r2(0.0, 2.0) == 1.0 && sur_r2(1.0, 2.0) == 0.5 && sur_r2(3.0, 2.0) == -0.5 && sur_r2(1.0, 0.0) != sur_r2(1.0, 0.0));
    for (int i = 1; i + 1 < argc; i += 2) {
        if (argv[i][0] == 'm') {                                      // m row,elem,thresh,invert -> member
            long long row, elem, th, inv;
            sscanf(argv[i + 1], "%lld,%lld,%lld,%lld", &row, &elem, &th, &inv);
            printf("member %d\n", (int)sur_member(key, 2, 4, row, elem, th, inv != 0));
        } else {                                                      // p bits(d_j) bits(A_jj) -> good
            char x[64], y[64];
            sscanf(argv[i + 1], "%63[^,],%63s", x, y);
            printf("pivot %d\n", (int)sur_pivot_ok(from_bits(x), from_bits(y)));
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
    d = tmp_path_factory.mktemp("rules_surrogate")
    src, exe = d / "rules_surrogate_check.cpp", d / "rules_surrogate_check"
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


def test_surrogate_rules_give_their_vectors(program):
    assert _run(program, []) == []


def test_membership_is_the_restatement(program):
    args = []
    for row, elem, th, inv in MEMBER:
        args += ["m", "%d,%d,%d,%d" % (row, elem, th, inv)]
    got = [int(line.split()[1]) for line in _run(program, args)]
    assert got == [int(py_member(*m)) for m in MEMBER]
    assert got[9] == got[10] == 1                                       # the control row holds every player, inverted or not


def test_pivot_rule_at_its_edge(program):
    args = []
    for dj, ajj in PIVOT:
        args += ["p", "%d,%d" % (bits(dj), bits(ajj))]
    got = [int(line.split()[1]) for line in _run(program, args)]
    assert got == [int(py_pivot(*p)) for p in PIVOT]
    # exactly 2^-30 of the diagonal is NOT good, one ulp above is; zero, negative and NaN pivots are not; the rule is relative
    assert got[:7] == [1, 0, 1, 0, 0, 0, 0] and got[7] == 1 and got[8:11] == [0, 0, 1] and got[11:13] == [0, 0] and got[13:15] == [0, 0]
    assert got[15] == 0 and math.isnan(PIVOT[13][0])
