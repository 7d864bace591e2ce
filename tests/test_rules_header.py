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

    // the restriction builders' sources: one graph, nodes 0..2, columns (0,1) (1,0) (1,2) (2,1); twin pairs the reverses
    const int64_t ei[8] = {0, 1, 1, 2, 1, 0, 2, 1}, gptr[2] = {0, 3}, geptr[2] = {0, 4};
    const int32_t twin[4] = {1, 0, 3, 2};
    const int64_t rg[2] = {0, 0};
    const BatchSrc edges{ei, 4, 3, gptr, geptr, 1, rg, 0}, nodes{ei, 4, 3, gptr, geptr, 1, rg, 1};
    CHECK(occ_src(edges, rg, twin).twin == twin && occ_src(nodes, rg, twin).twin == nullptr);      // twin ignored in mode 1
    CHECK(sub_src(edges, nullptr, 0, 0, rg, rg, twin, 3).twin == twin && sub_src(nodes, nullptr, 0, 0, rg, rg, twin, 3).twin == nullptr);
    CHECK(restrict_ws_need(10, 0, 0) == 416 && restrict_ws_need(10, 7, 0) == 416 && restrict_ws_need(10, 7, 1) == 696);

    const int64_t re[2] = {-1, 1};                                    // replica 0 the control, replica 1 without node 1
    const OccSrc occ = occ_src(nodes, re, nullptr);
    const OccRep oc = replica(occ, 0), o1 = replica(occ, 1);
    CHECK(oc.nn == 3 && oc.em == 4 && node_stays(occ, oc, 0) && node_stays(occ, oc, 1) && node_stays(occ, oc, 2));
    CHECK(node_stays(occ, o1, 0) && !node_stays(occ, o1, 1) && node_stays(occ, o1, 2));
    CHECK(col_stays(occ, oc, 0) && !col_stays(occ, o1, 0) && !col_stays(occ, o1, 3));
    const int64_t ce[2] = {-1, 2};                                    // edge mode: column 2 and its twin 3 go, every node stays
    const OccSrc oce = occ_src(edges, ce, twin);
    const OccRep oe = replica(oce, 1);
    CHECK(node_stays(oce, oe, 1) && col_stays(oce, oe, 0) && col_stays(oce, oe, 1) && !col_stays(oce, oe, 2) && !col_stays(oce, oe, 3));

    const int32_t key[3] = {0, 2, 1};                                 // node keys; threshold 2 keeps the keys below it
    const int64_t crow[2] = {-1, 0}, cth[2] = {2, 2};
    CHECK(co_src(nodes, nullptr, 5, crow, cth, 0, 3).K == 0);        // no key: K forced to 0
    CHECK(co_src(BatchSrc{ei, 4, 0, gptr, geptr, 1, rg, 1}, key, 5, crow, cth, 0, 3).K == 0);   // no element: K forced to 0
    const CoSrc co = co_src(nodes, key, 1, crow, cth, 0, 3);
    CHECK(co.K == 1 && co.M == 3 && co_src(edges, key, 1, crow, cth, 0, 3).M == 4);
    const CoRep cc = replica(co, 0), c1 = replica(co, 1);
    CHECK(cc.row == nullptr && node_stays(co, cc, 0) && node_stays(co, cc, 1) && node_stays(co, cc, 2));
    CHECK(node_stays(co, c1, 0) && !node_stays(co, c1, 1) && node_stays(co, c1, 2));
    CHECK(!col_stays(co, c1, 0) && col_stays(co, cc, 0));
    CHECK(replica(co_src(nodes, key, 1, crow, cth, 0, 2), 1).nn == 0);                            // a graph longer than the map row

    const uint32_t bits[1] = {0x5u};                                  // nodes 0 and 2 present; the flip of replica 1 brings 1 back
    const int64_t srow[3] = {-1, 0, 0}, sflip[3] = {-1, -1, 1}, rg3[3] = {0, 0, 0};
    const BatchSrc nodes3{ei, 4, 3, gptr, geptr, 1, rg3, 1};
    const SubSrc sub = sub_src(nodes3, bits, 1, 1, srow, sflip, nullptr, 3);
    const SubRep sc = replica(sub, 0), s1 = replica(sub, 1), s2 = replica(sub, 2);
    CHECK(sc.all && node_stays(sub, sc, 0) && node_stays(sub, sc, 1) && node_stays(sub, sc, 2));
    CHECK(node_stays(sub, s1, 0) && !node_stays(sub, s1, 1) && node_stays(sub, s1, 2) && !col_stays(sub, s1, 0));
    CHECK(node_stays(sub, s2, 1) && col_stays(sub, s2, 0));
    const SubSrc sube = sub_src(BatchSrc{ei, 4, 3, gptr, geptr, 1, rg3, 0}, bits, 1, 1, srow, sflip, nullptr, 3);
    CHECK(node_stays(sube, replica(sube, 1), 1) && !col_stays(sube, replica(sube, 1), 1));      // edge mode: nodes stay, column 1 absent
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
