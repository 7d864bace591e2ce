// The rules libcalhip.so (the kernels of this directory) and libcalhost.so (csrc_host/calhost.cpp) share, each stated ONCE: the
// hashes, keys, clamps, selection counts, plans and replica rules whose integer results the two libraries promise bit for bit.
// A new rule of that kind goes here first; neither side keeps a copy.
//
// Plain C++: <math.h>, <stdint.h>, <string.h> and cal_hip.h, no HIP header.  CAL_RULE is the qualifier of every function:
// host + device, always inlined under hipcc; `inline` under any other compiler.  The restriction builders' rules read the
// sources declared here; the other replica rules are templates over the argument struct: the kernels' *Args and the host's *Src
// carry the same field names (ei, E, N, ptr, eptr, B, rg, ...).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "cal_hip.h"

#if defined(__HIPCC__)
#define CAL_RULE __host__ __device__ __forceinline__
#else
#define CAL_RULE inline
#endif

namespace cal {

// ---- hashes ----------------------------------------------------------------------------------------------------------------------
// Random-intervention permutation (model.py:147-152, `random.shuffle(range(num))`) drawn on the device: graph b gets
// the key splitmix64(seed, *counter, b), the permutation is the argsort of the keys (randperm_block, common.hpp).  Also the
// hash of the noise replicas, the WL colours and the edge explainer's concrete samples.
CAL_RULE unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// 32-bit finaliser (two multiply-xorshift rounds).  Round 4: the 64-bit splitmix used before cost three 64-bit multiplies per
// decision -- ~12 quarter-rate v_mul_lo/hi_u32, ~250 cycles per wave -- and every row needs (slots + 1) x heads of them: the
// training-mode GAT kernels spent more VALU time hashing than on the softmax.  Keys are (slot id * K + head) < 2^32.
CAL_RULE uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x21F0AAADu;
    x ^= x >> 15; x *= 0x735A2D97u;
    x ^= x >> 15;
    return x;
}
// Counter-based attention-dropout keep decision for (edge slot id, head): reproducible in the backward.
CAL_RULE float keep_scale(uint64_t seed, int64_t id, int k, int K, float p, float inv_keep) {
    if (p <= 0.f) return 1.f;
    const uint32_t key = (uint32_t)(id * K + k);
    const uint32_t r = mix32(mix32(key + (uint32_t)seed) ^ (uint32_t)(seed >> 32));
    return ((float)r * (1.0f / 4294967296.0f)) >= p ? inv_keep : 0.f;
}

CAL_RULE float lrelu(float v, float slope) { return v > 0.f ? v : slope * v; }

// what one player's logit gives, all of it finite for any finite theta: with z = exp(-|theta|) in (0, 1]
//   m = sigma(theta),  dm = m (1 - m) = z / (1 + z)^2,  H(m) = softplus(theta) - theta m = log1p(z) + |theta| z / (1 + z)
// (no difference of large numbers, no logarithm of m).  One text; each side compiles it under its own flags.
struct Logit { float m, dm, ent; };
CAL_RULE Logit logit_terms(float th) {
    const float a = fabsf(th), z = expf(-a), r = 1.f / (1.f + z);
    Logit o;
    o.m = th >= 0.f ? r : z * r;
    o.dm = z * r * r;
    o.ent = log1pf(z) + a * (z * r);
    return o;
}

// ---- segments and ranking --------------------------------------------------------------------------------------------------------
// segment g of p clamped into [0, M]: [lo, lo + m); a malformed p reads nothing outside the arrays.  With hi = lo + m this is
// lo = min(max(p[g], 0), M), hi = min(max(p[g + 1], lo), M) for every p, decreasing or out of range, and every M >= 0 (every
// entry point requires that): lo <= M, so max(.., lo) followed by min(.., M) is the two-sided clamp below.
CAL_RULE void seg_clamp(const int64_t* p, int64_t g, int64_t M, int64_t& lo, int64_t& m) {
    int64_t l = p[g], h = p[g + 1];
    l = l < 0 ? 0 : (l > M ? M : l);
    h = h < l ? l : (h > M ? M : h);
    lo = l;
    m = h - l;
}

CAL_RULE uint32_t float_bits(float s) {
    uint32_t u;
    memcpy(&u, &s, 4);
    return u;
}
// 32-bit keys that order like the scores
CAL_RULE uint32_t score_key(float s) {
    if (s != s) return 1u;                                     // NaN: below every number
    const uint32_t u = s == 0.f ? 0u : float_bits(s);          // -0 ranks as +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// k_g of a segment of m elements with P positives (k >= 0: top k; -1: ceil(ratio m); -2: P)
CAL_RULE int64_t sel_count(int64_t m, int64_t P, double ratio, int64_t k) {
    if (k >= 0) return k < m ? k : m;
    if (k == -1) {
        const double c = ceil(ratio * (double)m);
        return c < (double)m ? (int64_t)c : m;
    }
    return P;
}
// ... of the n elements of a segment that take part in a rank agreement (k >= 0: top k; else ceil(ratio n))
CAL_RULE int64_t ag_sel_count(int64_t n, double ratio, int64_t k) {
    if (k >= 0) return k < n ? k : n;
    const double c = ceil(ratio * (double)n);
    return c < (double)n ? (int64_t)c : n;
}

// ROC-AUC of a segment of m elements from r2 = 2 x the sum of the positives' 1-based ascending average ranks
CAL_RULE double seg_auc(int64_t m, int64_t P, int64_t r2) {
    if (P <= 0 || P >= m) return __builtin_nan("");
    return ((double)r2 * 0.5 - (double)P * (double)(P + 1) * 0.5) / ((double)P * (double)(m - P));
}

// key of the column (u, v) of a graph of nn nodes, x = u - nlo, y = v - nlo its local ends: the undirected edge, then the
// direction (rev: u > v)
CAL_RULE uint64_t und_edge_key(uint64_t x, uint64_t y, uint64_t nn, bool rev) {
    return (((x < y ? x : y) * nn + (x < y ? y : x)) << 1) | (uint64_t)rev;
}

// ---- the parametric edge explainer -----------------------------------------------------------------------------------------------
// column e of a player: in range, with both end nodes in range
CAL_RULE bool column_ok(int64_t e, const int32_t* __restrict__ row32, const int32_t* __restrict__ col32, int64_t E, int64_t N,
                        int& u, int& v) {
    u = v = 0;
    if (e < 0 || e >= E) return false;
    u = row32[e];
    v = col32[e];
    return u >= 0 && u < N && v >= 0 && v < N;
}

// nodes of one workgroup of the row kernel: 16 at the least, at most 512 workgroups
CAL_RULE int mlp_rows_per_block(int64_t N) {
    const int64_t rpb = (N + 511) / 512;
    return (int)(rpb < 16 ? 16 : rpb);
}

CAL_RULE bool mlp_sizes_ok(int64_t N, int64_t E, int64_t Hd, int64_t B, int64_t P) {
    return N >= 0 && E >= 0 && B >= 0 && P >= 0 && N < (1ll << 31) && E < (1ll << 31) && B < (1ll << 31) && P < (1ll << 31) &&
           Hd >= 4 && Hd <= 256 && Hd % 4 == 0;
}

// ---- Weisfeiler-Lehman colours ---------------------------------------------------------------------------------------------------
constexpr unsigned long long kWlInit = CAL_WL_C_INIT, kWlSelf = CAL_WL_C_SELF, kWlOut = CAL_WL_C_OUT, kWlIn = CAL_WL_C_IN,
                             kWlNode = CAL_WL_C_NODE, kWlGraph = CAL_WL_C_GRAPH;

// the next colour of a node
CAL_RULE unsigned long long wl_next(unsigned long long c, unsigned long long so, unsigned long long si) {
    return splitmix64(splitmix64(splitmix64(c + kWlSelf) + so) + si);
}

// ---- the batch builders: replica r -> node range [nlo, nlo + nn), column range [elo, elo + em) (all zero without a graph), and
// which of the graph's columns / elements stay.  A: the sources below for the restriction builders, NoArgs / NoiseSrc, Side /
// SpliceSide.

// The restriction builders (occlusion, coalitions, subsets): replica r is graph rg[r] of the batch with some of its elements
// left out.  Mode 0: every node stays; mode 1: the nodes that stay are renumbered densely and a column stays iff both ends stay.
// A column that leaves its graph is dropped.  Each rule is a source -- the batch and what the rule reads, made by its maker,
// which both libraries call -- and three overloads on it: replica(s, r), node_stays(s, q, l) for LOCAL node l of the replica's
// graph, col_stays(s, q, e) for column e of it.  A new rule is a source, a maker and these three.
struct BatchSrc {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    int64_t B;
    const int64_t* rg;         // [R] graph of every replica (outside [0, B): none)
    int mode;                  // 0 edges, 1 nodes
};

// bytes of ws of R replicas: two counts each, and in mode 1 a map row of max_nodes ids each (occlusion has no map: max_nodes = 0)
CAL_RULE int64_t restrict_ws_need(int64_t R, int64_t max_nodes, int mode) {
    R = R > 0 ? R : 0;
    return 16 * R + (mode == 1 ? 4 * R * (max_nodes > 0 ? max_nodes : 0) : 0) + 256;
}

// occlusion: the node removed (rn) and the columns removed (c0, c1); -1 = none, which equals no id
struct OccSrc : BatchSrc {
    const int64_t* re;         // [R] the element removed (global column / node id; not one of the graph's: nothing)
    const int32_t* twin;       // [E] or null
};
struct OccRep {
    int64_t nlo, nn, elo, em, rn, c0, c1;
};

// (a twin map pairs columns: it counts in mode 0 only)
CAL_RULE OccSrc occ_src(const BatchSrc& b, const int64_t* rep_elem, const int32_t* twin) {
    return OccSrc{b, rep_elem, b.mode == 0 ? twin : nullptr};
}

CAL_RULE OccRep replica(const OccSrc& a, int64_t r) {
    OccRep q{0, 0, 0, 0, -1, -1, -1};
    const int64_t g = a.rg[r];
    if (g < 0 || g >= a.B) return q;
    seg_clamp(a.ptr, g, a.N, q.nlo, q.nn);
    seg_clamp(a.eptr, g, a.E, q.elo, q.em);
    const int64_t e = a.re[r];
    if (a.mode == 0) {
        if (e >= q.elo && e < q.elo + q.em) {
            q.c0 = e;
            if (a.twin) q.c1 = a.twin[e];                         // (a negative twin or one outside the graph meets no column)
        }
    } else if (e >= q.nlo && e < q.nlo + q.nn) {
        q.rn = e;
    }
    return q;
}

// LOCAL node l of the replica's graph stays
CAL_RULE bool node_stays(const OccSrc&, const OccRep& q, int64_t l) { return q.nlo + l != q.rn; }

// column e of the replica's graph stays
CAL_RULE bool col_stays(const OccSrc& a, const OccRep& q, int64_t e) {
    const int64_t u = a.ei[e], v = a.ei[a.E + e];
    return u >= q.nlo && u < q.nlo + q.nn && v >= q.nlo && v < q.nlo + q.nn && e != q.c0 && e != q.c1 && u != q.rn && v != q.rn;
}

// coalitions: the replica's key row (null: everything stays) and threshold.  In mode 1 a graph with more nodes than the map's row
// length (mx) has no replica either.
struct CoSrc : BatchSrc {
    const int32_t* key;        // [K, M], M = E (mode 0) or N (mode 1)
    int64_t K, M;
    const int64_t* rrow;       // [R] key row of every replica (outside [0, K): everything stays)
    const int64_t* rth;        // [R] threshold
    int invert;                // 0: key < threshold stays, 1: key >= threshold stays
    int64_t mx;                // (mode 1) the map's row length: bounds every graph's node count
};
struct CoRep {
    int64_t nlo, nn, elo, em, th;
    const int32_t* row;
};

// (no key entry: K = 0, every replica keeps everything there is)
CAL_RULE CoSrc co_src(const BatchSrc& b, const int32_t* key, int64_t K, const int64_t* rep_row, const int64_t* rep_thresh, int invert,
                      int64_t max_nodes) {
    const int64_t M = b.mode == 0 ? b.E : b.N;
    return CoSrc{b, key, key && M > 0 ? K : 0, M, rep_row, rep_thresh, invert, max_nodes};
}

CAL_RULE CoRep replica(const CoSrc& a, int64_t r) {
    CoRep q{0, 0, 0, 0, 0, nullptr};
    const int64_t g = a.rg[r];
    if (g < 0 || g >= a.B) return q;
    seg_clamp(a.ptr, g, a.N, q.nlo, q.nn);
    seg_clamp(a.eptr, g, a.E, q.elo, q.em);
    if (a.mode == 1 && q.nn > a.mx) {
        q.nlo = q.nn = q.elo = q.em = 0;
        return q;
    }
    const int64_t k = a.rrow[r];
    if (k >= 0 && k < a.K) q.row = a.key + k * a.M;
    q.th = a.rth[r];
    return q;
}

// element e (a column in mode 0, a node in mode 1; inside [0, M)) stays in the replica
CAL_RULE bool elem_stays(const CoSrc& a, const CoRep& q, int64_t e) {
    if (!q.row) return true;
    const int64_t k = q.row[e];
    return a.invert ? k >= q.th : k < q.th;
}

// LOCAL node l of the replica's graph stays
CAL_RULE bool node_stays(const CoSrc& a, const CoRep& q, int64_t l) { return a.mode == 0 || elem_stays(a, q, q.nlo + l); }

// column e of the replica's graph stays
CAL_RULE bool col_stays(const CoSrc& a, const CoRep& q, int64_t e) {
    const int64_t u = a.ei[e], v = a.ei[a.E + e];
    if (!(u >= q.nlo && u < q.nlo + q.nn && v >= q.nlo && v < q.nlo + q.nn)) return false;
    return a.mode == 0 ? elem_stays(a, q, e) : elem_stays(a, q, u) && elem_stays(a, q, v);
}

// subsets: the replica's bitset row over its own graph's elements (all: no row, everything present) and the LOCAL indices its
// flip toggles (f0 the flip, f1 its twin column; -1: none).  The elements are the graph's columns in mode 0, its nodes in mode 1.
struct SubSrc : BatchSrc {
    const uint32_t* bits;      // [K, W]
    int64_t K, W;
    const int64_t* rrow;       // [R] bitset row of every replica (outside [0, K): everything present)
    const int64_t* rflip;      // [R] local index toggled (outside the graph's elements: none)
    const int32_t* twin;       // [E] or null
    int64_t mx;                // (mode 1) the map's row length: bounds every graph's node count
};
struct SubRep {
    int64_t nlo, nn, elo, em, f0, f1;
    const uint32_t* row;
    bool all;
};

// (a twin map pairs columns: it counts in mode 0 only)
CAL_RULE SubSrc sub_src(const BatchSrc& b, const uint32_t* bits, int64_t K, int64_t W, const int64_t* rep_row,
                        const int64_t* rep_flip, const int32_t* twin, int64_t max_nodes) {
    return SubSrc{b, bits, K, W, rep_row, rep_flip, b.mode == 0 ? twin : nullptr, max_nodes};
}

// bit j of a row of W words: a local index >= 32 W is absent
CAL_RULE bool bit_at(const uint32_t* row, int64_t W, int64_t j) {
    if (j < 0 || j >= 32 * W) return false;
    return (row[j >> 5] >> (j & 31)) & 1u;
}

// the local indices a flip toggles in a segment of m elements that starts at global element lo: f itself when inside [0, m), and
// (twin given, a column segment) the twin column when it lies inside the segment and is another column than f
CAL_RULE void flip_pair(int64_t f, int64_t lo, int64_t m, const int32_t* twin, int64_t& f0, int64_t& f1) {
    f0 = f1 = -1;
    if (f < 0 || f >= m) return;
    f0 = f;
    if (twin) {
        const int64_t t = (int64_t)twin[lo + f] - lo;
        if (t >= 0 && t < m && t != f) f1 = t;
    }
}

CAL_RULE SubRep replica(const SubSrc& a, int64_t r) {
    SubRep q{0, 0, 0, 0, -1, -1, nullptr, true};
    const int64_t g = a.rg[r];
    if (g < 0 || g >= a.B) return q;
    seg_clamp(a.ptr, g, a.N, q.nlo, q.nn);
    seg_clamp(a.eptr, g, a.E, q.elo, q.em);
    if (a.mode == 1 && q.nn > a.mx) {
        q.nlo = q.nn = q.elo = q.em = 0;
        return q;
    }
    const int64_t k = a.rrow[r];
    if (k >= 0 && k < a.K) {
        q.row = a.bits + k * a.W;
        q.all = false;
    }
    if (a.mode == 0) flip_pair(a.rflip[r], q.elo, q.em, a.twin, q.f0, q.f1);
    else flip_pair(a.rflip[r], q.nlo, q.nn, nullptr, q.f0, q.f1);
    return q;
}

// LOCAL element j (a column of the graph in mode 0, a node in mode 1) stays in the replica: its bit after the toggle
CAL_RULE bool elem_stays(const SubSrc& a, const SubRep& q, int64_t j) {
    return (q.all || bit_at(q.row, a.W, j)) != (j == q.f0 || j == q.f1);
}

// LOCAL node l of the replica's graph stays
CAL_RULE bool node_stays(const SubSrc& a, const SubRep& q, int64_t l) { return a.mode == 0 || elem_stays(a, q, l); }

// column e of the replica's graph stays
CAL_RULE bool col_stays(const SubSrc& a, const SubRep& q, int64_t e) {
    const int64_t u = a.ei[e], v = a.ei[a.E + e];
    if (!(u >= q.nlo && u < q.nlo + q.nn && v >= q.nlo && v < q.nlo + q.nn)) return false;
    return a.mode == 0 ? elem_stays(a, q, e - q.elo) : elem_stays(a, q, u - q.nlo) && elem_stays(a, q, v - q.nlo);
}

// ---- the beam step (cal_beam_step): all integer.  Graph g's states are the rows [g beam, g beam + n_state[g]) of bits; a
// candidate c is (rep_row[c], rep_flip[c]) with its replica's p[c] and flipped[c].  A: BeamArgs / BeamSrc (beam, nst, rrow, rflip, p,
// flipped).
constexpr int kBeamMax = 16;                         // states of a graph
constexpr int kBeamWords = 64;                       // words of a state: 2048 local elements

// the parent of candidate c of graph g: its slot in [0, beam) among g's live states, or `beam`: the full set (a row that is none
// of them)
template <class A>
CAL_RULE int beam_parent(const A& a, int64_t g, int64_t c) {
    const int64_t s = a.rrow[c] - g * (int64_t)a.beam;
    int64_t n = a.nst[g];
    n = n < 0 ? 0 : (n > a.beam ? a.beam : n);
    return s >= 0 && s < n ? (int)s : a.beam;
}

// word w of the full set of a segment of m elements in W words
CAL_RULE uint32_t full_word(int64_t m, int64_t W, int64_t w) {
    const int64_t n = m < 32 * W ? m : 32 * W, lo = 32 * w;
    if (n <= lo) return 0u;
    return n - lo >= 32 ? 0xFFFFFFFFu : (1u << (n - lo)) - 1u;
}

// what the flips f0, f1 (local, -1: none; an index >= 32 W toggles nothing) toggle in word w
CAL_RULE uint32_t flip_word(int64_t f0, int64_t f1, int64_t w) {
    uint32_t x = 0u;
    if (f0 >= 0 && (f0 >> 5) == w) x ^= 1u << (f0 & 31);
    if (f1 >= 0 && (f1 >> 5) == w) x ^= 1u << (f1 & 31);
    return x;
}

// the 64-bit head of a candidate's place in the order: flipped first, then score_key(p) ascending (smaller sorts first)
CAL_RULE uint64_t beam_head(uint8_t flipped, float p) { return ((uint64_t)(flipped ? 0u : 1u) << 32) | (uint64_t)score_key(p); }

// candidate i comes before candidate j: (flipped first, score_key(p) ascending, rep_row ascending, rep_flip ascending), and two
// candidates that agree in all four in index order.  h: beam_head, r: rep_row, f: rep_flip.
CAL_RULE bool beam_before(uint64_t hi, int64_t ri, int64_t fi, int64_t i, uint64_t hj, int64_t rj, int64_t fj, int64_t j) {
    if (hi != hj) return hi < hj;
    if (ri != rj) return ri < rj;
    if (fi != fj) return fi < fj;
    return i < j;
}
template <class A>
CAL_RULE bool beam_before(const A& a, int64_t i, int64_t j) {
    return beam_before(beam_head(a.flipped[i], a.p[i]), a.rrow[i], a.rflip[i], i, beam_head(a.flipped[j], a.p[j]), a.rrow[j],
                       a.rflip[j], j);
}

// structural noise: H(s, i), the replica's seed, deletion threshold and a = max(rep_add, 0)
constexpr unsigned long long kNoiseDel = CAL_NOISE_C_DEL, kNoiseAdd = CAL_NOISE_C_ADD;

CAL_RULE unsigned long long noise_hash(unsigned long long s, unsigned long long i) { return splitmix64(splitmix64(s) + i); }

struct NoRep {
    int64_t nlo, nn, elo, em, del, a;
    unsigned long long seed;
};

template <class A>
CAL_RULE NoRep noise_replica(const A& a, int64_t r) {
    NoRep q{0, 0, 0, 0, 0, 0, 0};
    const int64_t add = a.radd[r];
    q.a = add > 0 ? add : 0;
    const int64_t g = a.rg[r];
    if (g < 0 || g >= a.B) return q;
    seg_clamp(a.ptr, g, a.N, q.nlo, q.nn);
    seg_clamp(a.eptr, g, a.E, q.elo, q.em);
    q.seed = (unsigned long long)a.rseed[r];
    q.del = a.rdel[r];
    return q;
}

// column e of the replica's graph stays: inside the node range, and a self loop or its player not deleted
template <class A>
CAL_RULE bool noise_stays(const A& a, const NoRep& q, int64_t e) {
    const int64_t u = a.ei[e], v = a.ei[a.E + e];
    if (!(u >= q.nlo && u < q.nlo + q.nn && v >= q.nlo && v < q.nlo + q.nn)) return false;
    if (u == v || q.del <= 0) return true;
    int64_t rep = e;
    if (a.twin) {                                                  // the lower column of a pair (a twin outside the segment: none)
        const int64_t t = a.twin[e];
        if (t >= q.elo && t < e) rep = t;
    }
    return !((int64_t)(noise_hash(q.seed ^ kNoiseDel, (unsigned long long)(rep - q.elo)) >> 1) < q.del);
}

// the key of the pair (u, v) of local ids of a graph of n nodes
CAL_RULE uint64_t pair_key(bool undirected, uint64_t u, uint64_t v, uint64_t n) {
    return undirected ? (u < v ? u * n + v : v * n + u) : u * n + v;
}

// splice: the part of pair p on side s; all zero when absent
template <class S>
CAL_RULE void side_ranges(const S& s, int64_t p, int64_t& nlo, int64_t& nn, int64_t& elo, int64_t& em) {
    const int64_t g = s.pick[p];
    nlo = nn = elo = em = 0;
    if (g < 0 || g >= s.B) return;
    seg_clamp(s.ptr, g, s.N, nlo, nn);
    seg_clamp(s.eptr, g, s.E, elo, em);
}

template <class S>
CAL_RULE bool col_valid(const S& s, int64_t e, int64_t nlo, int64_t nn) {
    const int64_t u = s.ei[e], v = s.ei[s.E + e];
    return u >= nlo && u < nlo + nn && v >= nlo && v < nlo + nn;
}

// ---- exact motif matching --------------------------------------------------------------------------------------------------------
constexpr int kMotifN = CAL_MOTIF_MAX_NODES;         // nodes of a target graph, rows of the bit matrix
constexpr int kMotifK = CAL_MOTIF_MAX_PATTERN;
static_assert(kMotifN == 256 && kMotifK == 8, "a node id is one byte of the key, a row four 64-bit words");

// one pattern, planned.  Positions are the places of the match order.
struct MotifPlan {
    unsigned long long order;   // byte d: pi[d], the pattern node of position d
    unsigned long long padj;    // byte d: bit j set iff pi[d] and pi[j] are adjacent
    uint32_t parent;            // bits [3d, 3d + 3): the parent position of position d >= 1
    int32_t k;                  // nodes
    int64_t lo;                 // first node of the pattern in pat_labels
    int64_t edges;              // adjacent unordered pairs
};
CAL_RULE int motif_node(const MotifPlan& q, int d) { return (int)((q.order >> (8 * d)) & 0xFF); }
CAL_RULE unsigned motif_adj(const MotifPlan& q, int d) { return (unsigned)(q.padj >> (8 * d)) & 0xFFu; }
CAL_RULE int motif_parent(const MotifPlan& q, int d) { return (int)(q.parent >> (3 * d)) & 7; }

// A pattern's plan from its columns; false: no node, too many nodes or not connected.
CAL_RULE bool motif_plan(const int64_t* ei, int64_t PE, int64_t elo, int64_t ehi, int64_t nlo, int64_t k, MotifPlan& q) {
    if (k < 1 || k > kMotifK) return false;
    unsigned adj[kMotifK] = {};
    for (int64_t e = elo; e < ehi; ++e) {
        const int64_t u = ei[e] - nlo, v = ei[PE + e] - nlo;
        if (u < 0 || u >= k || v < 0 || v >= k || u == v) continue;
        adj[u] |= 1u << v;
        adj[v] |= 1u << u;
    }
    int pi[kMotifK], edges = 0;
    unsigned placed = 0;
    for (int d = 0; d < k; ++d) {
        int bestn = -1, bests = -1;
        for (int i = 0; i < k; ++i) {
            if (placed >> i & 1u) continue;
            const int s = __builtin_popcount(d ? adj[i] & placed : adj[i]);
            if (s > bests) {
                bests = s;
                bestn = i;
            }
        }
        if (d && bests == 0) return false;                            // not connected
        pi[d] = bestn;
        placed |= 1u << bestn;
    }
    q.order = 0;
    q.padj = 0;
    q.parent = 0;
    for (int d = 0; d < k; ++d) {
        q.order |= (unsigned long long)pi[d] << (8 * d);
        int par = -1;
        for (int j = 0; j < k; ++j)
            if (adj[pi[d]] >> pi[j] & 1u) {
                q.padj |= 1ull << (8 * d + j);
                if (par < 0 && j < d) par = j;
            }
        if (d) q.parent |= (uint32_t)par << (3 * d);
        edges += __builtin_popcount(adj[d]);
    }
    q.k = (int32_t)k;
    q.lo = nlo;
    q.edges = edges / 2;
    return true;
}

// the key of an embedding: the images img[d] of the positions as bytes in pattern-node order, node 0 in the top byte, the bytes
// of the nodes k .. 7 0xFF
CAL_RULE unsigned long long motif_key(const MotifPlan& q, const int* img) {
    unsigned long long key = q.k < kMotifK ? ~0ull >> (8 * q.k) : 0ull;
    for (int d = 0; d < q.k; ++d) key |= (unsigned long long)img[d] << (56 - 8 * motif_node(q, d));
    return key;
}

// ---- graph centralities (cal_centrality) -----------------------------------------------------------------------------------------
// Sources are dealt to kCentW "waves" statically: source s belongs to wave s mod kCentW, a wave takes its sources in ascending
// s and keeps ONE partial sum per output element; the partials are added in wave order, ((p0 + p1) + p2) + p3.  On the host a
// wave is a loop index.
constexpr int kCentW = 4;
static_assert(kCentW == 4, "cent_join adds four partials");
constexpr int kCentUnreached = -1;                   // hop distance of a node the search did not reach (also what `hop` reports)
constexpr int kCentHopSeed = 0;                      // `hop` of a marked node
constexpr int64_t kCentSkipInt = -1;                 // every integer output of a skipped graph; the fp64 outputs are NaN
constexpr int kCentSlots = 256;                      // slots of cent_tree_sum

CAL_RULE int cent_wave(int64_t s) { return (int)(s % kCentW); }
CAL_RULE double cent_skip_f64() { return __builtin_nan(""); }
CAL_RULE double cent_join(double p0, double p1, double p2, double p3) { return ((p0 + p1) + p2) + p3; }

// what a node v one level above u pulls from u, in ascending u: sigma(v) * q(u) with q(u) = (1 + delta(u)) / sigma(u); the same
// product is the term of the edge {v, u}
CAL_RULE double cent_q(double delta, double sigma) { return (1.0 + delta) / sigma; }

// The sum of v[0 .. n) PageRank uses (dangling mass, L1 change): slot i & 255 takes v[i] in ascending i, then the 256 slots are
// halved, s[i] += s[i + h] for h = 128, 64, .. 1.  s: kCentSlots doubles, destroyed.  (On the device the halvings of h <= 32 are
// the xor butterfly of a wave, which gives every lane the bits of s[0].)
CAL_RULE double cent_tree_sum(double* s) {
    for (int h = kCentSlots / 2; h > 0; h >>= 1)
        for (int i = 0; i < h; ++i) s[i] += s[i + h];
    return s[0];
}

// one PageRank step of a node: pull = the sum of x[u] / deg[u] over its neighbours u in ascending id, dangling = the tree sum of
// x over the nodes without a neighbour, n the graph's nodes
// One operation per statement: the device build contracts a * b + c inside a statement, and pr_iters is promised bit for bit.
CAL_RULE double cent_pr_step(double alpha, double pull, double dangling, double n) {
    const double t = pull + dangling / n;
    const double a = alpha * t;
    const double b = (1.0 - alpha) / n;
    return a + b;
}
// the stopping test: err = the tree sum of |x_new - x_old|.  The step that meets it is counted in pr_iters.
CAL_RULE bool cent_pr_done(double err, double tol) { return err < tol; }

// ---- nearest neighbours in embedding space (cal_knn) -----------------------------------------------------------------------------
constexpr int kKnnMaxK = 64, kKnnMaxH = 256, kKnnMaxC = 64;     // limits of the device library
constexpr int kKnnQB = 32;                                      // queries of a workgroup
constexpr int kKnnCUs = 256;                                    // compute units the chunk plan spreads over
constexpr uint64_t kKnnNone = ~0ull;                            // no neighbour: above every key (an index is below 2^31)

// the distance of a pair from the two squared norms and the dot product (T: float on the device, double on the host).
// metric 0: squared Euclidean; 1: cosine distance, 1 where either row has norm zero.  The clamp is part of the key.
CAL_RULE float knn_sqrt(float v) { return sqrtf(v); }
CAL_RULE double knn_sqrt(double v) { return sqrt(v); }
template <class T>
CAL_RULE T knn_dist(int metric, T qn, T xn, T dot) {
    if (metric == 0) return (qn + xn) - (T)2 * dot;
    if (qn == (T)0 || xn == (T)0) return (T)1;
    return (T)1 - dot / (knn_sqrt(qn) * knn_sqrt(xn));
}

// the distance as it is ordered and reported: a non-finite one is +inf (last), anything else not above zero (-0, a negative
// rounding residue) is +0.  A distance is then >= +0, and its bits order like its value.
CAL_RULE float knn_clamp(float d) {
    if (d != d || d == __builtin_inff() || d == -__builtin_inff()) return __builtin_inff();
    return d > 0.f ? d : 0.f;
}
// the total order of a query's candidates: distance first, the lower bank row on equal distances
CAL_RULE uint64_t knn_key(float d, uint32_t idx) { return ((uint64_t)float_bits(knn_clamp(d)) << 32) | (uint64_t)idx; }
CAL_RULE float knn_key_dist(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    float d;
    memcpy(&d, &u, 4);
    return d;
}
CAL_RULE int32_t knn_key_idx(uint64_t key) { return (int32_t)(uint32_t)key; }

// bank row j may be returned for a query whose skipped row is skip (a skip outside [0, M) meets no row)
CAL_RULE bool knn_eligible(int64_t j, int64_t skip) { return j != skip; }
// k' of a query: the neighbours it gets
CAL_RULE int64_t knn_count(int64_t k, int64_t M, int64_t skip) {
    const int64_t n = M - ((skip >= 0 && skip < M) ? 1 : 0);
    return k < n ? k : n;
}
// a neighbour's label counts for class `label` iff it lies in [0, C)
CAL_RULE bool knn_votes_for(int64_t label, int64_t C) { return label >= 0 && label < C; }
// the majority of a vote row: the lowest class among the most voted (0 for C = 0)
CAL_RULE int knn_majority(const int32_t* votes, int C) {
    int best = 0;
    for (int c = 1; c < C; ++c)
        if (votes[c] > votes[best]) best = c;
    return best;
}

// the chunk plan: rows of a bank chunk, a multiple of 32.  A positive multiple of 32 given by the caller is taken as it is;
// otherwise enough chunks that query blocks x chunks cover the compute units, as far as the bank has 32-row pieces.
CAL_RULE int64_t knn_chunk_rows(int64_t nq, int64_t M, int64_t chunk_rows) {
    if (chunk_rows > 0 && chunk_rows % 32 == 0) return chunk_rows;
    const int64_t qb = (nq + kKnnQB - 1) / kKnnQB, pieces = (M + 31) / 32;
    int64_t want = qb > 0 ? (kKnnCUs + qb - 1) / qb : 1;
    want = want < 1 ? 1 : (want > pieces ? pieces : want);
    return ((pieces + want - 1) / want) * 32;
}
CAL_RULE int64_t knn_chunks(int64_t M, int64_t rows) { return (M + rows - 1) / rows; }

// ---- k-means on embedding rows (cal_kmeans, cal_kmeans_assign) -------------------------------------------------------------------
constexpr int kKmMaxK = 64, kKmMaxH = 256;                      // limits of the device library
constexpr int kKmTile = 128;                                    // a superblock is a multiple of this many rows
// superblocks of the default plan.  A superblock's partial is K x H floats (+ K counts, an fp64 inertia, a moved count): at the
// device limits (K = 64, H = 256) 512 x 64 KB = 32 MB of partial sums (+ 136 KB for the rest), whatever N is.
constexpr int64_t kKmMaxSpans = 512;

// the distance of a row to a centroid: knn_dist(0, xn, cn, dot) through knn_clamp, the norms ONE ascending fmaf chain each (the
// device) or fp64 sums (the host, rounded once).  The key orders a row's centroids: distance first, the LOWER centroid on ties.
CAL_RULE uint64_t kmeans_key(float d, uint32_t c) { return knn_key(d, c); }
// a row whose nearest key carries +inf (every distance non-finite) is assigned -1: no sum, no count, no inertia
CAL_RULE bool kmeans_assignable(uint64_t best_key) { return knn_key_dist(best_key) != __builtin_inff(); }
CAL_RULE int32_t kmeans_cluster(uint64_t best_key) { return kmeans_assignable(best_key) ? knn_key_idx(best_key) : -1; }

// rows of a superblock: the caller's positive multiple of 128 as it is; for 0 the smallest multiple of 128 that leaves at most
// kKmMaxSpans superblocks.  The order of sums below is by superblock, so the BITS of the centroids depend on this value.
CAL_RULE int64_t kmeans_span(int64_t N, int64_t span_rows) {
    if (span_rows > 0 && span_rows % kKmTile == 0) return span_rows;
    const int64_t pieces = (N + kKmTile - 1) / kKmTile;
    const int64_t per = (pieces + kKmMaxSpans - 1) / kKmMaxSpans;
    return (per < 1 ? 1 : per) * kKmTile;
}
CAL_RULE int64_t kmeans_spans(int64_t N, int64_t span) { return (N + span - 1) / span; }

// Order of sums.  The partial of superblock s for (c, h) is ONE chain of plain fp32 additions over the rows of s assigned to c,
// in ascending row order, from +0; a cluster's sum is the partials added in ascending s (from the partial of s = 0); counts are
// integers.  The inertia is fp64: a superblock's chain over its assigned rows' fp32 distances in ascending row order from 0,
// then the superblocks in ascending s.
CAL_RULE float kmeans_add(float acc, float v) { return acc + v; }
// the new centroid coordinate: the mean, correctly rounded division; an empty cluster keeps its centroid's bits
CAL_RULE float kmeans_mean(float sum, int64_t count, float old) { return count ? sum / (float)count : old; }

// the K distinct initial rows of a seed: a splitmix64 walk x <- splitmix64(x) from x = seed, row x mod N, repeats rejected.
// Needs 1 <= K <= N.  All integer.
CAL_RULE void kmeans_seed_rows(int64_t N, int64_t K, uint64_t seed, int64_t* out) {
    unsigned long long x = seed;
    for (int64_t i = 0; i < K;) {
        x = splitmix64(x);
        const int64_t r = (int64_t)(x % (unsigned long long)N);
        bool seen = false;
        for (int64_t j = 0; j < i; ++j) seen = seen || out[j] == r;
        if (!seen) out[i++] = r;
    }
}

// ---- surrogate attributions: one weighted least-squares fit per graph (cal_surrogate_fit) ----------------------------------------
// Graph g has the players pl_elem[pl_ptr[g] .. pl_ptr[g + 1]) (n of them, seg_clamp into [0, P]) and the samples rep_ptr[g] ..
// rep_ptr[g + 1] (S of them, seg_clamp into [0, R]).  Mode 0 ("shap"): d = n unknowns, y_s = v_s - v_empty[g], the solution of
// A x = b corrected onto sum(phi) = Delta = v_full[g] - v_empty[g].  Mode 1 ("lime"): d = n + 1, the intercept the LAST unknown
// (its z is 1 in every sample), y_s = v_s, ridge on the first n diagonal entries only.
//
// Every floating-point operation is one of the functions below, so both libraries perform the same operations in the same order:
// a multiply-add is __builtin_fma (never an a * b + c expression, which one compiler contracts and the other does not), a sum of
// weights a plain add.  Terms whose z is 0 are SKIPPED, not added as zeros.
//   Gram          A_ij = the chain of sur_gram_add(., w_s) over ascending s with z_si and z_sj, from +0; then sur_ridge on A_ii
//   right side    b_i  = the chain of sur_rhs_add(., w_s, y_s) over ascending s with z_si, from +0
//   Cholesky      left-looking.  d_j = the chain of sur_sub(., L_jk, L_jk) over ascending k < j from A_jj; column j is good iff
//                 sur_pivot_ok(d_j, A_jj) (A_jj with its ridge); L_jj = sur_sqrt(d_j);
//                 L_ij = sur_div(the chain of sur_sub(., L_ik, L_jk) over ascending k < j from A_ij, L_jj)
//   forward       y_i = sur_div(the chain of sur_sub(., L_ik, y_k) over ASCENDING k < i from b_i, L_ii), i ascending
//   back          x_i = sur_div(the chain of sur_sub(., L_ki, x_k) over DESCENDING k > i from y_i, L_ii), i descending
//   u             the same two substitutions from the right side of ones (mode 0)
//   sums          sum(x), sum(u): plain adds over ascending i from +0
//   phi           mode 0: sur_correct(x_i, u_i, sum(x), sum(u), Delta), phi0 = v_empty[g];  mode 1: x_i, phi0 = x_n
//   weighted R^2  sw = the chain of sur_gram_add(., w_s), swv = the chain of sur_rhs_add(., w_s, v_s), mean = sur_div(swv, sw);
//                 fit_s = the chain of plain adds of phi_p over ascending p with z_sp, from phi0; SSR = the chain of
//                 sur_sq_add(., w_s, v_s - fit_s), SST = the chain of sur_sq_add(., w_s, v_s - mean), all over ascending s from +0;
//                 r2 = sur_r2(SSR, SST)
constexpr int kSurrogateMaxDim = 128;                           // the largest matrix dimension d of the device library
constexpr int kSurrogateMaxPlayers = 127;                       // the largest player count n of the device library

// z(s, p) of sample s for the player whose representative is element elem (inside [0, M)): a key row outside [0, K) is the
// control sample of coalition_batch, every player present whatever invert says
CAL_RULE bool sur_member(const int32_t* key, int64_t K, int64_t M, int64_t row, int64_t elem, int64_t thresh, bool invert) {
    if (row < 0 || row >= K) return true;
    return ((int64_t)key[row * M + elem] < thresh) != invert;
}
CAL_RULE bool sur_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }
// a sample the fit can use: a finite value, a finite weight >= 0
CAL_RULE bool sur_sample_ok(double v, double w) { return sur_finite(v) && sur_finite(w) && w >= 0.0; }
// a player the fit can use: its representative names an element
CAL_RULE bool sur_player_ok(int64_t elem, int64_t M) { return elem >= 0 && elem < M; }
CAL_RULE int64_t sur_dim(int64_t n, int mode) { return mode == 1 ? n + 1 : n; }
// the status of a graph, by precedence: 2 too many players (device library only), 3 a sample or player that cannot be used (or,
// mode 0, a non-finite v_empty / v_full), 1 rank-deficient by the pivot rule, 0 fitted.  Non-zero: phi, phi0 and r2 are NaN.
CAL_RULE int sur_status(bool too_many, bool bad, bool deficient) { return too_many ? 2 : (bad ? 3 : (deficient ? 1 : 0)); }
// mode 0 with ONE player is defined, not solved: phi = Delta (status 0 unless 3)
CAL_RULE bool sur_one_player(int64_t n, int mode) { return mode == 0 && n == 1; }

CAL_RULE double sur_y(double v, double v_empty, int mode) { return mode == 0 ? v - v_empty : v; }
CAL_RULE double sur_gram_add(double acc, double w) { return acc + w; }
CAL_RULE double sur_rhs_add(double acc, double w, double y) { return __builtin_fma(w, y, acc); }
CAL_RULE double sur_ridge(double a, double ridge, int64_t i, int64_t n) { return i < n ? a + ridge : a; }
CAL_RULE double sur_sub(double acc, double a, double b) { return __builtin_fma(-a, b, acc); }
// column j is good iff its pivot is above 2^-30 of the diagonal entry it came from (NaN is not)
CAL_RULE bool sur_pivot_ok(double dj, double ajj) { return dj > ajj * 0x1p-30; }
CAL_RULE double sur_sqrt(double v) { return __builtin_sqrt(v); }
CAL_RULE double sur_div(double a, double b) { return a / b; }
// the Lagrange form of sum(phi) = Delta
CAL_RULE double sur_correct(double x, double u, double sx, double su, double delta) {
    const double c = (sx - delta) / su;
    return __builtin_fma(-u, c, x);
}
CAL_RULE double sur_sq_add(double acc, double w, double r) {
    const double e = w * r;
    return __builtin_fma(e, r, acc);
}
CAL_RULE double sur_r2(double ssr, double sst) {
    if (sst == 0.0) return __builtin_nan("");
    const double q = ssr / sst;
    return 1.0 - q;
}

}  // namespace cal
