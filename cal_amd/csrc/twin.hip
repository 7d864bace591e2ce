// Reverse-edge ("twin") map of a batch of graphs stored as both directions of every undirected edge.
//
// Graph g owns the nodes [ptr[g], ptr[g+1]) and the edge_index columns [edge_ptr[g], edge_ptr[g+1]).  Among the columns of g
// equal to (u, v), u != v, the j-th in ascending column order pairs with the j-th column of g equal to (v, u): twin[e] is the
// partner's global column index, -1 when there is no j-th partner.  A self loop is its own twin; a column with an endpoint
// outside its graph's node range gets -1 and pairs with nothing.  So twin[twin[e]] == e wherever twin[e] >= 0, and the output
// is uniquely determined (duplicates allowed).  totals[0] = columns with twin < 0, totals[1] = self loops.
//
// A column becomes the 64-bit key ((min(u,v) - lo) n_g + (max(u,v) - lo)) << 1 | (u > v): the two directions of an edge differ
// in bit 0 only, and ascending key order keeps them adjacent.  Positions come from counting, not from sorting: with
// lt = #{key_j < key_i}, eq = #{key_j == key_i}, j = #{key_j == key_i, j < i} and eqp = #{key_j == key_i ^ 1}, element i sits
// at sorted[lt + j] and its partner, if j < eqp, at sorted[lt + eq + j] (u < v) or sorted[lt - eqp + j] (u > v).
//
//  * segments of at most S = kSegCap columns: k_twin_lds, one group of G threads per segment (the geometry of segment.hpp,
//    shared with explain.hip: G = 64 .. 1024, 256-thread workgroups hold 256 / G segments).  Keys [cap] u64 and sorted [cap]
//    i32 in LDS (24 KB at the cap); every lane counts its element against the whole row read as 128-bit broadcasts (two keys
//    per read, every lane the same address: no bank conflict; the only scattered LDS access is the one write to sorted[]).
//    One launch.
//  * larger segments: the same kernel sorts every S-column chunk and writes its keys and column indices in sorted order to
//    ws; k_twin_merge (one workgroup per large segment) finds each column's occurrence number and its partner by binary
//    searches over the chunks staged through LDS; k_twin_totals sums the workgroups' counts.  Three launches.
//
// No value is accumulated atomically.  Every workgroup writes its two counts to ws; the totals are their sum in workgroup
// order.  In the one-launch path the workgroup that finishes last does that sum, and the only way to know it is last is a
// completion ticket (last_workgroup of rebatch.hpp): the integer result does not depend on which workgroup that is.  The large
// path needs no ticket.
#include "rebatch.hpp"

namespace cal {
namespace {

constexpr int kIt = kSegCap / kSegWide;   // columns per lane at the widest group
constexpr uint64_t kPad = ~0ull;   // key of a column that pairs with nothing, and of the LDS rows' padding

struct TwinArgs {
    const int64_t* ei;         // [2, E]
    int64_t E;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    int64_t B, max_edges;
    int32_t* twin;             // [E]
    int64_t* totals;           // [2]
    int64_t* part;             // ws: [2 x workgroups] columns with twin < 0, self loops
    uint64_t* skey;            // ws: chunk keys in sorted order [E]          (large segments only)
    int32_t* sidx;             // ws: their column indices inside the segment (large segments only)
    int ticket;                // completion ticket slot, -1: no ticket (the large path)
    int nblk;                  // workgroups of the first launch (grid.x)
};

__device__ __forceinline__ void twin_ranges(const TwinArgs& a, int64_t g, int64_t& nlo, int64_t& nn, int64_t& elo, int64_t& m) {
    nlo = a.ptr[g];
    nn = a.ptr[g + 1] - nlo;
    nn = nn < 0 ? 0 : nn;
    seg_clamp(a.eptr, g, a.E, elo, m);
}

__device__ __forceinline__ uint64_t edge_key(const TwinArgs& a, int64_t e, int64_t nlo, int64_t nn, bool& self) {
    const int64_t u = a.ei[e], v = a.ei[a.E + e];
    self = false;
    if (u < nlo || u >= nlo + nn || v < nlo || v >= nlo + nn) return kPad;
    self = u == v;
    const uint64_t x = (uint64_t)(u - nlo), y = (uint64_t)(v - nlo);
    return und_edge_key(x, y, (uint64_t)nn, u > v);
}

// grid (ceil(B / (NT / G)), chunks), NT threads; dynamic LDS: keys [NT/G][cap] u64, sorted [NT/G][cap] i32, [NT/64] i64.
// cap = G x (columns per lane) >= min(max_edges, S).  Segments of at most cap columns are finished here (chunk 0 only); a
// segment above S (then G = NT = 1024, cap = S) gets its chunk blockIdx.y sorted into ws; one above max_edges gets -1.
template <int NT>
__global__ void __launch_bounds__(NT) k_twin_lds(TwinArgs a, int G, int cap) {
    extern __shared__ __align__(16) uint64_t tlds[];
    __shared__ int last;
    const int spb = NT / G, grp = threadIdx.x / G, lt = threadIdx.x % G;
    uint64_t* sk = tlds + (size_t)grp * cap;
    int32_t* so = reinterpret_cast<int32_t*>(tlds + (size_t)spb * cap) + (size_t)grp * cap;
    long long* red = reinterpret_cast<long long*>(reinterpret_cast<char*>(tlds) + (size_t)12 * spb * cap);
    const int64_t g = (int64_t)blockIdx.x * spb + grp;
    const int64_t c = blockIdx.y;
    int64_t nlo = 0, nn = 0, elo = 0, m = 0;
    if (g < a.B) twin_ranges(a, g, nlo, nn, elo, m);
    const SegUnit u = seg_unit(g < a.B, m, a.max_edges, cap, c);
    const bool bad = u.bad, full = u.full, chunk = u.chunk;
    const int un = u.un, nq = (un + 1) & ~1;
    const int64_t ulo = u.ulo, base = elo + ulo;
    const int nit = cap / G;

    uint64_t ki[kIt];
    bool self[kIt];
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        const int q = lt + it * G;
        ki[it] = kPad;
        self[it] = false;
        if (it < nit && q < nq) {
            if (q < un) ki[it] = edge_key(a, base + q, nlo, nn, self[it]);
            sk[q] = ki[it];
        }
    }
    long long unp = 0, nself = 0;
    if (bad && c == 0) {
        for (int64_t q = lt; q < m; q += G) {
            a.twin[elo + q] = -1;
            ++unp;
        }
    }
    __syncthreads();

    int ltc[kIt], eqc[kIt], eqb[kIt], eqp[kIt];
#pragma unroll
    for (int it = 0; it < kIt; ++it) ltc[it] = eqc[it] = eqb[it] = eqp[it] = 0;
    for (int j = 0; j < nq; j += 2) {
        const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(sk + j);
        const uint64_t kj[2] = {kv.x, kv.y};
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            if (it < nit) {
                const int q = lt + it * G;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    ltc[it] += kj[t] < ki[it];
                    const int e = kj[t] == ki[it];
                    eqc[it] += e;
                    eqb[it] += e & (j + t < q);
                    eqp[it] += kj[t] == (ki[it] ^ 1ull);
                }
            }
        }
    }

    int slot[kIt];
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        const int q = lt + it * G;
        slot[it] = -1;
        if (it < nit && q < un) {
            const int pos = ltc[it] + eqb[it];
            if (chunk) {                                           // the chunk in sorted order (kPad columns last)
                a.skey[base + pos] = ki[it];
                a.sidx[base + pos] = (int32_t)(ulo + q);
            } else if (ki[it] != kPad && !self[it]) {
                so[pos] = q;
                if (eqb[it] < eqp[it]) slot[it] = ((ki[it] & 1ull) ? ltc[it] - eqp[it] : ltc[it] + eqc[it]) + eqb[it];
            }
        }
    }
    __syncthreads();
    if (full) {
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int q = lt + it * G;
            if (it < nit && q < un) {
                int32_t t = -1;
                if (self[it]) {
                    t = (int32_t)(base + q);
                    ++nself;
                } else if (slot[it] >= 0) {
                    t = (int32_t)(base + so[slot[it]]);
                }
                a.twin[base + q] = t;
                unp += t < 0;
            }
        }
    }

    if (c != 0) return;                                            // (uniform; the chunks' workgroups counted nothing)
    unp = wg_sum<NT>(unp, red);
    nself = wg_sum<NT>(nself, red);
    if (threadIdx.x == 0) {
        a.part[2 * blockIdx.x] = unp;
        a.part[2 * blockIdx.x + 1] = nself;
    }
    if (a.ticket < 0 || !last_workgroup(a.ticket, a.nblk, &last)) return;
    long long s0 = 0, s1 = 0;
    for (int i = threadIdx.x; i < a.nblk; i += NT) {
        s0 += __hip_atomic_load(a.part + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s1 += __hip_atomic_load(a.part + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    s0 = wg_sum<NT>(s0, red);
    s1 = wg_sum<NT>(s1, red);
    if (threadIdx.x == 0) {
        a.totals[0] = s0;
        a.totals[1] = s1;
    }
}

// grid B, kSegWide threads: the twins of one large segment from its sorted chunks; its counts to part[2 (nblk + g)]
__global__ void __launch_bounds__(kSegWide) k_twin_merge(TwinArgs a) {
    __shared__ __align__(16) uint64_t sk[kSegCap];
    __shared__ long long red[kSegWide / 64];
    const int64_t g = blockIdx.x;
    int64_t nlo, nn, elo, m;
    twin_ranges(a, g, nlo, nn, elo, m);
    const bool act = m > kSegCap && m <= a.max_edges;            // (uniform over the workgroup)
    const int64_t nch = act ? (m + kSegCap - 1) / kSegCap : 0;
    long long unp = 0, nself = 0;
    for (int64_t c = 0; c < nch; ++c) {
        const int un = (int)(m - c * kSegCap < kSegCap ? m - c * kSegCap : kSegCap);
        uint64_t ki[kIt];
        int64_t j[kIt], tw[kIt];
        int32_t idx[kIt];
        bool open[kIt];                                            // still looking for its partner
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int t = threadIdx.x + it * kSegWide;
            ki[it] = t < un ? a.skey[elo + c * kSegCap + t] : kPad;
            idx[it] = t < un ? a.sidx[elo + c * kSegCap + t] : 0;
            j[it] = 0;
            tw[it] = -1;
            open[it] = false;
        }
        // occurrence number: equal keys of the chunks before, then of this chunk's sorted order (ties by column index)
        for (int64_t cc = 0; cc <= c; ++cc) {
            const int n2 = (int)(m - cc * kSegCap < kSegCap ? m - cc * kSegCap : kSegCap);
            for (int t = threadIdx.x; t < n2; t += kSegWide) sk[t] = a.skey[elo + cc * kSegCap + t];
            __syncthreads();
#pragma unroll
            for (int it = 0; it < kIt; ++it) {
                if (ki[it] != kPad) {                                  // (an ascending row: the keys < k, then those == k)
                    const uint64_t k = ki[it];
                    const int lb = first_false(sk, n2, [k](uint64_t x) { return x < k; });
                    const int ub = cc < c ? first_false(sk, n2, [k](uint64_t x) { return x <= k; }) : threadIdx.x + it * kSegWide;
                    j[it] += ub - lb;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            if (ki[it] != kPad) {
                const int64_t e = elo + idx[it];
                if (a.ei[e] == a.ei[a.E + e]) tw[it] = e;
                else open[it] = true;
            }
        }
        // the j-th column with the reversed key, walking the chunks in column order
        for (int64_t cc = 0; cc < nch; ++cc) {
            const int n2 = (int)(m - cc * kSegCap < kSegCap ? m - cc * kSegCap : kSegCap);
            for (int t = threadIdx.x; t < n2; t += kSegWide) sk[t] = a.skey[elo + cc * kSegCap + t];
            __syncthreads();
#pragma unroll
            for (int it = 0; it < kIt; ++it) {
                if (open[it]) {
                    const uint64_t p = ki[it] ^ 1ull;
                    const int lb = first_false(sk, n2, [p](uint64_t x) { return x < p; });
                    const int cnt = first_false(sk, n2, [p](uint64_t x) { return x <= p; }) - lb;
                    if (j[it] < cnt) {
                        tw[it] = elo + a.sidx[elo + cc * kSegCap + lb + j[it]];
                        open[it] = false;
                    } else {
                        j[it] -= cnt;
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            if ((int)threadIdx.x + it * kSegWide < un) {
                const int64_t e = elo + idx[it];
                a.twin[e] = (int32_t)tw[it];
                unp += tw[it] < 0;
                nself += tw[it] == e;
            }
        }
    }
    unp = wg_sum<kSegWide>(unp, red);
    nself = wg_sum<kSegWide>(nself, red);
    if (threadIdx.x == 0) {
        a.part[2 * (a.nblk + g)] = unp;
        a.part[2 * (a.nblk + g) + 1] = nself;
    }
}

// one workgroup: totals = the sum of the np workgroup counts, in order
__global__ void __launch_bounds__(kSegWide) k_twin_totals(TwinArgs a, int64_t np) {
    __shared__ long long red[kSegWide / 64];
    long long s0 = 0, s1 = 0;
    for (int64_t i = threadIdx.x; i < np; i += kSegWide) {
        s0 += a.part[2 * i];
        s1 += a.part[2 * i + 1];
    }
    s0 = wg_sum<kSegWide>(s0, red);
    s1 = wg_sum<kSegWide>(s1, red);
    if (threadIdx.x == 0) {
        a.totals[0] = s0;
        a.totals[1] = s1;
    }
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_edge_twin_ws(int64_t E, int64_t B) {
    E = E > 0 ? E : 0;
    B = B > 0 ? B : 0;
    return 32 * B + 12 * E + 256;
}

CAL_EXPORT int cal_edge_twin(const int64_t* edge_index, int64_t E, const int64_t* ptr, const int64_t* edge_ptr, int64_t B,
                             int64_t max_edges, int32_t* twin, int64_t* totals, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(E >= 0 && B >= 0 && max_edges >= 0, "E, B, max_edges must be >= 0");
    CAL_REQUIRE(E < ((int64_t)1 << 31), "2^31 columns or more are not supported (twin is int32)");
    CAL_REQUIRE(totals, "totals is null");
    CAL_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");
    CAL_REQUIRE(E == 0 || (edge_index && twin), "edge_index / twin are null");
    if (B == 0) {
        if (hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), stream) != hipSuccess) {
            cal::set_error("cal_edge_twin: hipMemsetAsync failed");
            return 1;
        }
        return 0;
    }
    CAL_REQUIRE(ws && ws_bytes >= cal_edge_twin_ws(E, B) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                "ws must be 8-byte aligned and hold cal_edge_twin_ws(E, B) bytes");
    const SegGeom q = seg_geom(max_edges, B);
    CAL_REQUIRE(q.chunks_ok(), "max_edges too large");
    CAL_REQUIRE(q.grid_ok(), "too many segments");
    const int64_t nblk = q.nblk;
    char* w = (char*)ws;
    TwinArgs a{edge_index, E, ptr, edge_ptr, B, max_edges, twin, totals, (int64_t*)w, (uint64_t*)(w + 32 * B),
               (int32_t*)(w + 32 * B + 8 * E), q.large ? -1 : next_ticket(), (int)nblk};
    const size_t lds = (size_t)12 * q.spb * q.cap + (size_t)(q.NT / 64) * 8;
    CAL_SEG_LAUNCH(k_twin_lds, q, lds, stream, a);
    CAL_CHECK_LAUNCH("k_twin_lds");
    if (q.large) {
        hipLaunchKernelGGL(k_twin_merge, dim3((unsigned)B), dim3(kSegWide), 0, stream, a);
        CAL_CHECK_LAUNCH("k_twin_merge");
        hipLaunchKernelGGL(k_twin_totals, dim3(1), dim3(kSegWide), 0, stream, a, nblk + B);
        CAL_CHECK_LAUNCH("k_twin_totals");
    }
    return 0;
}
