// The 32 x 32 tile vocabulary of the per-graph fused kernels (engine_gconv.hpp, engine_gconv_bwd.hpp, engine_ggat.hpp,
// engine_ggin.hpp, engine_gwide.hpp): everything here is built on v_mfma_f32_32x32x2_f32, one wave per tile.
//
//   lane (li = lane & 31, lk = lane >> 5) feeds row / column li of the operands at reduction step 2 i + lk and holds
//   column li of the result: register r of the accumulator is row mma_row(r, lk).
//
//   basics      gc_f32x16, mma_row, gc_quad_transpose, gc_store_tile, gc_store16 (store policy: plain | write-through)
//   products    mma_kmajor     both operands k-major    [k * LD + row]   (4 B reads, two-stage pipeline)
//               mma_rowk       both operands row-major  [row * LD + k]   (16 B reads, four MFMA steps per read)
//               mma_rowk_tile  the same, addressed by tile                (see there why it is a form of its own)
//               mma_arow       A row-major, B k-major                     (two-stage pipeline)
//               mma_step4      float4 x float4 -> four MFMA steps
// Accumulator zeroing stays written out in the kernels: as a helper (by reference or by value) it changed the instruction
// order hipcc emits for the kernels around it, and these kernels are latency-bound.  What surrounds the products (unit
// extents, slot batch, operand tiles, BatchNorm tables, column-sum epilogue) is engine_gunit.hpp.
#pragma once
#include "engine.hpp"

namespace cal {

typedef float gc_f32x16 __attribute__((ext_vector_type(16)));

// row of accumulator register r in lane half lk: inside the tile, or of the matrix when the tile starts at row `base`
// (summed left to right from base, the order the kernels have always used: the address arithmetic follows it)
__device__ __forceinline__ int mma_row(int r, int lk, int base = 0) { return base + (r & 3) + 8 * (r >> 2) + 4 * lk; }
struct MmaIdent { __device__ __forceinline__ float operator()(float v) const { return v; } };

// ---- storing a 32 x 32 MFMA accumulator tile --------------------------------------------------------------------------
// Lane (li, lk) of a 32x32 tile holds ONE column (li) of the rows (r & 3) + 8 (r >> 2) + 4 lk: stored as it lies that is 16
// 4-byte store instructions per tile.  The four registers of a row group and the four lanes of a quad form a 4 x 4 block of
// (row, column): transposed inside the quad (two DPP exchanges, no LDS) every lane holds four CONSECUTIVE columns of one
// row, i.e. one 16-byte store -- 4 instructions per tile instead of 16, same bytes, same addresses.  Measured on
// k_gconv_bwd (profiles/r3/store_burst.txt): the store phase of a workgroup is 3.4 us of its 12 us and stays 2.8 us with
// the wide stores -- it is bound by BYTES (a workgroup's 64 KB leave its CU at ~20 GB/s), not by instruction issue; the wide
// form is kept for the 0.5 us.
__device__ __forceinline__ float gc_dpp_xor1(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ float gc_dpp_xor2(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true)); }   // quad_perm [2,3,0,1]
// in: lane q of the quad holds (v0..v3) = column q of rows 0..3; out: row q of columns 0..3
__device__ __forceinline__ void gc_quad_transpose(float& v0, float& v1, float& v2, float& v3, int q) {
    const bool o1 = q & 1, o2 = q & 2;
    float r = gc_dpp_xor1(o1 ? v0 : v1);
    if (o1) v0 = r; else v1 = r;
    r = gc_dpp_xor1(o1 ? v2 : v3);
    if (o1) v2 = r; else v3 = r;
    r = gc_dpp_xor2(o2 ? v0 : v2);
    if (o2) v0 = r; else v2 = r;
    r = gc_dpp_xor2(o2 ? v1 : v3);
    if (o2) v1 = r; else v3 = r;
}
// ---- store policy ------------------------------------------------------------------------------------------------------
// A plain store leaves its line dirty in the L2 of the XCD that wrote it until the write-back at the end of the kernel; a
// write-through store (sc1) sends the bytes on at once and drops the line, so a kernel that ends in a burst of tens of KB
// per workgroup does not queue all of it behind its last instruction.  The result in memory is the same.  Rules of a
// write-through site:
//   - it stores 16 bytes per lane (gc_store_tile writes each 128-byte line whole with one instruction); 4- and 8-byte
//     write-through stores cost several times more per byte, so 4-byte sites (gn / gself, k_feat_bwd_mma's scalar slab
//     stores, the bias partials, the striped atomics) stay plain;
//   - its bytes are not loaded again inside the same launch (the line is gone from this XCD's L2);
//   - the store goes through a buffer resource {base, bytes}: base is the wave's own first tile word (wave-uniform: a kernel
//     argument plus offsets of the workgroup / wave index), bytes what is left from that word to the end of what the
//     workgroup owns (its graph's slab, its graph's rows) -- every call site subtracts the tile's offset from the owned
//     extent, a negative value counts as 0.  An offset past it is dropped by the range check instead of landing in a
//     neighbour's rows.  (The compiler schedules the buffer store and pads its hazards itself.)
// Which sites write through is one mask, fixed by the A/B of profiles/r7/ab_writethrough.txt; -DCAL_WT_SITES=0x.. (through
// CAL_HIPCC_EXTRA of build.py) overrides it for a profiling build, 0 = every store plain.  WT_Z was rejected by that A/B: the
// bit is a profiling override only, the default build never compiles its write-through form and the suite does not cover it.
enum class GcStore { Plain, WriteThrough };
constexpr int WT_DW = 1;          // dW slab of k_gconv_bwd
constexpr int WT_DXP = 2;         // dX' partial tiles of k_gconv_bwd
constexpr int WT_Z = 4;           // z rows of the two-branch k_gconv_fwd (rejected: override only)
constexpr int WT_OUT = 8;         // output tiles of k_gconv_fwd
#ifndef CAL_WT_SITES
#define CAL_WT_SITES 0x0B        // dW slabs, dX' partials, output tiles (A/B: profiles/r7/ab_writethrough.txt)
#endif
constexpr GcStore gc_site(int bit) { return (CAL_WT_SITES & bit) ? GcStore::WriteThrough : GcStore::Plain; }

typedef unsigned int gc_u32x4 __attribute__((ext_vector_type(4)));
// 16 bytes at base + byte_off; WriteThrough: base and bytes wave-uniform, dropped when byte_off + 16 > bytes
template <GcStore P>
__device__ __forceinline__ void gc_store16(float* base, int bytes, int byte_off, const float4& v) {
    if constexpr (P == GcStore::WriteThrough) {
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, max(bytes, 0), 0x00020000);
        const gc_u32x4 u = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
        __builtin_amdgcn_raw_buffer_store_b128(u, rsrc, byte_off, 0, /*sc1*/ 16);
    } else {
        *reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + byte_off) = v;
    }
}

// tile(row, col) -> base[row * ld + col] for the rows with row < nrow (base, ld: 16-byte aligned / a multiple of 4 floats);
// f(v): applied to every element before the store (bias, ReLU ..); bytes (WriteThrough only): what the caller owns from base on
template <GcStore P, typename F>
__device__ __forceinline__ void gc_store_tile(const gc_f32x16& acc, float* base, size_t ld, int nrow, int li, int lk, F f, int bytes) {
    const int q = li & 3, c4 = li & ~3;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v0 = f(acc[4 * g]), v1 = f(acc[4 * g + 1]), v2 = f(acc[4 * g + 2]), v3 = f(acc[4 * g + 3]);
        gc_quad_transpose(v0, v1, v2, v3, q);
        const int row = 8 * g + 4 * lk + q;
        if constexpr (P == GcStore::WriteThrough) {
            if (row < nrow) gc_store16<P>(base, bytes, (row * (int)ld + c4) * 4, make_float4(v0, v1, v2, v3));
        } else {
            if (row < nrow) *reinterpret_cast<float4*>(base + (size_t)row * ld + c4) = make_float4(v0, v1, v2, v3);
        }
    }
}
// the plain forms (a write-through site calls the one above: it has to name its extent)
template <typename F>
__device__ __forceinline__ void gc_store_tile(const gc_f32x16& acc, float* base, size_t ld, int nrow, int li, int lk, F f) {
    gc_store_tile<GcStore::Plain>(acc, base, ld, nrow, li, lk, f, 0);
}
__device__ __forceinline__ void gc_store_tile(const gc_f32x16& acc, float* base, size_t ld, int nrow, int li, int lk) {
    gc_store_tile<GcStore::Plain>(acc, base, ld, nrow, li, lk, MmaIdent(), 0);
}

// ---- products ---------------------------------------------------------------------------------------------------------
// k-major: NA tiles of A against NB tiles of B over kred (a multiple of 32), operands A[k * LDA + row], B[k * LDB + col].
// a / b point at this lane's row / column of the first tile; the second tile of an operand lies 32 rows / columns further.
// One of the operands is shared: acc[0] = a(0) b(0), acc[1] = a(1) b(0) (NA == 2) or a(0) b(1) (NB == 2).
// ax / bx transform every A / B element as it is read (identity, or e.g. the BatchNorm affine of the lane's column).
// The reads of block kb + 1 are issued before the 16 MFMA steps of block kb; the sched_barriers keep hipcc from sinking
// them back behind the MFMAs.
// (mma_kmajor_ptrs: the same with the lane pointers of both tiles of each operand given; the unused one may be null)
template <int NA, int NB, int LDA, int LDB, class AX, class BX>
__device__ __forceinline__ void mma_kmajor_ptrs(const float* a, const float* a1, const float* b, const float* b1, int kred, int lk, AX ax, BX bx, gc_f32x16 (&acc)[2]) {
    static_assert(NA == 1 || NB == 1, "one of the operands is shared");
    float av[2][2][16], bv[2][2][16];
    auto read_ops = [&](int kb, int s) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = kb * 32 + 2 * i + lk;
            av[s][0][i] = ax(a[k * LDA]);
            if (NA == 2) av[s][1][i] = ax(a1[k * LDA]);
            bv[s][0][i] = bx(b[k * LDB]);
            if (NB == 2) bv[s][1][i] = bx(b1[k * LDB]);
        }
    };
    auto mul = [&](int s) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][0][i], bv[s][0][i], acc[0], 0, 0, 0);
            if (NA == 2) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][1][i], bv[s][0][i], acc[1], 0, 0, 0);
            if (NB == 2) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][0][i], bv[s][1][i], acc[1], 0, 0, 0);
        }
    };
    const int nkb = kred / 32;
    read_ops(0, 0);
    for (int kb = 0; kb < nkb; kb += 2) {
        if (kb + 1 < nkb) read_ops(kb + 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mul(0);
        __builtin_amdgcn_sched_barrier(0);
        if (kb + 1 < nkb) {
            if (kb + 2 < nkb) read_ops(kb + 2, 0);
            __builtin_amdgcn_sched_barrier(0);
            mul(1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int NA, int NB, int LDA, int LDB, class AX, class BX>
__device__ __forceinline__ void mma_kmajor(const float* a, const float* b, int kred, int lk, AX ax, BX bx, gc_f32x16 (&acc)[2]) {
    mma_kmajor_ptrs<NA, NB, LDA, LDB>(a, a + 32, b, b + 32, kred, lk, ax, bx, acc);
}

// four MFMA steps from one 16-byte read per operand: lane (li, lk) holds the four consecutive k of every eight of its row.
// Any bijection of k onto (MFMA step, lk) is a valid reduction order as long as A and B share it.
__device__ __forceinline__ void mma_step4(const float4& a, const float4& b, gc_f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// row-major in k: operands A[row * LDA + k], B[col * LDB + k] with strides = 4 mod 32 floats (16 B reads of 32 consecutive
// rows are bank-conflict free, 4 B reads would be 4-way conflicts).  a0_row / a1_row / b_row point at this lane's rows;
// acc0 = rows of a0_row, acc1 = rows of a1_row (TWO; otherwise a1_row and acc1 are not touched).  kred % 32 == 0.
template <bool TWO>
__device__ __forceinline__ void mma_rowk(const float* a0_row, const float* a1_row, const float* b_row, int kred, int lk,
                                             gc_f32x16& acc0, gc_f32x16& acc1) {
    for (int k0 = 0; k0 < kred; k0 += 32) {
        float4 av[4], aw[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + 8 * i + 4 * lk;
            av[i] = *reinterpret_cast<const float4*>(a0_row + k);
            if (TWO) aw[i] = *reinterpret_cast<const float4*>(a1_row + k);
            bv[i] = *reinterpret_cast<const float4*>(b_row + k);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float a[4] = {av[i].x, av[i].y, av[i].z, av[i].w}, b[4] = {bv[i].x, bv[i].y, bv[i].z, bv[i].w};
            const float a2[4] = {TWO ? aw[i].x : 0.f, TWO ? aw[i].y : 0.f, TWO ? aw[i].z : 0.f, TWO ? aw[i].w : 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc0, 0, 0, 0);
                if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[j], b[j], acc1, 0, 0, 0);
            }
        }
    }
}
// one tile (the unused second row and accumulator of mma_rowk<false> are never read or written)
__device__ __forceinline__ void mma_rowk(const float* a_row, const float* b_row, int kred, int lk, gc_f32x16& acc) {
    mma_rowk<false>(a_row, nullptr, b_row, kred, lk, acc, acc);
}

// The same product addressed by tile: At[i * LD + j], Zt[col * LD + j], this wave's row tile r0 (TWO: and r0 + 2) against
// column tile ct.  A function of its own because the forward kernels fold 4 lk into the lane pointers ahead of the k loop
// and mma_rowk adds it inside: hipcc keeps the two groupings apart, and the forward kernels' address arithmetic (and
// with it their instruction order) changes when they go through mma_rowk.
template <bool TWO, int LD>
__device__ __forceinline__ void mma_rowk_tile(const float* At, const float* Zt, int kred, int r0, int ct, int li, int lk,
                                               gc_f32x16& acc0, gc_f32x16& acc1) {
    const float* a0p = At + (r0 * 32 + li) * LD + 4 * lk;
    const float* a1p = At + ((r0 + 2) * 32 + li) * LD + 4 * lk;
    const float* bp = Zt + (ct * 32 + li) * LD + 4 * lk;
    for (int k0 = 0; k0 < kred; k0 += 32) {
        float4 a0[4], a1[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a0[i] = *reinterpret_cast<const float4*>(a0p + k0 + 8 * i);
            if (TWO) a1[i] = *reinterpret_cast<const float4*>(a1p + k0 + 8 * i);
            bv[i] = *reinterpret_cast<const float4*>(bp + k0 + 8 * i);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x[4] = {a0[i].x, a0[i].y, a0[i].z, a0[i].w}, b[4] = {bv[i].x, bv[i].y, bv[i].z, bv[i].w};
            const float y[4] = {TWO ? a1[i].x : 0.f, TWO ? a1[i].y : 0.f, TWO ? a1[i].z : 0.f, TWO ? a1[i].w : 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[j], b[j], acc0, 0, 0, 0);
                if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y[j], b[j], acc1, 0, 0, 0);
            }
        }
    }
}

// A row-major in k (Xr[row * LDA + k], LDA = 4 mod 32: conflict-free 16 B reads), B k-major (Bs[k * LDB + col], as a weight
// slice is loaded), pipelined like mma_kmajor; r0 / ct: this wave's row / column tile, TWO: it also owns row tile r0 + 2.
// Lane (li, lk) takes the four consecutive k of every eight from its row with one ds_read_b128 and the matching four B
// values with 4 B reads.  Against a k-major A stage: no transposing scalar stores while staging (8 float4 stores per lane
// instead of 32 scalar ones) and a third fewer LDS reads in the product.
// (Not folded into mma_rowk: that one has no read-ahead, and giving it one changes the instruction order of its callers.)
template <bool TWO, int LDA, int LDB>
__device__ __forceinline__ void mma_arow(const float* Xr, const float* Bs, int kred, int r0, int ct, int li, int lk,
                                         gc_f32x16& acc0, gc_f32x16& acc1) {
    const float* a0p = Xr + (r0 * 32 + li) * LDA + 4 * lk;
    const float* a1p = Xr + ((r0 + 2) * 32 + li) * LDA + 4 * lk;
    const float* bp = Bs + ct * 32 + li + 4 * lk * LDB;
    float4 a0[2][4], a1[2][4];
    float bv[2][16];
    auto read_ops = [&](int kb, int s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a0[s][i] = *reinterpret_cast<const float4*>(a0p + kb * 32 + 8 * i);
            if (TWO) a1[s][i] = *reinterpret_cast<const float4*>(a1p + kb * 32 + 8 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[s][4 * i + j] = bp[(kb * 32 + 8 * i + j) * LDB];
        }
    };
    auto mul = [&](int s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x[4] = {a0[s][i].x, a0[s][i].y, a0[s][i].z, a0[s][i].w};
            const float y[4] = {TWO ? a1[s][i].x : 0.f, TWO ? a1[s][i].y : 0.f, TWO ? a1[s][i].z : 0.f, TWO ? a1[s][i].w : 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[j], bv[s][4 * i + j], acc0, 0, 0, 0);
                if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y[j], bv[s][4 * i + j], acc1, 0, 0, 0);
            }
        }
    };
    const int nkb = kred / 32;
    read_ops(0, 0);
    for (int kb = 0; kb < nkb; kb += 2) {
        if (kb + 1 < nkb) read_ops(kb + 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mul(0);
        __builtin_amdgcn_sched_barrier(0);
        if (kb + 1 < nkb) {
            if (kb + 2 < nkb) read_ops(kb + 2, 0);
            __builtin_amdgcn_sched_barrier(0);
            mul(1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

}  // namespace cal
