// Test hook: gc_store_tile / gc_store16 (engine_mma.hpp) under either store policy, one 64-lane workgroup per call.
// tests/test_gpu_store_tile.py pre-fills a buffer with a sentinel, has a 32 x 32 accumulator whose element (row, col) holds the
// bits 0x40000000 | row << 8 | col stored at word `tile_off` of it with row stride `ld`, and compares every word.  The hook adds
// no logic to the store; it only refuses a description whose plain-policy stores would leave the buffer.  No twin in the
// host library.
#include "engine_mma.hpp"

using namespace cal;

namespace {

template <GcStore P>
__global__ void __launch_bounds__(64) k_store_probe(float* base, int ld, int nrow, int bytes) {
    const int lane = threadIdx.x, li = lane & 31, lk = lane >> 5;
    gc_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = __uint_as_float(0x40000000u | (unsigned)mma_row(r, lk) << 8 | (unsigned)li);
    gc_store_tile<P>(acc, base, (size_t)ld, nrow, li, lk, MmaIdent(), bytes);
}

}  // namespace

// policy 0 plain, 1 write-through.  buf: buf_words floats (DEVICE); the tile's word (row, col) is buf[tile_off + row * ld + col]
// for row < min(nrow, 32).  bytes: the extent from the tile's first word the write-through store may touch (stores past it are
// dropped); the plain policy ignores it.  0 launched, 2 refused with a message.
CAL_EXPORT int cal_probe_store_tile(int policy, float* buf, int64_t buf_words, int64_t tile_off, int nrow, int ld, int64_t bytes,
                                    void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(policy == 0 || policy == 1, "policy is 0 (plain) or 1 (write-through)");
    CAL_REQUIRE(buf && buf_words > 0 && ((uintptr_t)buf & 15) == 0, "buffer missing or not 16-byte aligned");
    CAL_REQUIRE(ld >= 32 && ld % 4 == 0 && ld <= (1 << 20), "ld: a multiple of 4 floats, at least one tile wide");
    CAL_REQUIRE(tile_off >= 0 && tile_off % 4 == 0, "tile offset: a non-negative multiple of 4 floats");
    CAL_REQUIRE(nrow >= 0 && nrow <= 32, "nrow in 0 .. 32");
    CAL_REQUIRE(bytes >= 0 && bytes < (1ll << 31), "extent out of range");
    const int64_t last = nrow > 0 ? tile_off + (int64_t)(nrow - 1) * ld + 32 : tile_off;
    CAL_REQUIRE(last <= buf_words, "the tile's rows leave the buffer");
    CAL_REQUIRE(tile_off * 4 + bytes <= buf_words * 4, "the extent leaves the buffer");
    if (policy == 0) hipLaunchKernelGGL(k_store_probe<GcStore::Plain>, dim3(1), dim3(64), 0, stream, buf + tile_off, ld, nrow, (int)bytes);
    else hipLaunchKernelGGL(k_store_probe<GcStore::WriteThrough>, dim3(1), dim3(64), 0, stream, buf + tile_off, ld, nrow, (int)bytes);
    CAL_CHECK_LAUNCH("k_store_probe");
    return 0;
}
