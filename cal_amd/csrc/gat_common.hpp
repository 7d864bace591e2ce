// Device helpers shared by the GATConv kernels (gat.hip) and the per-graph fused GAT layer of the step engine
// (engine_ggat.hpp): the counter-based attention-dropout mask (mix32, keep_scale: rules.hpp) must be bit-identical in both.
#pragma once
#include "common.hpp"

namespace cal {

// Inside a replayed hipGraph the seed argument is frozen; the engine passes the address of its per-step device
// counter so every training step still draws a fresh mask (null: the seed is used as given).
__device__ __forceinline__ uint64_t step_seed(uint64_t seed, const uint64_t* ctr) {
    return ctr ? seed + *ctr * 0x9E3779B97F4A7C15ull : seed;
}

}  // namespace cal
