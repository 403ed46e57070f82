// What the ragged translation units (k_ragged*.hip) share: the limit of a flat grid, the wave-uniform load and the mark of the host
// arithmetic that a kernel evaluates too.  The host part is plain C++, so that window_host.hpp can include this file in a program
// without HIP.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SICN_HD __host__ __device__
#else
#define SICN_HD
#endif
#include <stdint.h>

namespace sicn {
constexpr int64_t RAGGED_MAX_ITEMS = 0x7fffffffLL;   // a launch has fewer work items than this (grid.x)

// one image in one layer of a ragged net (k_ragged.hip builds the table, k_ragged.hip and k_ragged_rgb.hip read it): its sizes, its
// first work item and its byte offsets in the layer's input and output tensors
struct RaggedRow {
    int32_t IW, IH, OW, OH, tiles_x, first_item;
    int64_t in_off, out_off;
};
}

#ifdef __HIPCC__
namespace {
// a value that depends on blockIdx only, moved to scalar registers
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni(uint64_t v) { return (uint64_t)uni((uint32_t)v) | (uint64_t)uni((uint32_t)(v >> 32)) << 32; }
}  // namespace
#endif
