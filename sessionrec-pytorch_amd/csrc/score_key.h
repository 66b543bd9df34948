// The order-preserving 32-bit key of a served score (score_cutoff.hip: the radix search; select_many.hip: the sort key).
#pragma once
#include "common.h"

namespace score_tile {

// s + 0.0f (-0.0 -> +0.0) as a key whose unsigned order is the order of the floats (no NaN)
__device__ __forceinline__ unsigned key_of(float s) {
    const unsigned u = __float_as_uint(s + 0.f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float score_of(unsigned key) {
    return __uint_as_float((key >> 31) ? key ^ 0x80000000u : ~key);
}

}  // namespace score_tile
