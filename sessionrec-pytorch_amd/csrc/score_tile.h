// The MFMA tile product under the catalogue pass of score_pass.h (rank.hip, recommend.hip, score_norm.hip): a workgroup of 4
// wavefronts scores 32 sessions against a 128-item chunk with v_mfma_f32_32x32x2_f32 (exact fp32), up to four session
// vectors (mixture components) per session.  The C session tiles sit in LDS when they fit, else they are read through the
// cache - same code, same summation order, same result.
//   lane (item r = lane & 31, half h = lane >> 5) loads the float4 at columns 8j + 4h of its item row, the A lane reads the
//   same columns of its session, so the MFMA's two k slots of step i are columns 8j + i and 8j + 4 + i - a permutation of the
//   sum, no staging of the table.  Accumulator register r of lane (l31, h) is (session session_of(r, h), item l31).
#pragma once
#include "common.h"

namespace score_tile {

constexpr int SB = 32;          // sessions per workgroup (one MFMA tile edge)
constexpr int CHUNK = 128;      // items per step: 32 per wavefront
constexpr int MAXCOMP = 4;
constexpr int MAXL = 64;
constexpr int LDS_BYTES = 160 * 1024;

__device__ __forceinline__ int session_of(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// the k loop runs in groups of 32 columns; LDS rows are 16-byte aligned with a stride of 4 banks mod 32
__host__ __device__ __forceinline__ int padded_d(int d) { return (d + 31) & ~31; }
__host__ __device__ __forceinline__ int tile_ld(int d) { return padded_d(d) + 4; }
inline size_t tile_bytes(int C, int d) { return (size_t)C * SB * tile_ld(d) * 4; }

template <int C>
__device__ __forceinline__ float mix(const float (&z)[C]) {
    if constexpr (C == 1) {
        return z[0];
    } else {
        float m = z[0];
#pragma unroll
        for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
        if (m == -INFINITY) return m;
        float l = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) l += expf(z[c] - m);
        return m + logf(l);
    }
}

// all 256 threads: session rows b0 .. b0 + SB of every component -> Ss [C][SB][tile_ld(d)], zero-padded (rows >= B, columns >= d)
template <int C>
__device__ __forceinline__ void stage_tiles(float* Ss, const float* sr, int ld_sr, long comp_stride, int b0, int B, int d, int tid) {
    const int dp = padded_d(d), LD = tile_ld(d), q = dp / 4;
    for (int i = tid; i < C * SB * q; i += 256) {
        const int row = i / q, k = (i % q) * 4;
        const int c = row / SB, b = b0 + row % SB;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < B && k < d) x = *reinterpret_cast<const float4*>(sr + (size_t)c * comp_stride + (size_t)b * ld_sr + k);
        *reinterpret_cast<float4*>(Ss + (size_t)row * LD + k) = x;
    }
}

// A operand rows of this lane's session (clamped when read through the cache: the caller ignores sessions >= B)
template <int C, bool SR_LDS>
__device__ __forceinline__ void a_rows(const float* (&arow)[C], const float* Ss, const float* sr, int ld_sr, long comp_stride,
                                       int b0, int B, int d, int l31, int half) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (SR_LDS) arow[c] = Ss + (size_t)(c * SB + l31) * tile_ld(d) + 4 * half;
        else arow[c] = sr + (size_t)c * comp_stride + (size_t)min(b0 + l31, B - 1) * ld_sr + 4 * half;
    }
}

// raw dot products of this wavefront's 32 items (brow: this lane's item row + 4 * half) with the 32 sessions, per component
template <int C, bool SR_LDS>
__device__ __forceinline__ void dots(const float* const (&arow)[C], const float* brow, int d, int half, f32x16 (&acc)[C]) {
    const int dp = padded_d(d);
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    // 32 columns per group: 4 float4 of the item row per lane, loaded one group AHEAD of the MFMAs that consume them
    float4 bq[4], bn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 8 * j + 4 * half;
        bq[j] = k < d ? *reinterpret_cast<const float4*>(brow + 8 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int g = 0; g < dp; g += 32) {
        if (g + 32 < dp) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = g + 32 + 8 * j + 4 * half;
                bn[j] = k < d ? *reinterpret_cast<const float4*>(brow + g + 32 + 8 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float4 aq[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (SR_LDS || g + 8 * j + 4 * half < d) aq[c] = *reinterpret_cast<const float4*>(arow[c] + g + 8 * j);
                else aq[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[c].x, bq[j].x, acc[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[c].y, bq[j].y, acc[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[c].z, bq[j].z, acc[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[c].w, bq[j].w, acc[c], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[j] = bn[j];
    }
}

}  // namespace score_tile
