// srec_score_items: the score of srec_score_rank / srec_score_select at GIVEN items of every session - M candidate ids per
// session (re-ranking, allow-lists, sampled-negative evaluation, lists longer than recommend.hip's 128), WITHOUT the (B, V)
// score matrix (replaces `logits = model(...); logits.gather(1, items)` over msgifsr.py:306-321 / srgnn.py:145-147).  The
// served score, its layouts and limits: score_pass.h, which also gives the argument block, its checks and switch_c.
// Per slot: id < 0 (padding) -> -INFINITY; a row outside [id_lo, id_lo + V) belongs to another shard -> 0.0f, nothing is
// read for it (results of disjoint row ranges add up); SREC_LISTED_SCORE: a listed item scores with off_in;
// SREC_LISTED_DROP: the owning shard gives -INFINITY.  Duplicate ids are scored independently.
//
// A gather: M rows of d floats per session, nothing to reuse but the session vectors, so the kernel is built around the
// number of row loads in flight, not around a tile product (rank.hip's wave_dots keeps ONE row per wavefront in flight and
// re-reads the session vector from memory for every row).
//   workgroup (256 threads) = one session x a chunk of 256 of its candidate slots.  Thread i resolves slot i once: id ->
//     local row / padding / foreign, and its membership in listed[b,:] (staged in LDS), so the hot loop reads two LDS words
//     per slot and no id or list from memory.
//   a row is read by T = min(64, d / 4 rounded up to a power of two) lanes as 16-byte loads: one 64-lane load instruction
//     carries 64 / T rows (d >= 256: one row, columns 4 lane + 256 j, j < J = ceil(d / 256)).  The C session vectors sit in
//     registers, every lane its own columns (C J float4), read once per workgroup.
//   a wavefront issues the loads of U row groups (U J = 8 loads of 16 bytes per lane, and the U column scales) before it
//     reduces any: 8 KB in flight per wavefront.  The partial dot products meet over the T lanes of a row in a butterfly of
//     lane exchanges (the U C exchanges of a stage are independent of each other), so the order of the sum depends on
//     (d, C) alone - never on M, the slot, the shard or the view.
// No atomics, no workspace, no scratch memory; every out[b,m] is written by exactly one lane.  Sessions run along grid.x.
//
// a bias in the descriptor (template parameter BIAS; false: the instances of the call without one, unchanged): the owning shard
// adds bias[group[b], local row] after the mixture.  The lookup sits where thread i resolves slot i: a bias of -INFINITY
// turns the slot into a padding slot (no row is read for it), any other value goes to a third LDS word per slot that the
// writing lane adds - no memory instruction joins the hot loop, and a foreign id reads neither the table nor the bias.
#include "common.h"
#include "score_pass.h"

namespace {

using score_tile::MAXL;
using score_tile::mix;
using score_tile::PassArgs;

constexpr int CH = 256;             // candidate slots per workgroup pass (one per thread when they are resolved)
constexpr int ROW_PAD = -1;         // slot states below the local rows: -INFINITY ...
constexpr int ROW_FOREIGN = -2;     // ... and 0.0f (another shard owns the id)

struct ItemArgs : PassArgs {        // off_in: null under SREC_LISTED_DROP; group: null when G == 1
    const int* items; long ld_items; int M;
    int logT;                       // a row is read by 1 << logT lanes
    float* out;
};

template <int C, int J, bool BIAS>
__global__ __launch_bounds__(256) void score_items_kernel(ItemArgs a) {
    constexpr int U = 8 / J;                                        // row groups in flight per wavefront
    __shared__ int lst[MAXL];
    __shared__ int srow[CH];                                        // local row, ROW_PAD or ROW_FOREIGN
    __shared__ int sin[CH];                                         // 1: the slot's item is listed (SCORE mode)
    __shared__ float sbias[BIAS ? CH : 1];                          // the slot's bias (finite: -INFINITY became ROW_PAD)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int T = 1 << a.logT, R = 64 >> a.logT;                    // lanes per row, rows per load instruction
    const int t = lane & (T - 1), g = lane >> a.logT;
    const int d = a.d, M = a.M, L = a.L;

    float4 s[C][J];
    float oex[C], oin[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* sp = a.sr + (size_t)c * a.comp_stride + (size_t)b * a.ld_sr;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int k = 4 * t + 256 * j;
            s[c][j] = k < d ? *reinterpret_cast<const float4*>(sp + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        oex[c] = a.off_ex != nullptr ? a.off_ex[(size_t)c * a.B + b] : 0.f;
        oin[c] = a.off_in != nullptr ? a.off_in[(size_t)c * a.B + b] : 0.f;
    }
    if (tid < L) lst[tid] = a.listed[(size_t)b * L + tid];
    __syncthreads();

    const int* ids = a.items + (size_t)b * a.ld_items;
    // this session's bias row; a group id outside [0, G) is the caller's error and is held inside the operand
    const float* brow = nullptr;
    if constexpr (BIAS) brow = a.bias + (a.group != nullptr ? (size_t)min(max(a.group[b], 0), a.G - 1) * a.ld_bias : 0);
    float* orow = a.out + (size_t)b * M;
    const int nchunk = (M + CH - 1) / CH;
    for (int chunk = blockIdx.y; chunk < nchunk; chunk += gridDim.y) {
        const int m0 = chunk * CH, n = min(CH, M - m0);
        {
            int row = ROW_PAD, in = 0;
            float bv = 0.f;
            if (tid < n) {
                const long id = ids[m0 + tid];
                const long lr = id - a.id_lo;
                if (id >= 0) {
                    if (lr < 0 || lr >= (long)a.V) {
                        row = ROW_FOREIGN;
                    } else {
                        for (int i = 0; i < L; ++i) in |= (int)((long)lst[i] == id);
                        row = (in && a.drop) ? ROW_PAD : (int)lr;
                        if constexpr (BIAS) {
                            if (row >= 0) {
                                bv = brow[lr];
                                if (bv == -INFINITY) row = ROW_PAD;
                            }
                        }
                    }
                }
            }
            srow[tid] = row;
            sin[tid] = in;
            if constexpr (BIAS) sbias[tid] = bv;
        }
        __syncthreads();

        // slots of one step: (u, wave, g) -> (u * 4 + wave) * R + g, so a short chunk spreads over the four wavefronts
        for (int base = 0; base < n; base += 4 * U * R) {
            int row[U];
            float4 e[U][J];
            float csv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int sl = base + (u * 4 + wave) * R + g;
                row[u] = sl < n ? srow[sl] : ROW_PAD;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {                           // every load of the step, before any use
                const bool live = row[u] >= 0;
                const float* er = a.E + (size_t)(live ? row[u] : 0) * a.ld_e;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const int k = 4 * t + 256 * j;
                    e[u][j] = (live && k < d) ? *reinterpret_cast<const float4*>(er + k) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                csv[u] = (live && a.cs != nullptr) ? a.cs[row[u]] : 1.f;
            }
            float p[U][C];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float acc = 0.f;
#pragma unroll
                    for (int j = 0; j < J; ++j)
                        acc += e[u][j].x * s[c][j].x + e[u][j].y * s[c][j].y + e[u][j].z * s[c][j].z + e[u][j].w * s[c][j].w;
                    p[u][c] = acc;
                }
            // butterfly over the T lanes of a row (T is uniform); the U C exchanges of one stage are independent
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                if (o < T) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int c = 0; c < C; ++c) p[u][c] += __shfl_xor(p[u][c], o, 64);
                }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int sl = base + (u * 4 + wave) * R + g;
                if (t == 0 && sl < n) {
                    float v;
                    if (row[u] >= 0) {
                        const bool in = sin[sl] != 0;
                        float z[C];
#pragma unroll
                        for (int c = 0; c < C; ++c) z[c] = csv[u] * p[u][c] + (in ? oin[c] : oex[c]);
                        v = mix<C>(z);
                        if constexpr (BIAS) v += sbias[sl];
                    } else {
                        v = row[u] == ROW_PAD ? -INFINITY : 0.f;
                    }
                    orow[m0 + sl] = v;
                }
            }
        }
        __syncthreads();                                            // the next chunk overwrites srow / sin
    }
}

template <int C, int J>
int launch(const ItemArgs& a, hipStream_t st) {
    const int nchunk = cdiv(a.M, CH);
    const dim3 grid(a.B, nchunk < 65535 ? nchunk : 65535);
    if (a.bias == nullptr) hipLaunchKernelGGL((score_items_kernel<C, J, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((score_items_kernel<C, J, true>), grid, dim3(256), 0, st, a);
    SREC_LAUNCH_CHECK();
    return 0;
}

template <int C>
int run(const ItemArgs& a, hipStream_t st) {
    if (a.d <= 256) return launch<C, 1>(a, st);
    if (a.d <= 512) return launch<C, 2>(a, st);
    return launch<C, 4>(a, st);
}

}  // namespace

extern "C" int srec_score_items(const void* served, const int* items, long ld_items, int M, float* out, void* stream) {
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    ItemArgs a{};
    if (score_tile::pass_args(a, *s, true) || M < 1 || s->ld_sr < s->d || s->ld_e < s->d || ((uintptr_t)items & 3) ||
        ((uintptr_t)out & 3) || items == nullptr || out == nullptr || (ld_items != 0 && ld_items < (long)M))
        return SREC_BAD_ARG;
    if (s->listed_mode == SREC_LISTED_DROP) a.off_in = nullptr;     // (ItemArgs)
    if (s->G == 1) a.group = nullptr;
    a.items = items; a.ld_items = ld_items; a.M = M; a.out = out;
    while ((4 << a.logT) < s->d && a.logT < 6) ++a.logT;            // the smallest power of two of lanes that covers a row
    hipStream_t st = (hipStream_t)stream;
    return score_tile::switch_c(s->C, [&](auto c) { return run<c.value>(a, st); });
}
