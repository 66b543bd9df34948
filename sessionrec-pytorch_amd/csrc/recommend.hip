// srec_score_select[_biased]: the K best catalog items of every session (K <= 128) under the served score (score_pass.h:
// score, eligibility, layouts and limits), WITHOUT the (B, V) score matrix - the serving path (model.recommend).
// Output: values descending, global ids id_lo + row, ties towards the lower id (topk.hip, rank.hip); a session with fewer
// than K eligible rows ends in (-INFINITY, -1) slots; K > V is legal.  An item that merely SCORES -INFINITY is eligible: it
// still beats an unfilled slot.
//
// Pass 1 (select_part_kernel): the pass of score_pass.h.  Every session keeps its running K best in LDS, sorted by (value
//   desc, id asc).  A lane whose eligible item beats the session's K-th best writes the score to slot [session][item of the
//   chunk] of a candidate array and the wavefront's ballot to a survivor mask: one slot per item of the chunk, so the list
//   cannot overflow (a chunk in which EVERY item is a candidate - the first one, or scores that rise with the id - is the
//   plain case), and no atomics at all.  One wavefront per session then merges the survivors into the sorted list: every
//   entry's new position is its own position plus the number of entries of the other side that are better (candidates:
//   binary search in the list), a permutation because (value, id) keys are distinct.  Cost O((K + n) n / 64) per merge,
//   nothing when no item survived.  One barrier per chunk covers the membership mask: the merges that follow the epilogue
//   end in the barrier ahead of the next mask's readers.
// Pass 2 (select_merge_kernel): one wavefront per session folds the per-range lists with the same merge.
// The output is a pure function of the inputs: positions come from comparisons of (value, id) keys, never from arrival.
// LDS (part_lds): the pass's 1.6 KB of offsets, mask and counts, 32 L ids (and 256 bytes of bias row offsets with G rows) +
// 0.5 KB of survivor masks + 32 K (value, id) pairs + 17 KB candidates + the session tiles when the sum stays within 160 KB
// (C = 3, d = 256, K = 128, L = 64: 160 384 bytes = 156.6 KB; with G rows 156.9 KB), else the tiles are read through the cache.
//
// srec_score_sample: the same two passes over the SAMPLED key  s' / T + g(seed, q[b], id_lo + v)  (NOISE = true instances;
// sample_noise.h is the noise): by the Gumbel-top-k identity the K best keys, in order, are a draw without replacement from
// softmax(s' / T) over the eligible rows.  The 32 sessions' hashed keys are staged in LDS once (128 bytes more, noisy
// instances only: 160 512 bytes in the case above, 160 768 with G rows - placed by the same rule); the lane that owns item v
// forms the item's half of the hash once per chunk and the key after the score, and the key takes the score's place in the
// threshold test, in cand and in both merges.  The noise is a function of GLOBAL ids, so row shards merge to the bits of one
// device, and a session's draw does not depend on the batch it came in.
#include "common.h"
#include "sample_noise.h"
#include "score_pass.h"

namespace {

using namespace score_tile;

constexpr int MAXK = 128;
constexpr int CST = CHUNK + 8;      // candidate row stride: sessions sl and sl + 4 (the two lane halves) 32 banks apart
constexpr int EMPTY = 0x7fffffff;   // id of an unfilled list slot: behind every real item of the same value

struct SelArgs : PassArgs {
    int K;
    float* pv; int* pi;             // [R][B][K] per-range lists (local rows; EMPTY = unfilled)
    float inv_t;                    // NOISE instances only: 1 / T, the seed and the session keys (NULL: the row index)
    unsigned long long seed;
    const int* qkeys;
    const float* floor;             // FLOOR instances only: [B], a pair with s' < floor[b] is ineligible
};

__device__ __forceinline__ bool better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// one wavefront: merge the candidates whose bit is set in m[0..4) (wave-uniform; candidate p = value cv[p], id ci[p] or
// id_base + p) into the list lv / li [K], sorted by `better`.  All keys are distinct.
template <bool IDS>
__device__ __forceinline__ void merge_sorted(float* lv, int* li, int K, const float* cv, const int* ci, int id_base,
                                             const unsigned (&m)[4], int lane) {
    float ev[2], xv[2]; int ei[2], xi[2], eadd[2], xr[2]; bool ch[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int p = lane + 64 * e;
        const bool in = p < K;
        ev[e] = in ? lv[p] : -INFINITY;
        ei[e] = in ? li[p] : EMPTY;
        ch[e] = (m[2 * e + (lane >> 5)] >> (lane & 31)) & 1u;
        xv[e] = ch[e] ? cv[p] : -INFINITY;
        xi[e] = ch[e] ? (IDS ? ci[p] : id_base + p) : EMPTY;
        eadd[e] = 0; xr[e] = 0;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        unsigned word = m[w];
        while (word != 0u) {
            const int q = w * 32 + __builtin_ctz(word);
            word &= word - 1u;
            const float qv = cv[q];
            const int qi = IDS ? ci[q] : id_base + q;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                eadd[e] += (int)better(qv, qi, ev[e], ei[e]);
                xr[e] += (int)better(qv, qi, xv[e], xi[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        int lo = 0, hi = ch[e] ? K : 0;                       // number of list entries better than this candidate
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (better(lv[mid], li[mid], xv[e], xi[e])) lo = mid + 1; else hi = mid;
        }
        xr[e] += lo;
    }
    __builtin_amdgcn_wave_barrier();                          // every read of the old list is done
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int p = lane + 64 * e;
        if (p < K && eadd[e] > 0 && p + eadd[e] < K) { lv[p + eadd[e]] = ev[e]; li[p + eadd[e]] = ei[e]; }
        if (ch[e] && xr[e] < K) { lv[xr[e]] = xv[e]; li[xr[e]] = xi[e]; }
    }
    __builtin_amdgcn_wave_barrier();
}

inline size_t part_lds(int C, int d, int K, int L, bool sr_lds, bool grouped = false, bool noisy = false, bool floored = false) {
    return pass_lds(L, grouped) + (size_t)SB * 4 * 4 + (size_t)SB * K * 8 + (size_t)SB * CST * 4 + (noisy ? (size_t)SB * 4 : 0) +
           (floored ? (size_t)SB * 4 : 0) + (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS, int BIAS, bool NOISE, bool FLOOR>
__global__ __launch_bounds__(256) void select_part_kernel(SelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d, K = a.K, L = a.L;
    float* offs = smem;                                             // the pass's arrays (PassLds) among this kernel's:
    float* offi = offs + MAXCOMP * SB;
    unsigned* inm = reinterpret_cast<unsigned*>(offi + MAXCOMP * SB);
    unsigned* surv = inm + SB * 4;                                  // [SB][4] survivors of this chunk
    int* nin = reinterpret_cast<int*>(surv + SB * 4);
    float* lv = reinterpret_cast<float*>(nin + SB);                 // [SB][K] running best values
    int* li = reinterpret_cast<int*>(lv + SB * K);                  // [SB][K] ... and local rows
    float* cand = reinterpret_cast<float*>(li + SB * K);            // [SB][CST] scores of this chunk's survivors
    int* lst = reinterpret_cast<int*>(cand + SB * CST);
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(lst + SB * L);
    unsigned* skey = reinterpret_cast<unsigned*>(goff + (BIAS == 2 ? SB : 0));   // [SB] hashed session keys (NOISE)
    float* flr = reinterpret_cast<float*>(skey + (NOISE ? SB : 0));  // [SB] the sessions' floors (FLOOR)
    float* Ss = flr + (FLOOR ? SB : 0);                             // [C][SB][LD] (SR_LDS); 16-byte aligned: all counts above are multiples of 4

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB, range = blockIdx.x;
    const int v0 = range * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const PassLds<true> ps{offs, offi, inm, nin, lst, goff, L > 0, a.drop != 0};

    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    for (int i = tid; i < SB * K; i += 256) { lv[i] = -INFINITY; li[i] = EMPTY; }
    SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)
    if constexpr (NOISE) {
        if (tid < SB) {
            const int b = b0 + tid;
            skey[tid] = srec_sample_skey(a.seed, b < a.B ? (unsigned)(a.qkeys != nullptr ? a.qkeys[b] : b) : 0u);
        }
    }
    if constexpr (FLOOR) {
        if (tid < SB) flr[tid] = b0 + tid < a.B ? a.floor[b0 + tid] : -INFINITY;
    }
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);

    for (int base = v0; base < v1; base += CHUNK) {
        SCORE_PASS_CHUNK_MASK(ps, L, base, tid)
        SCORE_PASS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)
        f32x16 acc[C];
        dots<C, SR_LDS>(arow, it.brow, d, half, acc);
        __syncthreads();              // membership bits written; the merges of the previous chunk are done

        // per-lane epilogue: item v (this lane's column) against 16 sessions
        [[maybe_unused]] const unsigned gmix = (unsigned)(a.id_lo + it.v) * 0x9E3779B1u + 0x7F4A7C15u;   // srec_sample_hash, the item's half
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            SCORE_PASS_ITEM_SCORE(C, BIAS, it, acc, r, ps, wave, l31, half, sl, in, s, bias_ok)
            [[maybe_unused]] bool kept = true;
            if constexpr (FLOOR) kept = !(s < flr[sl]);             // on the served score, before temperature and noise
            if constexpr (NOISE) s = fmaf(s, a.inv_t, srec_sample_gumbel(srec_sample_h32(skey[sl] ^ gmix)));   // the sampled key
            const bool hit = SCORE_PASS_ELIGIBLE(it, in, ps, b0 + sl < a.B, bias_ok) && (!FLOOR || kept) && better(s, it.v, lv[sl * K + K - 1], li[sl * K + K - 1]);
            const unsigned long long mk = __ballot(hit);
            if (hit) cand[sl * CST + wave * 32 + l31] = s;
            if (l31 == 0) surv[sl * 4 + wave] = half ? (unsigned)(mk >> 32) : (unsigned)mk;
        }
        __syncthreads();

        for (int j = wave; j < SB; j += 4) {
            unsigned m[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) m[w] = __builtin_amdgcn_readfirstlane(surv[j * 4 + w]);
            if ((m[0] | m[1] | m[2] | m[3]) != 0u)
                merge_sorted<false>(lv + j * K, li + j * K, K, cand + j * CST, nullptr, base, m, lane);
        }
    }
    __syncthreads();
    for (int i = tid; i < SB * K; i += 256) {
        const int j = i / K, r = i % K;
        if (b0 + j < a.B) {
            a.pv[((size_t)range * a.B + b0 + j) * K + r] = lv[i];
            a.pi[((size_t)range * a.B + b0 + j) * K + r] = li[i];
        }
    }
}

__global__ __launch_bounds__(256) void select_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int R,
                                                           int B, int K, long id_lo, float* __restrict__ out_v,
                                                           int* __restrict__ out_i) {
    __shared__ float lv[4][MAXK];
    __shared__ int li[4][MAXK];
    __shared__ float cv[4][MAXK];
    __shared__ int ci[4][MAXK];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + w;
    if (b >= B) return;
    float nv[2]; int ni[2];
    auto fetch = [&](int r) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int p = lane + 64 * e;
            const bool in = p < K && r < R;
            const size_t src = ((size_t)(in ? r : 0) * B + b) * K + (in ? p : 0);
            nv[e] = in ? pv[src] : -INFINITY;
            ni[e] = in ? pi[src] : EMPTY;
        }
    };
    fetch(0);
#pragma unroll
    for (int e = 0; e < 2; ++e) { lv[w][lane + 64 * e] = nv[e]; li[w][lane + 64 * e] = ni[e]; }
    __builtin_amdgcn_wave_barrier();
    fetch(1);
    for (int r = 1; r < R; ++r) {
        unsigned m[4];
        const float tv = lv[w][K - 1];
        const int ti = li[w][K - 1];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const bool hit = better(nv[e], ni[e], tv, ti);
            const unsigned long long mk = __ballot(hit);
            m[2 * e] = (unsigned)mk; m[2 * e + 1] = (unsigned)(mk >> 32);
            cv[w][lane + 64 * e] = nv[e]; ci[w][lane + 64 * e] = ni[e];
        }
        __builtin_amdgcn_wave_barrier();
        fetch(r + 1);                                               // the next list is under way during this merge
        if ((m[0] | m[1] | m[2] | m[3]) != 0u) merge_sorted<true>(lv[w], li[w], K, cv[w], ci[w], 0, m, lane);
        else __builtin_amdgcn_wave_barrier();
    }
    for (int r = lane; r < K; r += 64) {
        const int id = li[w][r];
        out_v[(size_t)b * K + r] = lv[w][r];
        out_i[(size_t)b * K + r] = id == EMPTY ? -1 : (int)(id_lo + id);
    }
}

template <int C, bool SR_LDS, int BIAS>
struct SelectPart { static constexpr auto kernel = select_part_kernel<C, SR_LDS, BIAS, false, false>; };
template <int C, bool SR_LDS, int BIAS>
struct SamplePart { static constexpr auto kernel = select_part_kernel<C, SR_LDS, BIAS, true, false>; };
template <int C, bool SR_LDS, int BIAS>
struct SelectFloorPart { static constexpr auto kernel = select_part_kernel<C, SR_LDS, BIAS, false, true>; };
template <int C, bool SR_LDS, int BIAS>
struct SampleFloorPart { static constexpr auto kernel = select_part_kernel<C, SR_LDS, BIAS, true, true>; };

inline int ranges(int B, int V) { return pick_ranges(B, V, 512, 4); }   // the lists and tiles leave room for one or two
                                                                        // workgroups per CU; the first chunk fills the list
}  // namespace

// ws: the per-range partial lists, (value, row) pairs
extern "C" int srec_score_select_ws(int B, int V, int d, int C, int L, int K, long* bytes) {
    if (bad_shape(B, V, d, C, L) || K < 1 || K > MAXK || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = (long)ranges(B, V) * B * K * 8;
    return 0;
}

namespace {

// both entry points (s: not NULL, B > 0): NOISE = false is the selection as it always was (inv_t / seed / qkeys are not
// read); floor == NULL launches the instances the calls without a floor always launched
template <bool NOISE>
int select_launch(const srec_served& s, int K, float inv_t, unsigned long long seed, const int* qkeys, const float* floor,
                  float* out_val, int* out_idx, void* ws, void* stream) {
    SelArgs a{};
    if (pass_args(a, s, true) || K < 1 || K > MAXK || out_val == nullptr || out_idx == nullptr || ws == nullptr ||
        ((uintptr_t)floor & 3))
        return SREC_BAD_ARG;
    const int B = s.B, V = s.V, d = s.d, C = s.C;
    const int R = ranges(B, V);
    const dim3 grid(split_ranges(a, R), cdiv(B, SB));
    a.K = K;
    a.pv = (float*)ws;
    a.pi = (int*)(a.pv + (size_t)R * B * K);
    a.inv_t = inv_t; a.seed = seed; a.qkeys = qkeys; a.floor = floor;
    hipStream_t st = (hipStream_t)stream;
    const bool floored = floor != nullptr;
    const auto lds = [&](int c, bool sr_lds, bool grouped) { return part_lds(c, d, K, a.L, sr_lds, grouped, NOISE, floored); };
    if (int rc = switch_c(C, [&](auto c) {
            if constexpr (NOISE) {
                return floored ? launch_pass<SampleFloorPart, true, c.value>(a, grid, lds, st)
                               : launch_pass<SamplePart, true, c.value>(a, grid, lds, st);
            } else {
                return floored ? launch_pass<SelectFloorPart, true, c.value>(a, grid, lds, st)
                               : launch_pass<SelectPart, true, c.value>(a, grid, lds, st);
            }
        }))
        return rc;
    hipLaunchKernelGGL(select_merge_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, a.pv, a.pi, (int)grid.x, B, K, s.id_lo, out_val,
                       out_idx);
    SREC_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int srec_score_select(const void* served, int K, const float* floor, float* out_val, int* out_idx, void* ws,
                                 void* stream) {
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    return select_launch<false>(*s, K, 1.f, 0ull, nullptr, floor, out_val, out_idx, ws, stream);
}

// ws: as srec_score_select_ws (the per-range lists hold keys where that call's hold scores)
extern "C" int srec_score_sample_ws(int B, int V, int d, int C, int L, int K, long* bytes) {
    return srec_score_select_ws(B, V, d, C, L, K, bytes);
}

extern "C" int srec_score_sample(const void* served, int K, float inv_temperature, unsigned long long seed,
                                 const int* session_keys, const float* floor, float* out_key, int* out_idx, void* ws,
                                 void* stream) {
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    if (!(inv_temperature > 0.f) || !(inv_temperature <= 3.402823466e+38f) || ((uintptr_t)session_keys & 3)) return SREC_BAD_ARG;
    return select_launch<true>(*s, K, inv_temperature, seed, session_keys, floor, out_key, out_idx, ws, stream);
}

// HOST: h [n_b, n_v] and w [n_b, n_v] of sample_noise.h for the sessions' keys (NULL: 0 .. n_b - 1) and the global ids
// (NULL: 0 .. n_v - 1); either output may be NULL.  No GPU is touched.
extern "C" int srec_sample_uniform(unsigned long long seed, const int* session_keys, int n_b, const int* ids, int n_v,
                                   unsigned* h_out, float* w_out) {
    if (n_b < 0 || n_v < 0 || (h_out == nullptr && w_out == nullptr)) return SREC_BAD_ARG;
    for (int b = 0; b < n_b; ++b) {
        const unsigned sk = srec_sample_skey(seed, (unsigned)(session_keys != nullptr ? session_keys[b] : b));
        for (int v = 0; v < n_v; ++v) {
            const unsigned h = srec_sample_hash(sk, (unsigned)(ids != nullptr ? ids[v] : v));
            if (h_out != nullptr) h_out[(size_t)b * n_v + v] = h;
            if (w_out != nullptr) w_out[(size_t)b * n_v + v] = srec_sample_w(h);
        }
    }
    return 0;
}
