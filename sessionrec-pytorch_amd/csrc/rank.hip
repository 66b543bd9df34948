// srec_score_rank: the RANK of every session's label among all catalog items WITHOUT materialising the (B, V) score
// matrix and without a K limit (evaluate: train.py:36-55 = model forward -> logits.topk(20); every HR / MRR / NDCG at any
// cutoff is a function of this one integer).  Scores may mix up to four soft-maxes (msgifsr.py:281-321: order fusion and
// the repeat / explore gate): the served score of score_pass.h, without a bias.
// rank[b] = #{ local rows v, id_lo + v != label_b : s[b,v] > target_b, or s[b,v] == target_b and id_lo + v < label_b } -
// the tie rule of topk.hip.  The label is left out BY ID, never by comparing its own score, so round-off cannot make it
// count against itself.  Counts of disjoint row ranges add up: a row-sharded table needs one integer all-reduce of rank
// (and one of target, which exactly one shard computes; the others write 0).
//
// Target pass (rank_target_kernel): one wavefront per session scores the label's row (off_in if the label is listed);
//   it also initialises rank[b] (0, or -1 for a label < 0).
// Count pass (rank_count_kernel, the hot path): the pass of score_pass.h with the listed set and the bias compiled out -
//   every item scores with off_ex.  A lane compares its (session, item) score with target_b; one ballot + two popcounts per
//   accumulator register count a session's items, partial counts meet in LDS and leave with ONE integer atomicAdd per
//   (session, workgroup).  Integer sums: the result does not depend on their order.
// Fix-up pass (rank_fixup_kernel, only with a listed set): one wavefront per (b, j) scores u = listed[b,j] with off_ex and
//   with off_in (same routine as the target pass) and adds [ahead(s_in)] - [ahead(s_ex)].  The order-1 node list of a
//   session holds every item ONCE, so the lists need no dedup (a repeated id would be corrected twice).  The count pass saw
//   that item's "ex" score in the MFMA's summation order, this pass in a wavefront's: within round-off of the target the two
//   comparisons can disagree and the sum is off by one - callers clamp a live session's rank at 0.
// LDS: 896 B of per-session scalars + the session tiles (C = 3, d = 256: 98 KB) when they fit 160 KB; C * 32 * (d + 4) floats,
// d rounded up to 32, do not when C * (d + 4) > 1273: they are read through the cache instead - same code.
#include "common.h"
#include "score_pass.h"

namespace {

using namespace score_tile;

struct RankArgs : PassArgs {
    const int* labels;
    float* target; int target_given;
    int* rank;
};

__device__ __forceinline__ bool ahead(float s, long id, float t, long lab) { return s > t || (s == t && id < lab); }

// one wavefront: raw dot products <sr_c[b], E_v>, c < C, the same value in every lane
template <int C>
__device__ __forceinline__ void wave_dots(const RankArgs& a, int b, long v, int lane, float (&dot)[C]) {
    const float* er = a.E + (size_t)v * a.ld_e;
#pragma unroll
    for (int c = 0; c < C; ++c) dot[c] = 0.f;
    for (int k = lane * 4; k < a.d; k += 256) {
        const float4 e4 = *reinterpret_cast<const float4*>(er + k);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* s = a.sr + (size_t)c * a.comp_stride + (size_t)b * a.ld_sr + k;
            dot[c] += e4.x * s[0] + e4.y * s[1] + e4.z * s[2] + e4.w * s[3];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) dot[c] = wave_sum(dot[c]);
}

template <int C>
__device__ __forceinline__ float score_of(const RankArgs& a, const float (&dot)[C], float csv, const float* off, int b) {
    float z[C];
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = csv * dot[c] + (off != nullptr ? off[(size_t)c * a.B + b] : 0.f);
    return mix<C>(z);
}

// one wavefront: is `id` among listed[b, :] ?
__device__ __forceinline__ bool is_listed(const RankArgs& a, int b, long id, int lane) {
    if (a.listed == nullptr || a.L <= 0) return false;
    const bool hit = lane < a.L && (long)a.listed[(size_t)b * a.L + lane] == id;
    return __ballot(hit) != 0ull;
}

template <int C>
__global__ __launch_bounds__(256) void rank_target_kernel(RankArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const long lab = a.labels[b];
    if (lane == 0 && a.rank != nullptr) a.rank[b] = lab < 0 ? -1 : 0;
    if (a.target_given) return;
    const long v = lab - a.id_lo;
    float t = 0.f;
    if (lab >= 0 && v >= 0 && v < a.V) {
        float dot[C];
        wave_dots<C>(a, b, v, lane, dot);
        const bool in = is_listed(a, b, lab, lane);
        t = score_of<C>(a, dot, a.cs != nullptr ? a.cs[v] : 1.f, in ? a.off_in : a.off_ex, b);
    }
    if (lane == 0) a.target[b] = t;
}

template <int C>
__global__ __launch_bounds__(256) void rank_fixup_kernel(RankArgs a) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= (long)a.B * a.L) return;
    const int b = (int)(p / a.L);
    const long lab = a.labels[b];
    const long u = a.listed[p];
    const long v = u - a.id_lo;
    if (lab < 0 || u < 0 || u == lab || v < 0 || v >= a.V) return;
    float dot[C];
    wave_dots<C>(a, b, v, lane, dot);
    const float csv = a.cs != nullptr ? a.cs[v] : 1.f;
    const float t = a.target[b];
    const int delta = (int)ahead(score_of<C>(a, dot, csv, a.off_in, b), u, t, lab) -
                      (int)ahead(score_of<C>(a, dot, csv, a.off_ex, b), u, t, lab);
    if (lane == 0 && delta != 0) atomicAdd(&a.rank[b], delta);
}

template <int C, bool SR_LDS>
__global__ __launch_bounds__(256) void rank_count_kernel(RankArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d;
    float* tgt = smem;                                   // [SB]
    float* offs = tgt + SB;                              // [MAXCOMP][SB]
    int* labs = reinterpret_cast<int*>(offs + MAXCOMP * SB);   // [SB] label - id_lo (clamped), or a value no row has
    int* cnt = labs + SB;                                // [SB]
    float* Ss = reinterpret_cast<float*>(cnt + SB);      // [C][SB][LD] (SR_LDS)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB;
    const int v0 = blockIdx.x * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);

    if (tid < SB) {
        const int b = b0 + tid;
        const bool ok = b < a.B && a.labels[b] >= 0;
        tgt[tid] = ok ? a.target[b] : INFINITY;          // nothing is ahead of +inf: dead sessions count nothing
        // label as a LOCAL row; labels owned by another shard keep their order relative to every local row
        long lv = ok ? (long)a.labels[b] - a.id_lo : -1;
        lv = lv < -1 ? -1 : (lv > (long)a.V ? (long)a.V : lv);
        labs[tid] = (int)lv;
        cnt[tid] = 0;
    }
    const PassLds<false> ps{offs};
    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    SCORE_PASS_PROLOGUE(0, a, ps, b0, v0, v1, tid, lane, wave)
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    // A operand rows: this lane's session (clamped when read through the cache; such sessions count nothing)
    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);

    int clo[16], chi[16];                                // wave-uniform counts: session (r&3)+8(r>>2) and the one 4 above
#pragma unroll
    for (int r = 0; r < 16; ++r) { clo[r] = 0; chi[r] = 0; }

    for (int base = v0; base < v1; base += CHUNK) {
        SCORE_PASS_LANE_ITEM(0, it, a, ps, base, v1, wave, l31, half)
        f32x16 acc[C];
        dots<C, SR_LDS>(arow, it.brow, d, half, acc);

        // per-lane epilogue: item v (this lane's column) against 16 sessions
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            SCORE_PASS_ITEM_SCORE(C, 0, it, acc, r, ps, wave, l31, half, sl, in, s, bias_ok)
            const float t = tgt[sl];
            const int lv = labs[sl];
            const bool hit = SCORE_PASS_ELIGIBLE(it, in, ps, true, bias_ok) && it.v != lv && (s > t || (s == t && it.v < lv));
            const unsigned long long m = __ballot(hit);
            clo[r] += __popc((unsigned)m);
            chi[r] += __popc((unsigned)(m >> 32));
        }
    }

    // lane i < 32 takes session i's count of this wavefront
    int mine = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int sl = (r & 3) + 8 * (r >> 2);
        if (lane == sl) mine = clo[r];
        if (lane == sl + 4) mine = chi[r];
    }
    if (lane < SB && mine != 0) atomicAdd(&cnt[lane], mine);
    __syncthreads();
    if (tid < SB && b0 + tid < a.B && cnt[tid] != 0 && a.labels[b0 + tid] >= 0) atomicAdd(&a.rank[b0 + tid], cnt[tid]);
}

inline size_t count_lds(int C, int d, bool sr_lds) {
    const size_t head = (size_t)(SB + MAXCOMP * SB + SB + SB) * 4;
    return head + (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS, int>
struct RankCount { static constexpr auto kernel = rank_count_kernel<C, SR_LDS>; };

template <int C>
int run(const RankArgs& a0, hipStream_t st) {
    RankArgs a = a0;
    hipLaunchKernelGGL((rank_target_kernel<C>), dim3(cdiv(a.B, 4)), dim3(256), 0, st, a);
    if (a.rank == nullptr) {                                    // target pass only (a shard ahead of the sum over shards)
        SREC_LAUNCH_CHECK();
        return 0;
    }
    const dim3 grid(split_ranges(a, pick_ranges(a.B, a.V, 1024, 2)), cdiv(a.B, SB));    // ~4 workgroups per CU (as topk.hip)
    const auto lds = [&](int c, bool sr_lds, bool) { return count_lds(c, a.d, sr_lds); };
    if (int rc = launch_pass<RankCount, false, C>(a, grid, lds, st)) return rc;
    if (a.listed != nullptr && a.L > 0) {
        const long n = (long)a.B * a.L;
        hipLaunchKernelGGL((rank_fixup_kernel<C>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, a);
    }
    SREC_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// rank == NULL (and !target_given): the target pass alone - a shard's share of target[], ahead of the sum over shards.
// no scratch is needed (partial counts meet through integer atomics); a token size keeps the caller's cache uniform
extern "C" int srec_score_rank_ws(int B, int V, int d, int C, int L, long* bytes) {
    if (bad_shape(B, V, d, C, L) || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = 16;
    return 0;
}

// the kernels here know neither a bias nor SREC_LISTED_DROP: a descriptor that carries one is refused, not half obeyed
extern "C" int srec_score_rank(const void* served, const int* labels, float* target, int target_given, int* rank, void* ws,
                               void* stream) {
    (void)ws;
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    RankArgs a{};
    if (pass_args(a, *s, false) || s->bias != nullptr || s->listed_mode != SREC_LISTED_SCORE || labels == nullptr ||
        target == nullptr || (rank == nullptr && target_given))
        return SREC_BAD_ARG;
    a.labels = labels; a.target = target; a.target_given = target_given; a.rank = rank;
    hipStream_t st = (hipStream_t)stream;
    return switch_c(s->C, [&](auto c) { return run<c.value>(a, st); });
}
