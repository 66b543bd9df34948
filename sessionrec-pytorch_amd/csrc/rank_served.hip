// srec_score_ahead: how many ELIGIBLE rows stand ahead of a given (label, target) pair per session under the BIASED served
// score of score_pass.h - the rank of the label among what a user is SHOWN (item_bias, allow / deny lists, exclude-seen, a
// truncation floor), without the (B, V) score matrix.  rank.hip counts under the plain score and refuses a bias and
// SREC_LISTED_DROP; this file is the route beside it, and rank.hip stays what it is.
//   ahead[b] = #{ local rows v : (b, v) eligible (SCORE_PASS_ELIGIBLE: v < V, not listed under SREC_LISTED_DROP, bias not
//                -INFINITY), id_lo + v != label_b, !(s'[b,v] < floor_b) with a floor, and
//                s'[b,v] > target_b or (s'[b,v] == target_b and id_lo + v < label_b) }           - the tie rule of rank.hip.
// The target is an INPUT: the label's served score is what srec_score_items returns (bias included, -INFINITY for a dropped
// item, shard results add up), so there is no target pass here.  The label is left out BY ID, never by comparing its own
// score, so the round-off between the two kernels' summation orders cannot make it count against itself.
// One kernel (ahead_count_kernel): the pass of score_pass.h WITH the listed set and the bias compiled in - listed items are
//   resolved inside the pass by the in-range mask (two barriers per chunk with a list, none without, as score_norm.hip), so
//   there is no fix-up pass and no count that can be off by one.  The epilogue is rank_count_kernel's: one ballot + two
//   popcounts per accumulator register, partial counts meet in LDS and leave with ONE integer atomicAdd per (session,
//   workgroup) into ahead[], which the entry point zeroes on the stream.  Integer sums: the result is a pure function of the
//   inputs, and the counts of disjoint row shards add up.  floor == NULL stages -INFINITY and runs the same instances.
//   A call WITHOUT a listed set (a deny list or a popularity correction alone) runs instances with the list machinery
//   compiled out (LISTS = false), as rank_count_kernel: the same scores, the same counts, the offsets read once per workgroup.
// LDS: the pass's 1.6 KB of offsets, mask and counts + 512 B of per-session scalars (target, label row, floor, count) + 32 L
// ids (+ 256 B of bias row offsets with G rows) + the session tiles when the sum stays within 160 KB, else the tiles are read
// through the cache - same code.
#include "common.h"
#include "score_pass.h"

namespace {

using namespace score_tile;

struct AheadArgs : PassArgs {
    const int* labels;              // [B] global ids (< 0: nothing is counted)
    const float* target;            // [B] the labels' served scores
    const float* floor;             // [B] or NULL
    int* ahead;                     // [B], zeroed by the entry point
};

inline size_t ahead_lds(int C, int d, int L, bool sr_lds, bool grouped) {
    return pass_lds(L, grouped) + (size_t)4 * SB * 4 + (sr_lds ? tile_bytes(C, d) : 0);
}

// LISTS = false (a call without a listed set): the list machinery is compiled out as in rank_count_kernel - every item scores
// with off_ex, whose LDS reads then leave the chunk loop (measured: profiles/served_rank_timing.md)
template <int C, bool SR_LDS, int BIAS, bool LISTS>
__global__ __launch_bounds__(256) void ahead_count_kernel(AheadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d, L = a.L;
    float* offs = smem;                                             // the pass's arrays (PassLds) among this kernel's:
    float* offi = offs + MAXCOMP * SB;
    unsigned* inm = reinterpret_cast<unsigned*>(offi + MAXCOMP * SB);
    int* nin = reinterpret_cast<int*>(inm + SB * 4);
    float* tgt = reinterpret_cast<float*>(nin + SB);                // [SB] the labels' scores (+inf: a session that counts nothing)
    float* flr = tgt + SB;                                          // [SB] the sessions' floors (-inf without one)
    int* labs = reinterpret_cast<int*>(flr + SB);                   // [SB] label - id_lo (clamped), or a value no row has
    int* cnt = labs + SB;                                           // [SB]
    int* lst = cnt + SB;
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(lst + SB * L);
    float* Ss = reinterpret_cast<float*>(goff + (BIAS == 2 ? SB : 0));  // [C][SB][LD] (SR_LDS); 16-byte aligned: all counts above are multiples of 4

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB;
    const int v0 = blockIdx.x * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const PassLds<LISTS> ps{offs, offi, inm, nin, lst, goff, LISTS && L > 0, a.drop != 0};

    if (tid < SB) {
        const int b = b0 + tid;
        const bool ok = b < a.B && a.labels[b] >= 0;
        tgt[tid] = ok ? a.target[b] : INFINITY;          // nothing is ahead of +inf: dead sessions count nothing
        flr[tid] = (ok && a.floor != nullptr) ? a.floor[b] : -INFINITY;
        // label as a LOCAL row; labels owned by another shard keep their order relative to every local row
        long lv = ok ? (long)a.labels[b] - a.id_lo : -1;
        lv = lv < -1 ? -1 : (lv > (long)a.V ? (long)a.V : lv);
        labs[tid] = (int)lv;
        cnt[tid] = 0;
    }
    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    // A operand rows: this lane's session (clamped when read through the cache; such sessions count nothing)
    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);

    int clo[16], chi[16];                                // wave-uniform counts: session (r&3)+8(r>>2) and the one 4 above
#pragma unroll
    for (int r = 0; r < 16; ++r) { clo[r] = 0; chi[r] = 0; }

    for (int base = v0; base < v1; base += CHUNK) {
        if (LISTS && ps.has_list) {
            __syncthreads();          // the epilogue of the previous chunk has read its membership bits
            SCORE_PASS_CHUNK_MASK(ps, L, base, tid)
        }
        SCORE_PASS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)
        f32x16 acc[C];
        dots<C, SR_LDS>(arow, it.brow, d, half, acc);
        if (LISTS && ps.has_list) __syncthreads(); // membership bits written

        // per-lane epilogue: item v (this lane's column) against 16 sessions
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            SCORE_PASS_ITEM_SCORE(C, BIAS, it, acc, r, ps, wave, l31, half, sl, in, s, bias_ok)
            const float t = tgt[sl];
            const int lv = labs[sl];
            const bool hit = SCORE_PASS_ELIGIBLE(it, in, ps, true, bias_ok) && it.v != lv && !(s < flr[sl]) &&
                             (s > t || (s == t && it.v < lv));
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
    // (cnt != 0 only for a live session with a label: tgt = +inf elsewhere)
    if (tid < SB && b0 + tid < a.B && cnt[tid] != 0) atomicAdd(&a.ahead[b0 + tid], cnt[tid]);
}

template <int C, bool SR_LDS, int BIAS>
struct AheadCount { static constexpr auto kernel = ahead_count_kernel<C, SR_LDS, BIAS, true>; };
template <int C, bool SR_LDS, int BIAS>
struct AheadCountPlain { static constexpr auto kernel = ahead_count_kernel<C, SR_LDS, BIAS, false>; };

}  // namespace

// no scratch is needed (partial counts meet through integer atomics); a token size keeps the ABI uniform
extern "C" int srec_score_ahead_ws(int B, int V, int d, int C, int L, long* bytes) {
    if (bad_shape(B, V, d, C, L) || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = 16;
    return 0;
}

extern "C" int srec_score_ahead(const void* served, const int* labels, const float* target, const float* floor, int* ahead,
                                void* ws, void* stream) {
    (void)ws;
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    AheadArgs a{};
    if (pass_args(a, *s, false) || labels == nullptr || target == nullptr || ahead == nullptr || ((uintptr_t)labels & 3) ||
        ((uintptr_t)target & 3) || ((uintptr_t)floor & 3) || ((uintptr_t)ahead & 3))
        return SREC_BAD_ARG;
    const int B = s->B, V = s->V, d = s->d, C = s->C;
    const dim3 grid(split_ranges(a, pick_ranges(B, V, 1024, 2)), cdiv(B, SB));     // ~4 workgroups per CU (as rank.hip)
    a.labels = labels; a.target = target; a.floor = floor; a.ahead = ahead;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(ahead, 0, (size_t)B * 4, st); e != hipSuccess) return (int)e;
    const auto lds = [&](int c, bool sr_lds, bool grouped) { return ahead_lds(c, d, a.L, sr_lds, grouped); };
    if (int rc = switch_c(C, [&](auto c) {
            return a.L > 0 ? launch_pass<AheadCount, true, c.value>(a, grid, lds, st)
                           : launch_pass<AheadCountPlain, true, c.value>(a, grid, lds, st);
        }))
        return rc;
    SREC_LAUNCH_CHECK();
    return 0;
}
