// srec_score_rank: the RANK of every session's label among all catalog items WITHOUT materialising the (B, V) score
// matrix and without a K limit (evaluate: train.py:36-55 = model forward -> logits.topk(20); every HR / MRR / NDCG at any
// cutoff is a function of this one integer).  Scores may mix up to four soft-maxes (msgifsr.py:281-321: order fusion and
// the repeat / explore gate):
//   s[b,v] = logsumexp_{c<C}( cs[v] * <sr_c[b], E_v> + off[c,b] ),  off = off_in if v is in listed[b,:] else off_ex
// (C == 1: s = z + off, no exp / log).  rank[b] = #{ local rows v, id_lo + v != label_b : s[b,v] > target_b, or
// s[b,v] == target_b and id_lo + v < label_b } - the tie rule of topk.hip.  The label is left out BY ID, never by comparing
// its own score, so round-off cannot make it count against itself.  Counts of disjoint row ranges add up: a row-sharded
// table needs one integer all-reduce of rank (and one of target, which exactly one shard computes; the others write 0).
//
// Target pass (rank_target_kernel): one wavefront per session scores the label's row (off_in if the label is listed);
//   it also initialises rank[b] (0, or -1 for a label < 0).
// Count pass (rank_count_kernel, the hot path; its tile product is score_tile.h, shared with recommend.hip): workgroup = 32
//   sessions x one item range, 4 wavefronts.  The C session
//   tiles sit in LDS for the lifetime of the workgroup (C = 3, d = 256: 98 KB); each wavefront owns 32 items of a
//   128-item chunk whose rows stream straight from HBM into the B operand of v_mfma_f32_32x32x2_f32 (exact fp32): lane
//   (item r, half h) loads the float4 at columns 8j + 4h, the A lane reads the same columns of its session from LDS, so the
//   MFMA's two k slots of step i are columns 8j + i and 8j + 4 + i - a permutation of the sum, no staging of the table.
//   The C accumulator tiles of a (session, item) pair live in one lane: scale by cs[v], add off_ex, combine, compare with
//   target_b; one ballot + two popcounts per accumulator register count a session's items, partial counts meet in LDS and
//   leave with ONE integer atomicAdd per (session, workgroup).  Integer sums: the result does not depend on their order.
//   This pass treats every item as "ex".
// Fix-up pass (rank_fixup_kernel, only with a listed set): one wavefront per (b, j) scores u = listed[b,j] with off_ex and
//   with off_in (same routine as the target pass) and adds [ahead(s_in)] - [ahead(s_ex)].  The order-1 node list of a
//   session holds every item ONCE, so the lists need no dedup (a repeated id would be corrected twice).  The count pass saw
//   that item's "ex" score in the MFMA's summation order, this pass in a wavefront's: within round-off of the target the two
//   comparisons can disagree and the sum is off by one - callers clamp a live session's rank at 0.
// Session tiles that do not fit the 160 KB of LDS (896 B of per-session scalars + C * 32 * (d + 4) floats, d rounded up to
// 32: C * (d + 4) > 1273) are read through the cache instead - same code.
#include "common.h"
#include "score_tile.h"

namespace {

using namespace score_tile;      // SB sessions x CHUNK items per step, mix<C>, the MFMA tile product (score_tile.h)

struct RankArgs {
    const float* sr; int ld_sr; long comp_stride;
    const float* E; int ld_e;
    const float* cs;
    const float* off_ex; const float* off_in;
    const int* listed; int L;
    const int* labels; long id_lo;
    int B, V, d;
    float* target; int target_given;
    int* rank;
    int items_per_range;
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
    for (int i = tid; i < C * SB; i += 256) {
        const int c = i / SB, b = b0 + i % SB;
        offs[c * SB + i % SB] = (a.off_ex != nullptr && b < a.B) ? a.off_ex[(size_t)c * a.B + b] : 0.f;
    }
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    // A operand rows: this lane's session (clamped when read through the cache; such sessions count nothing)
    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);

    int clo[16], chi[16];                                // wave-uniform counts: session (r&3)+8(r>>2) and the one 4 above
#pragma unroll
    for (int r = 0; r < 16; ++r) { clo[r] = 0; chi[r] = 0; }

    for (int base = v0; base < v1; base += CHUNK) {
        const int v = base + wave * 32 + l31;
        const bool vok = v < v1;
        const float* brow = a.E + (size_t)min(v, a.V - 1) * a.ld_e + 4 * half;
        const float csv = (a.cs != nullptr && vok) ? a.cs[v] : 1.f;
        f32x16 acc[C];
        dots<C, SR_LDS>(arow, brow, d, half, acc);

        // per-lane epilogue: item v (this lane's column) against 16 sessions
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int sl = session_of(r, half);
            float z[C];
#pragma unroll
            for (int c = 0; c < C; ++c) z[c] = csv * acc[c][r] + offs[c * SB + sl];
            const float s = mix<C>(z);
            const float t = tgt[sl];
            const int lv = labs[sl];
            const bool hit = vok && v != lv && (s > t || (s == t && v < lv));
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

inline int pick_ranges(int B, int V) {
    const int tiles = cdiv(B, SB);
    int R = cdiv(1024, tiles);                                  // ~4 workgroups per CU (as topk.hip)
    const int maxR = cdiv(V, 2 * CHUNK);                        // at least 2 chunks per range
    if (R > maxR) R = maxR;
    return R < 1 ? 1 : R;
}

inline size_t count_lds(int C, int d, bool sr_lds) {
    const size_t head = (size_t)(SB + MAXCOMP * SB + SB + SB) * 4;
    return head + (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS>
int launch_count(const RankArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    static std::atomic<unsigned long long> optin{0};
    if (int rc = srec_lds_optin((const void*)rank_count_kernel<C, SR_LDS>, LDS_BYTES, optin)) return rc;
    hipLaunchKernelGGL((rank_count_kernel<C, SR_LDS>), grid, dim3(256), lds, st, a);
    return 0;
}

template <int C>
int run(const RankArgs& a0, hipStream_t st) {
    RankArgs a = a0;
    hipLaunchKernelGGL((rank_target_kernel<C>), dim3(cdiv(a.B, 4)), dim3(256), 0, st, a);
    if (a.rank == nullptr) {                                    // target pass only (a shard ahead of the sum over shards)
        SREC_LAUNCH_CHECK();
        return 0;
    }
    const int R = pick_ranges(a.B, a.V);
    a.items_per_range = cdiv(cdiv(a.V, R), CHUNK) * CHUNK;
    const dim3 grid(cdiv(a.V, a.items_per_range), cdiv(a.B, SB));
    const bool fits = count_lds(C, a.d, true) <= (size_t)LDS_BYTES;
    const int rc = fits ? launch_count<C, true>(a, grid, count_lds(C, a.d, true), st)
                        : launch_count<C, false>(a, grid, count_lds(C, a.d, false), st);
    if (rc) return rc;
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
    if (B <= 0 || V <= 0 || d <= 0 || (d & 3) || d > 1024 || C < 1 || C > MAXCOMP || L < 0 || L > MAXL || bytes == nullptr)
        return SREC_BAD_ARG;
    *bytes = 16;
    return 0;
}

extern "C" int srec_score_rank(const float* sr, int ld_sr, long comp_stride, const float* E, int ld_e, const float* cs,
                               const float* off_ex, const float* off_in, const int* listed, int L, const int* labels,
                               long id_lo, int B, int V, int d, int C, float* target, int target_given, int* rank, void* ws,
                               void* stream) {
    (void)ws;
    if (B <= 0) return 0;
    if (V <= 0 || d <= 0 || (d & 3) || d > 1024 || C < 1 || C > MAXCOMP || L < 0 || L > MAXL || (ld_sr & 3) || (ld_e & 3) ||
        (comp_stride & 3) || ((uintptr_t)E & 15) || ((uintptr_t)sr & 15) || labels == nullptr || target == nullptr ||
        (rank == nullptr && target_given) || id_lo < 0)
        return SREC_BAD_ARG;
    RankArgs a{};
    a.sr = sr; a.ld_sr = ld_sr; a.comp_stride = comp_stride; a.E = E; a.ld_e = ld_e; a.cs = cs;
    a.off_ex = off_ex; a.off_in = off_in; a.listed = L > 0 ? listed : nullptr; a.L = a.listed != nullptr ? L : 0;
    a.labels = labels; a.id_lo = id_lo; a.B = B; a.V = V; a.d = d; a.target = target; a.target_given = target_given;
    a.rank = rank;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: return run<1>(a, st);
        case 2: return run<2>(a, st);
        case 3: return run<3>(a, st);
        default: return run<4>(a, st);
    }
}
