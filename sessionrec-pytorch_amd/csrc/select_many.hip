// srec_score_select_many_collect / _order: top-N lists beyond SREC_SELECT_MAXK (K <= SREC_SELECT_MANY_MAXK) under the served
// score (score_pass.h: score, eligibility, layouts and limits), WITHOUT the (B, V) score matrix and without a running list in
// LDS: srec_score_cutoff(top_k = K) gives every session the K-th best score as a floor, the collect pass appends everything
// at or above the floor to a global buffer, the order kernel sorts what was collected.
//
// Collect (collect_kernel): the pass of score_pass.h.  An eligible (session, row) pair SURVIVES when !(s' < floor[b]) - the
//   test of the FLOOR instances of select_part_kernel (recommend.hip), on the fp32 s' the cutoff compared.  Per 128-item chunk
//   every wavefront counts its survivors per session from the ballot (its two halves are two sessions), the four counts of a
//   session meet in LDS, ONE returned integer atomic per (workgroup, session, chunk) with survivors reserves the slots on the
//   session's counter n[b], and a lane's slot is base + the survivors of the lower wavefronts + the survivors below it in
//   the ballot.  A slot at or beyond cap is not written; the counter still counts it, so the caller sees n[b] > cap.
//   Arrival decides where a pair sits in the buffer, never what the buffer holds.  Two barriers per chunk (counts written /
//   bases written); the wave counts are double-buffered so that a wavefront may start the next chunk while another still
//   reads this one's.  The membership mask of the next chunk is written behind those barriers, so it needs none of its own
//   ahead of it.
// Order (order_kernel): one workgroup of 1024 threads per session.  The m = min(n[b], cap) pairs become 64-bit keys
//   (~key_of(s') << 32 | id; score_key.h), padded with all-ones to a power of two, and a bitonic network sorts them ascending
//   in LDS: (value descending, id ascending), the better() of recommend.hip.  Keys are distinct, so the output is a pure
//   function of the SET collected.  The first K go out as (score_of, id) - the value is s' + 0.0f - the rest of the K slots
//   as (-INFINITY, -1).
// No float atomics.  LDS: collect - the pass's 1.6 KB of offsets, mask and counts, 32 L ids (and 256 bytes of bias row offsets
// with G rows) + 128 bytes of floors + 128 bytes of bases + 1 KB of wave counts + the session tiles when the sum stays within
// 160 KB (C = 3, d = 256, L = 64, G rows: 108.6 KB; C = 4, d = 256: 141.1 KB), else the tiles are read through the cache;
// order - 8 bytes per key, 64 KB at SREC_SELECT_MANY_SORT = 8192 pairs.
#include "common.h"
#include "score_key.h"
#include "score_pass.h"

namespace {

using namespace score_tile;
typedef unsigned long long u64;

constexpr int MAXK = SREC_SELECT_MANY_MAXK;
constexpr int SORT = SREC_SELECT_MANY_SORT;
constexpr int ORDER_THREADS = 1024;
static_assert((SORT & (SORT - 1)) == 0 && SORT * 8 <= 64 * 1024, "the order kernel sorts a power of two of keys in 64 KB");
static_assert(MAXK <= SORT, "the list is a prefix of the sorted buffer");

struct ColArgs : PassArgs {
    const float* floor;             // [B]
    int cap;                        // slots per session
    float* bv; int* bi;             // [B][cap] (value, global id) in arrival order
    int* n;                         // [B] survivors (may exceed cap)
};

inline size_t col_lds(int C, int d, int L, bool sr_lds, bool grouped) {
    return pass_lds(L, grouped) + (size_t)(2 * SB + 2 * 4 * SB) * 4 + (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS, int BIAS>
__global__ __launch_bounds__(256) void collect_kernel(ColArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d, L = a.L;
    float* offs = smem;                                             // the pass's arrays (PassLds) among this kernel's:
    float* offi = offs + MAXCOMP * SB;
    unsigned* inm = reinterpret_cast<unsigned*>(offi + MAXCOMP * SB);
    int* nin = reinterpret_cast<int*>(inm + SB * 4);
    float* flr = reinterpret_cast<float*>(nin + SB);                // [SB] the sessions' floors
    int* sbase = reinterpret_cast<int*>(flr + SB);                  // [SB] first slot of the chunk's survivors
    int* wcnt = sbase + SB;                                         // [2][4][SB] survivors per (chunk parity, wavefront, session)
    int* lst = wcnt + 2 * 4 * SB;
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(lst + SB * L);
    float* Ss = reinterpret_cast<float*>(goff + (BIAS == 2 ? SB : 0));  // [C][SB][LD] (SR_LDS); 16-byte aligned: all counts above are multiples of 4

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB, range = blockIdx.x;
    const int v0 = range * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const PassLds<true> ps{offs, offi, inm, nin, lst, goff, L > 0, a.drop != 0};

    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    if (tid < SB) flr[tid] = b0 + tid < a.B ? a.floor[b0 + tid] : INFINITY;
    SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);
    const int cap = a.cap;
    const unsigned below = (1u << l31) - 1u;
    int par = 0;

    for (int base = v0; base < v1; base += CHUNK, par ^= 1) {
        // (the epilogue of the previous chunk read its membership bits ahead of that chunk's two barriers)
        if (ps.has_list) { SCORE_PASS_CHUNK_MASK(ps, L, base, tid) }
        SCORE_PASS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)
        f32x16 acc[C];
        dots<C, SR_LDS>(arow, it.brow, d, half, acc);
        if (ps.has_list) __syncthreads(); // membership bits written

        // per-lane epilogue: item v (this lane's column) against 16 sessions
        int* wc = wcnt + par * 4 * SB;
        float sv[16];
        unsigned keep = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            SCORE_PASS_ITEM_SCORE(C, BIAS, it, acc, r, ps, wave, l31, half, sl, in, s, bias_ok)
            const bool hit = SCORE_PASS_ELIGIBLE(it, in, ps, b0 + sl < a.B, bias_ok) && !(s < flr[sl]);
            sv[r] = s;
            keep |= hit ? 1u << r : 0u;
            const u64 mk = __ballot(hit);
            if (l31 == 0) wc[wave * SB + sl] = __popc(half ? (unsigned)(mk >> 32) : (unsigned)mk);
        }
        __syncthreads();                                            // the four wave counts of every session
        if (tid < SB) {
            const int tot = wc[tid] + wc[SB + tid] + wc[2 * SB + tid] + wc[3 * SB + tid];
            if (tot > 0) sbase[tid] = atomicAdd(&a.n[b0 + tid], tot);   // (tot > 0: the session is live)
        }
        __syncthreads();                                            // the bases
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool hit = (keep >> r) & 1u;
            const u64 mk = __ballot(hit);
            if (mk == 0ull) continue;                               // (wave-uniform; the plain case: survivors are sparse)
            if (hit) {
                const int sl = session_of(r, half);
                int pos = sbase[sl] + __popc((half ? (unsigned)(mk >> 32) : (unsigned)mk) & below);
                for (int w = 0; w < wave; ++w) pos += wc[w * SB + sl];
                if (pos < cap) {
                    const size_t at = (size_t)(b0 + sl) * cap + pos;
                    a.bv[at] = sv[r];
                    a.bi[at] = (int)(a.id_lo + it.v);
                }
            }
        }
    }
}

// one workgroup per session: keys ascending = (value descending, id ascending)
__global__ __launch_bounds__(ORDER_THREADS) void order_kernel(int cap, const int* __restrict__ n, const float* __restrict__ bv,
                                                              const int* __restrict__ bi, int K, float* __restrict__ out_val,
                                                              int* __restrict__ out_idx) {
    extern __shared__ __attribute__((aligned(16))) u64 keys[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int m = max(0, min(n[b], cap));
    int m2 = 1;
    while (m2 < m) m2 <<= 1;                                        // (<= the launch's LDS: cap rounded up the same way)
    const float* v = bv + (size_t)b * cap;
    const int* id = bi + (size_t)b * cap;
    for (int i = tid; i < m2; i += ORDER_THREADS)
        keys[i] = i < m ? ((u64)~key_of(v[i]) << 32) | (u64)(unsigned)id[i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= m2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (m2 >> 1); t += ORDER_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const u64 x = keys[i], y = keys[p];
                if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[p] = x; }
            }
            __syncthreads();
        }
    }
    float* ov = out_val + (size_t)b * K;
    int* oi = out_idx + (size_t)b * K;
    for (int i = tid; i < K; i += ORDER_THREADS) {
        const bool filled = i < m;
        const u64 key = filled ? keys[i] : 0ull;
        ov[i] = filled ? score_of(~(unsigned)(key >> 32)) : -INFINITY;
        oi[i] = filled ? (int)(unsigned)key : -1;
    }
}

template <int C, bool SR_LDS, int BIAS>
struct Collect { static constexpr auto kernel = collect_kernel<C, SR_LDS, BIAS>; };

inline int ranges(int B, int V) { return pick_ranges(B, V, 1024, 2); }  // ~4 workgroups per CU (as score_norm.hip)

}  // namespace

extern "C" int srec_score_select_many_collect(const void* served, const float* floor, int cap, float* buf_val, int* buf_idx,
                                              int* n, void* stream) {
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    ColArgs a{};
    if (pass_args(a, *s, true) || floor == nullptr || cap < 1 || buf_val == nullptr || buf_idx == nullptr || n == nullptr ||
        ((uintptr_t)floor & 3) || ((uintptr_t)buf_val & 3) || ((uintptr_t)buf_idx & 3) || ((uintptr_t)n & 3))
        return SREC_BAD_ARG;
    const int B = s->B, V = s->V, d = s->d, C = s->C;
    const dim3 grid(split_ranges(a, ranges(B, V)), cdiv(B, SB));
    a.floor = floor; a.cap = cap; a.bv = buf_val; a.bi = buf_idx; a.n = n;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(n, 0, (size_t)B * 4, st); e != hipSuccess) return (int)e;
    const auto lds = [&](int c, bool sr_lds, bool grouped) { return col_lds(c, d, a.L, sr_lds, grouped); };
    if (int rc = switch_c(C, [&](auto c) { return launch_pass<Collect, true, c.value>(a, grid, lds, st); })) return rc;
    SREC_LAUNCH_CHECK();
    return 0;
}

extern "C" int srec_score_select_many_order(int B, int cap, const int* n, const float* buf_val, const int* buf_idx, int K,
                                            float* out_val, int* out_idx, void* stream) {
    if (B <= 0) return 0;
    if (K < 1 || K > MAXK || cap < 1 || cap > SORT || n == nullptr || buf_val == nullptr || buf_idx == nullptr ||
        out_val == nullptr || out_idx == nullptr || ((uintptr_t)n & 3) || ((uintptr_t)buf_val & 3) || ((uintptr_t)buf_idx & 3) ||
        ((uintptr_t)out_val & 3) || ((uintptr_t)out_idx & 3))
        return SREC_BAD_ARG;
    int cap2 = 1;
    while (cap2 < cap) cap2 <<= 1;
    hipLaunchKernelGGL(order_kernel, dim3(B), dim3(ORDER_THREADS), (size_t)cap2 * 8, (hipStream_t)stream, cap, n, buf_val, buf_idx,
                       K, out_val, out_idx);
    SREC_LAUNCH_CHECK();
    return 0;
}
