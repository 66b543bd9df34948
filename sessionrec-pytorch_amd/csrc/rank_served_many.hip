// srec_score_ahead_many: srec_score_ahead (rank_served.hip) for M given items per session in ONE pass over the table - where
// each of M targets stands among what a user is SHOWN (rest-of-session evaluation, "where would these items land?").  The pass
// holds every (session, row) score in a register; it is compared with M thresholds instead of one.
//   ahead[b,j] = N[b,j] + A[b,j]  for a live slot (items[b,j] >= 0), 0 for an empty one
//   N[b,j] = #{ local rows v : (b, v) eligible (SCORE_PASS_ELIGIBLE), id_lo + v is NOT one of items[b,:], !(s'[b,v] < floor_b),
//               s'[b,v] > target[b,j] or (s'[b,v] == target[b,j] and id_lo + v < items[b,j]) }                  - the pass
//   A[b,j] = #{ i != j live : items[b,i] != items[b,j], target[b,i] > -inf, !(target[b,i] < floor_b),
//               target[b,i] > target[b,j] or (target[b,i] == target[b,j] and items[b,i] < items[b,j]) }  - among themselves
// The session's own targets are left out of the pass BY ID and ordered among themselves by their GIVEN values (the rule of
// rank_served.hip for its one label): round-off between the gather kernel and the pass cannot make a target count against
// itself or two targets count against each other.  With M == 1 the result is srec_score_ahead's.
// One kernel (ahead_many_kernel) on the pass skeleton of score_pass.h, listed set and bias compiled in as in ahead_count_kernel:
//   prologue, once per workgroup: the 32 sessions' live (target, id) pairs are ORDERED in LDS by (value descending, id
//     ascending, column ascending) with a counting rank (<= 64 x 64 comparisons per session); the target ids inside the
//     workgroup's row range are compacted, and SCORE_PASS_CHUNK_MASK builds a second 128-bit mask per chunk from them - "this
//     row is a target of this session".
//   per (session, row) score: against the ordered thresholds "row is ahead of threshold q" is monotone in q, so a row adds 1 to
//     exactly one bucket p = the first q it is ahead of, and N of ordered position q is the prefix sum of the buckets up to q.
//     A row ahead of the BEST threshold goes through ballot + popcount into wave-uniform registers (ahead_count_kernel's
//     epilogue); a row not ahead of the WORST one does nothing; a wavefront with a row in between searches (branch-free, at
//     most 6 LDS reads per pair, the 16 searches of a lane independent of each other) and adds 1 in LDS.
//   epilogue: prefix sum per session, the permutation undone, ONE integer atomicAdd per non-zero (session, slot, workgroup)
//     into ahead[B, M], which the entry point zeroes on the stream.  The workgroups of the first item range add A: in the
//     ordered list it is the number of showable targets in front.
// Integer sums only: the output is a pure function of the inputs, counts of disjoint row shards add up, no scratch.  A NaN
// among a session's target values is the caller's error, as a duplicate id is: nothing faults and the output stays a function
// of the inputs (the value is staged as -inf, so the ordering is total), but that session's counts are unspecified.
// LDS: ahead_count_kernel's + (12 * 32 + 4 + 5 * 32 * MP) * 4 bytes: 1 552 bytes of per-session scalars, the target mask and
// the flag word (padded to 4 words to keep the arrays behind it 16-byte aligned) + 5 arrays [32][MP] (MP = M rounded up to a
// power of two: thresholds, their local rows, buckets, positions, in-range rows) = 42 512 bytes at M = 64, 6 672 at M = 5
// + the session tiles when the sum stays within 160 KB, else the tiles are read through the cache - same code.
#include "common.h"
#include "score_pass.h"

namespace {

using namespace score_tile;

struct AheadManyArgs : PassArgs {
    const int* items;               // [B, M] global ids, row stride ld_items (< 0: an empty slot)
    const float* target;            // [B, M] the items' served scores, row stride ld_items
    long ld_items;
    int M, MP;                      // MP: M rounded up to a power of two (the LDS row stride)
    const float* floor;             // [B] or NULL
    int among;                      // add A (the first item range's workgroups do)
    int* ahead;                     // [B, M], zeroed by the entry point
};

inline int pow2_at_least(int m) {
    int p = 1;
    while (p < m) p <<= 1;
    return p;
}

inline size_t ahead_many_lds(int C, int d, int L, int MP, bool sr_lds, bool grouped) {
    return pass_lds(L, grouped) + (size_t)(8 * SB + 4 * SB + 4 + 5 * SB * MP) * 4 + (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS, int BIAS, bool LISTS>
__global__ __launch_bounds__(256) void ahead_many_kernel(AheadManyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d, L = a.L, M = a.M, MP = a.MP;
    float* offs = smem;                                             // the pass's arrays (PassLds) among this kernel's:
    float* offi = offs + MAXCOMP * SB;
    unsigned* inm = reinterpret_cast<unsigned*>(offi + MAXCOMP * SB);
    int* nin = reinterpret_cast<int*>(inm + SB * 4);
    float* tb = reinterpret_cast<float*>(nin + SB);                 // [SB] the best threshold's value (+inf: nothing is counted)
    int* ub = reinterpret_cast<int*>(tb + SB);                      // [SB] ... and its local row
    float* tw = reinterpret_cast<float*>(ub + SB);                  // [SB] the worst live threshold
    int* uw = reinterpret_cast<int*>(tw + SB);
    float* flr = reinterpret_cast<float*>(uw + SB);                 // [SB] the sessions' floors (-inf without one)
    int* nlv = reinterpret_cast<int*>(flr + SB);                    // [SB] live slots
    int* cnt = nlv + SB;                                            // [SB] rows ahead of the best threshold
    int* tnin = cnt + SB;                                           // [SB] target ids inside this workgroup's range
    unsigned* tinm = reinterpret_cast<unsigned*>(tnin + SB);        // [SB][4] targets of this chunk
    int* anyt = reinterpret_cast<int*>(tinm + SB * 4);              // [0]: some session has a target in this range ([1..3]: padding)
    int* lst = anyt + 4;
    float* thr = reinterpret_cast<float*>(lst + SB * L);            // [SB][MP] thresholds in order, -inf behind the live ones
    int* uid = reinterpret_cast<int*>(thr + SB * MP);               // [SB][MP] their local rows (clamped to [-1, V])
    float* rawt = reinterpret_cast<float*>(uid + SB * MP);          // [SB][MP] the values as given ...
    int* bkt = reinterpret_cast<int*>(rawt);                        //          ... then the buckets
    int* rawu = bkt + SB * MP;                                      // [SB][MP] the ids as given (-1: empty) ...
    int* posn = rawu;                                               //          ... then column -> ordered position (-1: empty)
    int* tlst = rawu + SB * MP;                                     // [SB][MP] in-range targets as local rows
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(tlst + SB * MP);
    float* Ss = reinterpret_cast<float*>(goff + (BIAS == 2 ? SB : 0));  // [C][SB][LD] (SR_LDS); 16-byte aligned: all counts above are multiples of 4

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB;
    const int v0 = blockIdx.x * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const PassLds<LISTS> ps{offs, offi, inm, nin, lst, goff, LISTS && L > 0, a.drop != 0};
    const int lmp = 31 - __clz(MP);

    if (tid < SB) {
        const int b = b0 + tid;
        flr[tid] = (b < a.B && a.floor != nullptr) ? a.floor[b] : -INFINITY;
        nlv[tid] = 0;
        cnt[tid] = 0;
        tnin[tid] = 0;
    }
    if (tid < SB * 4) tinm[tid] = 0u;
    if (tid < 4) anyt[tid] = 0;
    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)
    for (int i = tid; i < SB * MP; i += 256) {
        const int sb = i >> lmp, j = i & (MP - 1), b = b0 + sb;
        int u = -1;
        float t = 0.f;
        if (b < a.B && j < M) {
            u = a.items[(size_t)b * a.ld_items + j];
            if (u >= 0) t = a.target[(size_t)b * a.ld_items + j];
            if (t != t) t = -INFINITY;       // a NaN (the caller's error) is ordered and counted as -inf: the order stays total
        }
        rawu[i] = u < 0 ? -1 : u;
        rawt[i] = t;
        thr[i] = -INFINITY;
        uid[i] = a.V;
    }
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    // counting rank of every live pair among its session's: (value descending, id ascending, column ascending) - a total
    // order (no NaN is left), so the positions are distinct and < the session's live count, and no two threads write one slot
    int rk[SB * SREC_AHEAD_MAXT / 256];
#pragma unroll
    for (int k = 0; k < SB * SREC_AHEAD_MAXT / 256; ++k) {
        const int i = tid + 256 * k;
        rk[k] = -1;
        if (i < SB * MP) {
            const int sb = i >> lmp, j = i & (MP - 1);
            const int u = rawu[i];
            if (u >= 0) {
                const float t = rawt[i];
                int n = 0;
                for (int o = 0; o < M; ++o) {
                    const int uo = rawu[sb * MP + o];
                    const float to = rawt[sb * MP + o];
                    n += (uo >= 0 && (to > t || (to == t && (uo < u || (uo == u && o < j))))) ? 1 : 0;
                }
                rk[k] = n;
                thr[sb * MP + n] = t;
                // as a LOCAL row; targets owned by another shard keep their order relative to every local row
                long lv = (long)u - a.id_lo;
                lv = lv < -1 ? -1 : (lv > (long)a.V ? (long)a.V : lv);
                uid[sb * MP + n] = (int)lv;
                atomicAdd(&nlv[sb], 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SB * SREC_AHEAD_MAXT / 256; ++k) {
        const int i = tid + 256 * k;
        if (i < SB * MP) {
            posn[i] = rk[k];
            bkt[i] = 0;
        }
    }
    if (tid < SB) {
        const int nl = nlv[tid];
        tb[tid] = nl > 0 ? thr[tid * MP] : INFINITY;               // nothing is ahead of +inf: dead sessions count nothing
        ub[tid] = nl > 0 ? uid[tid * MP] : -1;
        tw[tid] = nl > 0 ? thr[tid * MP + nl - 1] : INFINITY;
        uw[tid] = nl > 0 ? uid[tid * MP + nl - 1] : -1;
    }
    // the session's targets inside [v0, v1) compacted to the front of its tlst row (ballot prefix, as SCORE_PASS_PROLOGUE
    // does for the listed ids; the clamped rows -1 and V are outside every range)
    for (int sb = wave; sb < SB; sb += 4) {
        const int nl = nlv[sb];
        bool ok = false;
        int loc = 0;
        if (lane < nl) {
            loc = uid[sb * MP + lane];
            ok = loc >= v0 && loc < v1;
        }
        const unsigned long long mk = __ballot(ok);
        if (ok) tlst[sb * MP + __popcll(mk & ((1ull << lane) - 1ull))] = loc;
        if (lane == 0) {
            tnin[sb] = __popcll(mk);
            if (mk != 0ull) atomicOr(&anyt[0], 1);
        }
    }
    __syncthreads();
    const bool has_t = anyt[0] != 0;
    const PassLds<true> pt{nullptr, nullptr, tinm, tnin, tlst, nullptr, has_t, false};
    const bool masks = (LISTS && ps.has_list) || has_t;

    // A operand rows: this lane's session (clamped when read through the cache; such sessions count nothing)
    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);

    int clo[16], chi[16];                                // wave-uniform counts: session (r&3)+8(r>>2) and the one 4 above
#pragma unroll
    for (int r = 0; r < 16; ++r) { clo[r] = 0; chi[r] = 0; }

    for (int base = v0; base < v1; base += CHUNK) {
        if (masks) {
            __syncthreads();          // the epilogue of the previous chunk has read its membership bits
            SCORE_PASS_CHUNK_MASK(ps, L, base, tid)
            SCORE_PASS_CHUNK_MASK(pt, MP, base, tid)
        }
        SCORE_PASS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)
        f32x16 acc[C];
        dots<C, SR_LDS>(arow, it.brow, d, half, acc);
        if (masks) __syncthreads(); // membership bits written

        // per-lane epilogue: item v (this lane's column) against 16 sessions
        float sv[16];
        unsigned midm = 0u;                              // bit r: the pair is behind the best threshold and ahead of the worst
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            SCORE_PASS_ITEM_SCORE(C, BIAS, it, acc, r, ps, wave, l31, half, sl, in, s, bias_ok)
            // (read even where no session has a target in this range - the mask is zero then: behind the workgroup-uniform
            // has_t the read bought nothing at M = 1 and cost 7 % at M = 64, measured)
            const bool tin = (tinm[sl * 4 + wave] >> l31) & 1u;
            const bool hit = SCORE_PASS_ELIGIBLE(it, in, ps, true, bias_ok) && !tin && !(s < flr[sl]);
            const float t0 = tb[sl];
            const bool a0 = s > t0 || (s == t0 && it.v < ub[sl]);
            const unsigned long long m = __ballot(hit && a0);
            clo[r] += __popc((unsigned)m);
            chi[r] += __popc((unsigned)(m >> 32));
            sv[r] = s;
            if (M > 1) {
                const float t1 = tw[sl];
                const bool a1 = s > t1 || (s == t1 && it.v < uw[sl]);
                if (hit && !a0 && a1) midm |= 1u << r;
            }
        }
        if (M > 1 && __any(midm != 0u)) {
            // the thresholds a row is surely behind form a prefix: th[q] > s (written so that a NaN is behind all).  The steps
            // are the outer loop: the 16 reads of a step are independent, so their LDS latencies overlap
            int p[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = session_of(r, half) * MP;
            for (int step = MP >> 1; step > 0; step >>= 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (!(sv[r] >= thr[p[r] + step - 1])) p[r] += step;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if ((midm >> r) & 1u) {
                    // the last step and the ties: the row is ahead of the worst live threshold, so q stops there at the latest
                    const int sl = session_of(r, half);
                    const float s = sv[r];
                    const int last = sl * MP + nlv[sl] - 1;
                    int q = p[r];
                    while (q < last && (thr[q] > s || (thr[q] == s && !(it.v < uid[q])))) ++q;
                    atomicAdd(&bkt[q], 1);
                }
            }
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
    // per session: N of ordered position q = the rows ahead of the best threshold + the buckets up to q; the first item
    // range adds A, the showable targets in front of q
    if (tid < SB) {
        const int nl = nlv[tid];
        const bool addA = a.among != 0 && blockIdx.x == 0;
        const float f = flr[tid];
        int run = cnt[tid], front = 0;
        for (int q = 0; q < nl; ++q) {
            run += bkt[tid * MP + q];
            bkt[tid * MP + q] = run + front;
            const float t = thr[tid * MP + q];
            if (addA && t > -INFINITY && !(t < f)) ++front;
        }
    }
    __syncthreads();
    for (int i = tid; i < SB * MP; i += 256) {
        const int sb = i >> lmp, j = i & (MP - 1), b = b0 + sb;
        const int q = posn[i];
        if (q >= 0 && b < a.B && j < M) {
            const int n = bkt[sb * MP + q];
            if (n != 0) atomicAdd(&a.ahead[(size_t)b * M + j], n);
        }
    }
}

template <int C, bool SR_LDS, int BIAS>
struct AheadMany { static constexpr auto kernel = ahead_many_kernel<C, SR_LDS, BIAS, true>; };
template <int C, bool SR_LDS, int BIAS>
struct AheadManyPlain { static constexpr auto kernel = ahead_many_kernel<C, SR_LDS, BIAS, false>; };

}  // namespace

// no scratch is needed (partial counts meet through integer atomics); a token size keeps the ABI uniform
extern "C" int srec_score_ahead_many_ws(int B, int V, int d, int C, int L, int M, long* bytes) {
    if (bad_shape(B, V, d, C, L) || M < 1 || M > SREC_AHEAD_MAXT || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = 16;
    return 0;
}

extern "C" int srec_score_ahead_many(const void* served, const int* items, const float* target, long ld_items, int M,
                                     const float* floor, int among_targets, int* ahead, void* ws, void* stream) {
    (void)ws;
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    AheadManyArgs a{};
    if (pass_args(a, *s, false) || M < 1 || M > SREC_AHEAD_MAXT || ld_items < (long)M || items == nullptr || target == nullptr ||
        ahead == nullptr || ((uintptr_t)items & 3) || ((uintptr_t)target & 3) || ((uintptr_t)floor & 3) || ((uintptr_t)ahead & 3))
        return SREC_BAD_ARG;
    const int B = s->B, V = s->V, d = s->d, C = s->C;
    const dim3 grid(split_ranges(a, pick_ranges(B, V, 1024, 2)), cdiv(B, SB));     // as srec_score_ahead
    a.items = items; a.target = target; a.ld_items = ld_items; a.M = M; a.MP = pow2_at_least(M); a.floor = floor;
    a.among = among_targets != 0; a.ahead = ahead;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(ahead, 0, (size_t)B * M * 4, st); e != hipSuccess) return (int)e;
    const auto lds = [&](int c, bool sr_lds, bool grouped) { return ahead_many_lds(c, d, a.L, a.MP, sr_lds, grouped); };
    if (int rc = switch_c(C, [&](auto c) {
            return a.L > 0 ? launch_pass<AheadMany, true, c.value>(a, grid, lds, st)
                           : launch_pass<AheadManyPlain, true, c.value>(a, grid, lds, st);
        }))
        return rc;
    SREC_LAUNCH_CHECK();
    return 0;
}
