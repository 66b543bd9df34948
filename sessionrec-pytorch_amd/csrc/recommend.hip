// srec_score_select: the K best catalog items of every session (K <= 128) under the score of srec_score_rank, WITHOUT the
// (B, V) score matrix - the serving path (model.recommend).  Same score, layouts and limits as rank.hip:
//   s[b,v] = logsumexp_{c<C}( cs[v] * <sr_c[b], E_v> + off[c,b] ),  off = off_in if v is in listed[b,:] else off_ex
// (C == 1: s = z + off, no exp / log); 1 <= C <= 4, d % 4 == 0, d <= 1024, L <= 64, cs / off_* / listed nullable.
// listed_mode SREC_LISTED_SCORE: listed items score with off_in; SREC_LISTED_DROP: listed items are never returned (off_in
// is not read).  Output: values descending, global ids id_lo + row, ties towards the lower id (topk.hip, rank.hip); a
// session with fewer than K eligible rows ends in (-INFINITY, -1) slots; K > V is legal.
//
// Pass 1 (select_part_kernel): workgroup = 32 sessions x one item range, 4 wavefronts, the tile product of rank.hip
//   (score_tile.h: session tiles in LDS or through the cache, item rows streamed into the MFMA B operand, a (session, item)
//   score in one lane).  Every session keeps its running K best in LDS, sorted by (value desc, id asc).  A lane whose item
//   beats the session's K-th best writes the score to slot [session][item of the chunk] of a candidate array and the
//   wavefront's ballot to a survivor mask: one slot per item of the chunk, so the list cannot overflow (a chunk in which
//   EVERY item is a candidate - the first one, or scores that rise with the id - is the plain case), and no atomics at all.
//   One wavefront per session then merges the survivors into the sorted list: every entry's new position is its own
//   position plus the number of entries of the other side that are better (candidates: binary search in the list), a
//   permutation because (value, id) keys are distinct.  Cost O((K + n) n / 64) per merge, nothing when no item survived.
//   Listed items: the ids of a session that fall into the workgroup's range are compacted in LDS once; per chunk a
//   128-bit membership mask per session is built from them (usually zero to two entries).
// Pass 2 (select_merge_kernel): one wavefront per session folds the per-range lists with the same merge.
// The output is a pure function of the inputs: positions come from comparisons of (value, id) keys, never from arrival.
// LDS: 1.5 KB of offsets and masks + 32 K (value, id) pairs + 17 KB candidates + 32 L ids + the session tiles when the sum
// stays within 160 KB (C = 3, d = 256, K = 128, L = 64: 156.5 KB), else the tiles are read through the cache.
//
// srec_score_select_biased: s' = s + bias[group[b], v], a per-item fp32 operand added AFTER the mixture; -INFINITY = the item is
// not in the catalogue for this session: it never enters a list (a condition of `hit`, not a consequence of its score - an
// item that merely scores -INFINITY still beats an unfilled slot, as before).  BIAS is a template parameter: 0 = none (the
// instances of srec_score_select, unchanged), 1 = one row for all sessions (the lane that owns item v loads bias[v] once per
// chunk beside its column scale), 2 = G rows (the 32 sessions' row offsets are staged in LDS, 256 bytes counted by
// part_lds; a lane loads its item's bias for its 16 sessions ahead of the tile product, every load coalesced over the 32
// items of a half-wavefront).  With the 256 bytes the C = 3, d = 256, K = 128, L = 64 case is 156.9 KB: still LDS tiles.
#include "common.h"
#include "score_tile.h"

namespace {

using namespace score_tile;

constexpr int MAXK = 128;
constexpr int CST = CHUNK + 8;      // candidate row stride: sessions sl and sl + 4 (the two lane halves) 32 banks apart
constexpr int EMPTY = 0x7fffffff;   // id of an unfilled list slot: behind every real item of the same value

struct SelArgs {
    const float* sr; int ld_sr; long comp_stride;
    const float* E; int ld_e;
    const float* cs;
    const float* off_ex; const float* off_in;
    const int* listed; int L; int drop;
    long id_lo;
    int B, V, d, K;
    int items_per_range;
    float* pv; int* pi;             // [R][B][K] per-range lists (local rows; EMPTY = unfilled)
    const float* bias; long ld_bias; // (appended: the unbiased instances read the arguments above where they were)
    const int* group; int G;
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

inline size_t part_lds(int C, int d, int K, int L, bool sr_lds, bool grouped = false) {
    const size_t head = (size_t)(2 * MAXCOMP * SB + SB * 4 + SB * 4 + SB) * 4;
    return head + (size_t)SB * K * 8 + (size_t)SB * CST * 4 + (size_t)SB * L * 4 + (grouped ? (size_t)SB * 8 : 0) +
           (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS, int BIAS>
__global__ __launch_bounds__(256) void select_part_kernel(SelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d, K = a.K, L = a.L;
    float* offs = smem;                                             // [MAXCOMP][SB] off_ex
    float* offi = offs + MAXCOMP * SB;                              // [MAXCOMP][SB] off_in (SCORE mode)
    unsigned* inm = reinterpret_cast<unsigned*>(offi + MAXCOMP * SB);   // [SB][4] listed items of this chunk
    unsigned* surv = inm + SB * 4;                                  // [SB][4] survivors of this chunk
    int* nin = reinterpret_cast<int*>(surv + SB * 4);               // [SB] listed ids inside this workgroup's range
    float* lv = reinterpret_cast<float*>(nin + SB);                 // [SB][K] running best values
    int* li = reinterpret_cast<int*>(lv + SB * K);                  // [SB][K] ... and local rows
    float* cand = reinterpret_cast<float*>(li + SB * K);            // [SB][CST] scores of this chunk's survivors
    int* lst = reinterpret_cast<int*>(cand + SB * CST);             // [SB][L] listed ids as local rows, in-range ones first
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(lst + SB * L);   // [SB] bias row offsets (BIAS == 2 only)
    float* Ss = reinterpret_cast<float*>(goff + (BIAS == 2 ? SB : 0));  // [C][SB][LD] (SR_LDS); 16-byte aligned: all counts above are multiples of 4

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB, range = blockIdx.x;
    const int v0 = range * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const bool has_list = L > 0;
    const bool drop = a.drop != 0;

    for (int i = tid; i < C * SB; i += 256) {
        const int c = i / SB, b = b0 + i % SB;
        offs[i] = (a.off_ex != nullptr && b < a.B) ? a.off_ex[(size_t)c * a.B + b] : 0.f;
        offi[i] = (a.off_in != nullptr && b < a.B && !drop) ? a.off_in[(size_t)c * a.B + b] : 0.f;
    }
    for (int i = tid; i < SB * K; i += 256) { lv[i] = -INFINITY; li[i] = EMPTY; }
    if (tid < SB * 4) inm[tid] = 0u;
    if constexpr (BIAS == 2) {
        // sessions past the batch read row 0; an id outside [0, G) is the caller's error and is held inside the operand
        if (tid < SB) goff[tid] = b0 + tid < a.B ? (unsigned long long)min(max(a.group[b0 + tid], 0), a.G - 1) * a.ld_bias : 0ull;
    }
    if (has_list) {
        // the session's listed ids inside [v0, v1), compacted to the front of its row in list order (ballot prefix)
        for (int j = wave; j < SB; j += 4) {
            const int b = b0 + j;
            bool ok = false; int loc = 0;
            if (lane < L && b < a.B) {
                const long u = a.listed[(size_t)b * L + lane];
                const long lr = u - a.id_lo;
                ok = u >= 0 && lr >= (long)v0 && lr < (long)v1;
                loc = (int)lr;
            }
            const unsigned long long mk = __ballot(ok);
            if (ok) lst[j * L + __popcll(mk & ((1ull << lane) - 1ull))] = loc;
            if (lane == 0) nin[j] = __popcll(mk);
        }
    }
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);

    for (int base = v0; base < v1; base += CHUNK) {
        if (has_list && tid < SB * 4) {                             // thread (session, 32-item word): membership bits
            const int j = tid >> 2, w = tid & 3, n = nin[j];
            unsigned bits = 0u;
            for (int i = 0; i < n; ++i) {
                const int o = lst[j * L + i] - base - 32 * w;
                if (o >= 0 && o < 32) bits |= 1u << o;
            }
            inm[tid] = bits;
        }
        const int v = base + wave * 32 + l31;
        const bool vok = v < v1;
        const float* brow = a.E + (size_t)min(v, a.V - 1) * a.ld_e + 4 * half;
        const float csv = (a.cs != nullptr && vok) ? a.cs[v] : 1.f;
        float bv = 0.f;               // BIAS == 1: this lane's item, all sessions
        float bg[BIAS == 2 ? 16 : 1]; // BIAS == 2: this lane's item, its 16 sessions (under way during the tile product)
        if constexpr (BIAS == 1) bv = vok ? a.bias[v] : 0.f;
        if constexpr (BIAS == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) bg[r] = a.bias[goff[session_of(r, half)] + min(v, a.V - 1)];
        }
        f32x16 acc[C];
        dots<C, SR_LDS>(arow, brow, d, half, acc);
        __syncthreads();              // membership bits written; the merges of the previous chunk are done

        // per-lane epilogue: item v (this lane's column) against 16 sessions
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int sl = session_of(r, half);
            const bool in = has_list && ((inm[sl * 4 + wave] >> l31) & 1u);
            const float* of = in ? offi : offs;
            float z[C];
#pragma unroll
            for (int c = 0; c < C; ++c) z[c] = csv * acc[c][r] + of[c * SB + sl];
            float s = mix<C>(z);
            bool elig = true;         // a bias of -INFINITY: not in the catalogue of this session
            if constexpr (BIAS != 0) {
                const float bb = BIAS == 1 ? bv : bg[BIAS == 2 ? r : 0];
                s += bb;
                elig = bb != -INFINITY;
            }
            const bool hit = vok && b0 + sl < a.B && !(in && drop) && elig && better(s, v, lv[sl * K + K - 1], li[sl * K + K - 1]);
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

inline int pick_ranges(int B, int V) {
    const int tiles = cdiv(B, SB);
    int R = cdiv(512, tiles);                                   // the lists and tiles leave room for one or two workgroups per CU
    const int maxR = cdiv(V, 4 * CHUNK);                        // at least 4 chunks per range: the first chunk fills the list
    if (R > maxR) R = maxR;
    return R < 1 ? 1 : R;
}

template <int C, bool SR_LDS, int BIAS>
int launch_part(const SelArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    static std::atomic<unsigned long long> optin{0};
    if (int rc = srec_lds_optin((const void*)select_part_kernel<C, SR_LDS, BIAS>, LDS_BYTES, optin)) return rc;
    hipLaunchKernelGGL((select_part_kernel<C, SR_LDS, BIAS>), grid, dim3(256), lds, st, a);
    return 0;
}

template <int C, int BIAS>
int run_part(const SelArgs& a, dim3 grid, hipStream_t st) {
    const bool fits = part_lds(C, a.d, a.K, a.L, true, BIAS == 2) <= (size_t)LDS_BYTES;
    return fits ? launch_part<C, true, BIAS>(a, grid, part_lds(C, a.d, a.K, a.L, true, BIAS == 2), st)
                : launch_part<C, false, BIAS>(a, grid, part_lds(C, a.d, a.K, a.L, false, BIAS == 2), st);
}

template <int C>
int run(const SelArgs& a, int R, float* out_val, int* out_idx, hipStream_t st) {
    const dim3 grid(R, cdiv(a.B, SB));
    const int rc = a.bias == nullptr ? run_part<C, 0>(a, grid, st)
                   : a.G == 1        ? run_part<C, 1>(a, grid, st)
                                     : run_part<C, 2>(a, grid, st);
    if (rc) return rc;
    hipLaunchKernelGGL(select_merge_kernel, dim3(cdiv(a.B, 4)), dim3(256), 0, st, a.pv, a.pi, R, a.B, a.K, a.id_lo, out_val,
                       out_idx);
    SREC_LAUNCH_CHECK();
    return 0;
}

bool bad_shape(int B, int V, int d, int C, int L, int K) {
    return B <= 0 || V <= 0 || d <= 0 || (d & 3) || d > 1024 || C < 1 || C > MAXCOMP || L < 0 || L > MAXL || K < 1 || K > MAXK;
}

}  // namespace

// ws: the per-range partial lists, (value, row) pairs
extern "C" int srec_score_select_ws(int B, int V, int d, int C, int L, int K, long* bytes) {
    if (bad_shape(B, V, d, C, L, K) || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = (long)pick_ranges(B, V) * B * K * 8;
    return 0;
}

extern "C" int srec_score_select_biased(const float* sr, int ld_sr, long comp_stride, const float* E, int ld_e, const float* cs,
                                        const float* off_ex, const float* off_in, const int* listed, int L, int listed_mode,
                                        long id_lo, int B, int V, int d, int C, int K, const float* bias, long ld_bias,
                                        const int* group, int G, float* out_val, int* out_idx, void* ws, void* stream) {
    if (B <= 0) return 0;
    if (bad_shape(B, V, d, C, L, K) || (ld_sr & 3) || (ld_e & 3) || (comp_stride & 3) || ((uintptr_t)E & 15) ||
        ((uintptr_t)sr & 15) || out_val == nullptr || out_idx == nullptr || ws == nullptr || id_lo < 0 ||
        id_lo + (long)V > 0x7fffffffL || (listed_mode != 0 && listed_mode != 1) || G < 1 || (group == nullptr && G > 1) ||
        (bias != nullptr && G > 1 && ld_bias < (long)V) || ((uintptr_t)bias & 3) || ((uintptr_t)group & 3))
        return SREC_BAD_ARG;
    SelArgs a{};
    a.sr = sr; a.ld_sr = ld_sr; a.comp_stride = comp_stride; a.E = E; a.ld_e = ld_e; a.cs = cs;
    a.off_ex = off_ex; a.off_in = off_in; a.listed = L > 0 ? listed : nullptr; a.L = a.listed != nullptr ? L : 0;
    a.drop = listed_mode; a.id_lo = id_lo; a.B = B; a.V = V; a.d = d; a.K = K;
    a.bias = bias; a.ld_bias = ld_bias; a.group = group; a.G = G;
    const int R = pick_ranges(B, V);
    a.items_per_range = cdiv(cdiv(V, R), CHUNK) * CHUNK;
    const int Ract = cdiv(V, a.items_per_range);
    a.pv = (float*)ws;
    a.pi = (int*)(a.pv + (size_t)R * B * K);
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: return run<1>(a, Ract, out_val, out_idx, st);
        case 2: return run<2>(a, Ract, out_val, out_idx, st);
        case 3: return run<3>(a, Ract, out_val, out_idx, st);
        default: return run<4>(a, Ract, out_val, out_idx, st);
    }
}

extern "C" int srec_score_select(const float* sr, int ld_sr, long comp_stride, const float* E, int ld_e, const float* cs,
                                 const float* off_ex, const float* off_in, const int* listed, int L, int listed_mode,
                                 long id_lo, int B, int V, int d, int C, int K, float* out_val, int* out_idx, void* ws,
                                 void* stream) {
    return srec_score_select_biased(sr, ld_sr, comp_stride, E, ld_e, cs, off_ex, off_in, listed, L, listed_mode, id_lo, B, V, d,
                                    C, K, nullptr, 0, nullptr, 1, out_val, out_idx, ws, stream);
}
