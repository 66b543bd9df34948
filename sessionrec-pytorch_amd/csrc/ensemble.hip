// srec_ens_select / srec_ens_ahead: the catalogue pass of score_pass.h over SEVERAL tables - the served score of a
// probability-averaged ensemble of models (include/srec_ens.h: srec_served_multi; contract in include/srec.h), WITHOUT one (B, V) matrix per member.
//   s[b,v] = logsumexp_{c<C}( cs_c[v] * <sr_c[b], E_c[v]> + off[c,b] ) (+ bias[group[b], v]),  1 <= C <= 8: every component has
//   its own table, width and column scale; offsets, the listed set, the bias and ELIGIBILITY are those of score_pass.h.
// The pass keeps the workgroup of score_pass.h (32 sessions x one item range, 4 wavefronts, 128-item chunks) and its text
// blocks for the offsets, the listed set, the chunk mask and the eligibility rule.  What differs:
//   * C is a RUN-TIME loop: per chunk and component one score_tile::dots<1, SR_LDS> with that component's rows and width (the
//     raw dot product of component c is, to the bit, what the single-table pass over (sr_c, E_c) forms), folded into a running
//     (max, sum) pair per accumulator register - an online log-sum-exp, one exp per component and pair, one log at the end.
//     Registers do not grow with C, and there are SR_LDS x BIAS instances per kernel, not x 8.  C == 1 forms z + off alone.
//   * the per-component pointers travel in the by-value argument block (EnsComps) and are read with scalar loads.
//   * the session tiles of ALL components sit in LDS back to back ([32][tile_ld(d_c)] each) when they fit beside the kernel's own
//     arrays within 160 KB, else every component is read through the cache - same code, same sums.
//   * the membership bits of a lane's 16 sessions are taken into one register after the first component's tile product (the
//     barrier that publishes the mask stands there), because every component's offset depends on them.
// Selection: the running K best per session, the survivor merge and the pass-2 merge are those of recommend.hip, restated
// here (a copy: the existing instances stay the code they are); counting: the epilogue of rank_served.hip.  No floor, no
// noise, no bf16.
// LDS of the select pass: 2 KB of offsets (8 components) + 1.1 KB of masks and counts + 32 K (value, id) pairs + 17 KB of
// candidates + 32 L ids (+ 256 B of bias row offsets with G rows) + the tiles: K = 20, no list, four components of d = 256:
// 25.7 KB + 130 KB.  Of the count pass: 2 KB + 0.6 KB + 512 B of per-session scalars + 32 L ids (+ 256 B) + the tiles.
#include "common.h"
#include "score_pass.h"

namespace {

using namespace score_tile;

constexpr int ENSC = SREC_ENS_MAXCOMP;
constexpr int MAXK = SREC_SELECT_MAXK;
constexpr int CST = CHUNK + 8;      // candidate row stride (recommend.hip)
constexpr int EMPTY = 0x7fffffff;   // id of an unfilled list slot: behind every real item of the same value

struct EnsComps {
    const float* sr[ENSC]; const float* E[ENSC]; const float* cs[ENSC];
    int ld_sr[ENSC], ld_e[ENSC], d[ENSC];
    int C;
};
// the shared members live in the PassArgs base, under the names the text blocks of score_pass.h read (its sr / E / cs / d
// are component 0's and are not read by the kernels)
struct EnsArgs : PassArgs { EnsComps m; };

inline bool ens_bad_shape(int B, int V, int C, int L) {
    return B <= 0 || V <= 0 || C < 1 || C > ENSC || L < 0 || L > MAXL;
}
inline bool ens_bad_width(int d) { return d <= 0 || (d & 3) || d > 1024; }

// pass_args for the multi-table descriptor: the same refusals, per component where the member is per component
inline int ens_args(EnsArgs& a, const srec_served_multi& s, bool ids_fit_int) {
    if (ens_bad_shape(s.B, s.V, s.C, s.L) || s.id_lo < 0 || (ids_fit_int && s.id_lo + (long)s.V > 0x7fffffffL) ||
        (s.listed_mode != SREC_LISTED_SCORE && s.listed_mode != SREC_LISTED_DROP) || s.G < 1 || (s.group == nullptr && s.G > 1) ||
        (s.bias != nullptr && s.G > 1 && s.ld_bias < (long)s.V) || ((uintptr_t)s.bias & 3) || ((uintptr_t)s.group & 3))
        return SREC_BAD_ARG;
    for (int c = 0; c < s.C; ++c) {
        if (ens_bad_width(s.d[c]) || s.sr[c] == nullptr || s.E[c] == nullptr || (s.ld_sr[c] & 3) || (s.ld_e[c] & 3) ||
            s.ld_sr[c] < s.d[c] || s.ld_e[c] < s.d[c] || ((uintptr_t)s.sr[c] & 15) || ((uintptr_t)s.E[c] & 15) ||
            ((uintptr_t)s.cs[c] & 3))
            return SREC_BAD_ARG;
    }
    a.m = EnsComps{};
    for (int c = 0; c < s.C; ++c) {
        a.m.sr[c] = s.sr[c]; a.m.E[c] = s.E[c]; a.m.cs[c] = s.cs[c];
        a.m.ld_sr[c] = s.ld_sr[c]; a.m.ld_e[c] = s.ld_e[c]; a.m.d[c] = s.d[c];
    }
    a.m.C = s.C;
    a.sr = s.sr[0]; a.ld_sr = s.ld_sr[0]; a.comp_stride = 0; a.E = s.E[0]; a.ld_e = s.ld_e[0]; a.cs = s.cs[0];
    a.off_ex = s.off_ex; a.off_in = s.off_in; a.listed = s.L > 0 ? s.listed : nullptr; a.L = a.listed != nullptr ? s.L : 0;
    a.drop = s.listed_mode; a.id_lo = s.id_lo; a.B = s.B; a.V = s.V; a.d = s.d[0]; a.items_per_range = 0;
    a.bias = s.bias; a.ld_bias = s.ld_bias; a.group = s.group; a.G = s.G;
    return 0;
}

// the pass's own arrays (PassLds) sized for 8 components
inline size_t ens_pass_lds(int L, bool grouped) {
    return (size_t)(2 * ENSC * SB + SB * 4 + SB + SB * L + (grouped ? SB * 2 : 0)) * 4;
}
inline size_t ens_tile_bytes(const EnsComps& m) {
    size_t n = 0;
    for (int c = 0; c < m.C; ++c) n += (size_t)SB * tile_ld(m.d[c]) * 4;
    return n;
}

// this lane's item of the chunk: what all components share (SCORE_PASS_LANE_ITEM without the table row and the column scale)
template <int BIAS>
struct EnsItem {
    int v; bool vok;
    float bv;                     // BIAS == 1
    float bg[BIAS == 2 ? 16 : 1]; // BIAS == 2: the lane's 16 sessions (under way during the tile products)
};

}  // namespace

// declares `it` (the bias loads are issued here, ahead of the tile products)
#define ENS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)                                                            \
    EnsItem<BIAS> it;                                                                                                        \
    it.v = base + wave * 32 + l31;                                                                                           \
    it.vok = it.v < v1;                                                                                                      \
    it.bv = 0.f;                                                                                                             \
    if constexpr (BIAS == 1) it.bv = it.vok ? (a).bias[it.v] : 0.f;                                                          \
    if constexpr (BIAS == 2) {                                                                                               \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_)                                                                    \
            it.bg[r_] = (a).bias[(ps).goff[score_tile::session_of(r_, half)] + min(it.v, (a).V - 1)];                        \
    }

// inside `for (c < C)`: component c's operands of this lane - the item's table row (clamped: rows >= V are never eligible)
// and column scale, the session's A row (tile in LDS at float offset toff, or clamped through the cache) - then its raw dot
// products acc[0]; toff moves on to the next component's tile
#define ENS_COMP_DOTS(SR_LDS, c, it, a, Ss, toff, b0, l31, half, csv, acc)                                                   \
    const int dc_ = (a).m.d[c];                                                                                              \
    const float* brow_ = (a).m.E[c] + (size_t)min((it).v, (a).V - 1) * (a).m.ld_e[c] + 4 * half;                             \
    const float* csp_ = (a).m.cs[c];                                                                                         \
    const float csv = (csp_ != nullptr && (it).vok) ? csp_[(it).v] : 1.f;                                                    \
    const float* arow_[1];                                                                                                   \
    if (SR_LDS) arow_[0] = Ss + toff + (size_t)l31 * score_tile::tile_ld(dc_) + 4 * half;                                    \
    else arow_[0] = (a).m.sr[c] + (size_t)min(b0 + l31, (a).B - 1) * (a).m.ld_sr[c] + 4 * half;                              \
    toff += score_tile::SB * score_tile::tile_ld(dc_);                                                                       \
    f32x16 acc[1];                                                                                                           \
    score_tile::dots<1, SR_LDS>(arow_, brow_, dc_, half, acc);

// after the barrier that publishes the chunk's mask: bit r of inb = the lane's item is listed for session_of(r, half)
#define ENS_MEMBER_BITS(ps, inb, wave, l31, half)                                                                            \
    if ((ps).has_list) {                                                                                                     \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_)                                                                    \
            inb |= (((ps).inm[score_tile::session_of(r_, half) * 4 + wave] >> l31) & 1u) << r_;                              \
    }

// component c of the 16 pairs of this lane into the running (max, sum): z = cs * dot + off, exactly SCORE_PASS_ITEM_SCORE's
// term.  c == 0 starts the pair at (z, 1); later components: one exp each; z == -inf adds nothing
#define ENS_FOLD(c, csv, acc, ps, inb, half, mx, sm)                                                                         \
    _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                                      \
        const float* of_ = ((inb >> r_) & 1u) ? (ps).offi : (ps).offs;                                                       \
        const float z_ = csv * acc[0][r_] + of_[c * score_tile::SB + score_tile::session_of(r_, half)];                      \
        if (c == 0) {                                                                                                        \
            mx[r_] = z_;                                                                                                     \
            sm[r_] = 1.f;                                                                                                    \
        } else {                                                                                                             \
            const bool up_ = z_ > mx[r_];                                                                                    \
            const float e_ = expf(up_ ? mx[r_] - z_ : z_ - mx[r_]);                                                          \
            sm[r_] = up_ ? sm[r_] * e_ + 1.f : (z_ > -INFINITY ? sm[r_] + e_ : sm[r_]);                                      \
            mx[r_] = up_ ? z_ : mx[r_];                                                                                      \
        }                                                                                                                    \
    }

// inside `for (r < 16)` after the component loop: declares sl, in, s (the biased served score) and bias_ok
#define ENS_ITEM_SCORE(C, BIAS, it, mx, sm, r, inb, half, sl, in, s, bias_ok)                                                \
    const int sl = score_tile::session_of(r, half);                                                                          \
    const bool in = (inb >> r) & 1u;                                                                                         \
    float s = C == 1 ? mx[r] : mx[r] + logf(sm[r]);                                                                          \
    bool bias_ok = true;                                                                                                     \
    if constexpr (BIAS != 0) {                                                                                               \
        const float bb_ = BIAS == 1 ? (it).bv : (it).bg[BIAS == 2 ? r : 0];                                                  \
        s += bb_;                                                                                                            \
        bias_ok = bb_ != -INFINITY;                                                                                          \
    }

namespace {

// all 256 threads: the session tiles of every component, back to back
__device__ __forceinline__ void ens_stage_tiles(float* Ss, const EnsComps& m, int b0, int B, int tid) {
    int toff = 0;
    for (int c = 0; c < m.C; ++c) {
        stage_tiles<1>(Ss + toff, m.sr[c], m.ld_sr[c], 0, b0, B, m.d[c], tid);
        toff += SB * tile_ld(m.d[c]);
    }
}

// ---- selection ----------------------------------------------------------------------------------------------------------

struct EnsSelArgs : EnsArgs {
    int K;
    float* pv; int* pi;             // [R][B][K] per-range lists (local rows; EMPTY = unfilled)
};

__device__ __forceinline__ bool better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// one wavefront: merge the candidates whose bit is set in m[0..4) into the list lv / li [K], sorted by `better`
// (recommend.hip: merge_sorted, restated)
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

inline size_t ens_part_lds(const EnsComps& m, int K, int L, bool sr_lds, bool grouped) {
    return ens_pass_lds(L, grouped) + (size_t)SB * 4 * 4 + (size_t)SB * K * 8 + (size_t)SB * CST * 4 +
           (sr_lds ? ens_tile_bytes(m) : 0);
}

template <bool SR_LDS, int BIAS>
__global__ __launch_bounds__(256) void ens_select_part_kernel(EnsSelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K = a.K, L = a.L, C = a.m.C;
    float* offs = smem;                                             // the pass's arrays (PassLds) among this kernel's:
    float* offi = offs + ENSC * SB;
    unsigned* inm = reinterpret_cast<unsigned*>(offi + ENSC * SB);
    unsigned* surv = inm + SB * 4;                                  // [SB][4] survivors of this chunk
    int* nin = reinterpret_cast<int*>(surv + SB * 4);
    float* lv = reinterpret_cast<float*>(nin + SB);                 // [SB][K] running best values
    int* li = reinterpret_cast<int*>(lv + SB * K);                  // [SB][K] ... and local rows
    float* cand = reinterpret_cast<float*>(li + SB * K);            // [SB][CST] scores of this chunk's survivors
    int* lst = reinterpret_cast<int*>(cand + SB * CST);
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(lst + SB * L);
    float* Ss = reinterpret_cast<float*>(goff + (BIAS == 2 ? SB : 0));   // the tiles (SR_LDS); 16-byte aligned: all counts above are multiples of 4

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB, range = blockIdx.x;
    const int v0 = range * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const PassLds<true> ps{offs, offi, inm, nin, lst, goff, L > 0, a.drop != 0};

    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    for (int i = tid; i < SB * K; i += 256) { lv[i] = -INFINITY; li[i] = EMPTY; }
    SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)
    if (SR_LDS) ens_stage_tiles(Ss, a.m, b0, a.B, tid);
    __syncthreads();

    for (int base = v0; base < v1; base += CHUNK) {
        SCORE_PASS_CHUNK_MASK(ps, L, base, tid)
        ENS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)
        float mx[16], sm[16];
        unsigned inb = 0u;
        int toff = 0;
        for (int c = 0; c < C; ++c) {
            ENS_COMP_DOTS(SR_LDS, c, it, a, Ss, toff, b0, l31, half, csv, acc)
            if (c == 0) {
                __syncthreads();      // membership bits written; the merges of the previous chunk are done
                ENS_MEMBER_BITS(ps, inb, wave, l31, half)
            }
            ENS_FOLD(c, csv, acc, ps, inb, half, mx, sm)
        }

        // per-lane epilogue: item v (this lane's column) against 16 sessions
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ENS_ITEM_SCORE(C, BIAS, it, mx, sm, r, inb, half, sl, in, s, bias_ok)
            const bool hit = SCORE_PASS_ELIGIBLE(it, in, ps, b0 + sl < a.B, bias_ok) && better(s, it.v, lv[sl * K + K - 1], li[sl * K + K - 1]);
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

// one wavefront per session folds the per-range lists (recommend.hip: select_merge_kernel, restated)
__global__ __launch_bounds__(256) void ens_select_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int R,
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

// (the first parameter is launch_pass's component count: always 1 here, C is a run-time member)
template <int, bool SR_LDS, int BIAS>
struct EnsSelectPart { static constexpr auto kernel = ens_select_part_kernel<SR_LDS, BIAS>; };

inline int ens_ranges(int B, int V) { return pick_ranges(B, V, 512, 4); }      // as recommend.hip

// ---- counting -----------------------------------------------------------------------------------------------------------

struct EnsAheadArgs : EnsArgs {
    const int* labels;              // [B] global ids (< 0: -1)
    const float* target;            // [B] the labels' served values
    int* ahead;                     // [B], zeroed by the entry point
};

inline size_t ens_ahead_lds(const EnsComps& m, int L, bool sr_lds, bool grouped) {
    return ens_pass_lds(L, grouped) + (size_t)3 * SB * 4 + (sr_lds ? ens_tile_bytes(m) : 0);
}

template <bool SR_LDS, int BIAS>
__global__ __launch_bounds__(256) void ens_ahead_kernel(EnsAheadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = a.L, C = a.m.C;
    float* offs = smem;                                             // the pass's arrays (PassLds) among this kernel's:
    float* offi = offs + ENSC * SB;
    unsigned* inm = reinterpret_cast<unsigned*>(offi + ENSC * SB);
    int* nin = reinterpret_cast<int*>(inm + SB * 4);
    float* tgt = reinterpret_cast<float*>(nin + SB);                // [SB] the labels' values (+inf: a session that counts nothing)
    int* labs = reinterpret_cast<int*>(tgt + SB);                   // [SB] label - id_lo (clamped), or a value no row has
    int* cnt = labs + SB;                                           // [SB]
    int* lst = cnt + SB;
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(lst + SB * L);
    float* Ss = reinterpret_cast<float*>(goff + (BIAS == 2 ? SB : 0));  // the tiles (SR_LDS); 16-byte aligned: all counts above are multiples of 4

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB;
    const int v0 = blockIdx.x * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const PassLds<true> ps{offs, offi, inm, nin, lst, goff, L > 0, a.drop != 0};

    if (tid < SB) {
        const int b = b0 + tid;
        const bool ok = b < a.B && a.labels[b] >= 0;
        tgt[tid] = ok ? a.target[b] : INFINITY;          // nothing is ahead of +inf: dead sessions count nothing
        // label as a LOCAL row; labels owned by another shard keep their order relative to every local row
        long lv = ok ? (long)a.labels[b] - a.id_lo : -1;
        lv = lv < -1 ? -1 : (lv > (long)a.V ? (long)a.V : lv);
        labs[tid] = (int)lv;
        cnt[tid] = 0;
        if (blockIdx.x == 0 && b < a.B && !ok) a.ahead[b] = -1;     // no label (no workgroup adds to it: its count stays 0)
    }
    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)
    if (SR_LDS) ens_stage_tiles(Ss, a.m, b0, a.B, tid);
    __syncthreads();

    int clo[16], chi[16];                                // wave-uniform counts: session (r&3)+8(r>>2) and the one 4 above
#pragma unroll
    for (int r = 0; r < 16; ++r) { clo[r] = 0; chi[r] = 0; }

    for (int base = v0; base < v1; base += CHUNK) {
        if (ps.has_list) {
            __syncthreads();          // the previous chunk has read its membership bits
            SCORE_PASS_CHUNK_MASK(ps, L, base, tid)
        }
        ENS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)
        float mx[16], sm[16];
        unsigned inb = 0u;
        int toff = 0;
        for (int c = 0; c < C; ++c) {
            ENS_COMP_DOTS(SR_LDS, c, it, a, Ss, toff, b0, l31, half, csv, acc)
            if (c == 0 && ps.has_list) {
                __syncthreads();      // membership bits written
                ENS_MEMBER_BITS(ps, inb, wave, l31, half)
            }
            ENS_FOLD(c, csv, acc, ps, inb, half, mx, sm)
        }

#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ENS_ITEM_SCORE(C, BIAS, it, mx, sm, r, inb, half, sl, in, s, bias_ok)
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
    // (cnt != 0 only for a live session with a label: tgt = +inf elsewhere)
    if (tid < SB && b0 + tid < a.B && cnt[tid] != 0) atomicAdd(&a.ahead[b0 + tid], cnt[tid]);
}

template <int, bool SR_LDS, int BIAS>
struct EnsAhead { static constexpr auto kernel = ens_ahead_kernel<SR_LDS, BIAS>; };

}  // namespace

// ws: the per-range partial lists, (value, row) pairs
extern "C" int srec_ens_select_ws(int B, int V, int d_max, int C, int L, int K, long* bytes) {
    if (ens_bad_shape(B, V, C, L) || ens_bad_width(d_max) || K < 1 || K > MAXK || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = (long)ens_ranges(B, V) * B * K * 8;
    return 0;
}

extern "C" int srec_ens_select(const void* desc, int K, float* out_val, int* out_idx, void* ws, void* stream) {
    const srec_served_multi* s = (const srec_served_multi*)desc;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    EnsSelArgs a{};
    if (ens_args(a, *s, true) || K < 1 || K > MAXK || out_val == nullptr || out_idx == nullptr || ws == nullptr)
        return SREC_BAD_ARG;
    const int B = s->B, V = s->V;
    const int R = ens_ranges(B, V);
    const dim3 grid(split_ranges(a, R), cdiv(B, SB));
    a.K = K;
    a.pv = (float*)ws;
    a.pi = (int*)(a.pv + (size_t)R * B * K);
    hipStream_t st = (hipStream_t)stream;
    const auto lds = [&](int, bool sr_lds, bool grouped) { return ens_part_lds(a.m, K, a.L, sr_lds, grouped); };
    if (int rc = launch_pass<EnsSelectPart, true, 1>(a, grid, lds, st)) return rc;
    hipLaunchKernelGGL(ens_select_merge_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, a.pv, a.pi, (int)grid.x, B, K, s->id_lo,
                       out_val, out_idx);
    SREC_LAUNCH_CHECK();
    return 0;
}

// no scratch is needed (partial counts meet through integer atomics); a token size keeps the ABI uniform
extern "C" int srec_ens_ahead_ws(int B, int V, int d_max, int C, int L, long* bytes) {
    if (ens_bad_shape(B, V, C, L) || ens_bad_width(d_max) || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = 16;
    return 0;
}

extern "C" int srec_ens_ahead(const void* desc, const int* labels, const float* target, int* ahead, void* ws, void* stream) {
    (void)ws;
    const srec_served_multi* s = (const srec_served_multi*)desc;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    EnsAheadArgs a{};
    if (ens_args(a, *s, false) || labels == nullptr || target == nullptr || ahead == nullptr || ((uintptr_t)labels & 3) ||
        ((uintptr_t)target & 3) || ((uintptr_t)ahead & 3))
        return SREC_BAD_ARG;
    const int B = s->B, V = s->V;
    const dim3 grid(split_ranges(a, pick_ranges(B, V, 1024, 2)), cdiv(B, SB));     // as rank_served.hip
    a.labels = labels; a.target = target; a.ahead = ahead;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(ahead, 0, (size_t)B * 4, st); e != hipSuccess) return (int)e;
    const auto lds = [&](int, bool sr_lds, bool grouped) { return ens_ahead_lds(a.m, a.L, sr_lds, grouped); };
    if (int rc = launch_pass<EnsAhead, true, 1>(a, grid, lds, st)) return rc;
    SREC_LAUNCH_CHECK();
    return 0;
}
