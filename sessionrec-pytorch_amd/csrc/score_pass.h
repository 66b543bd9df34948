// One pass over the item table under THE SERVED SCORE, shared by rank.hip (count against a target), recommend.hip (select
// the K best) and score_norm.hip (log-mass); score_items.hip takes the argument block, the checks and switch_c.
//   s[b,v] = logsumexp_{c<C}( cs[v] * <sr_c[b], E_v> + off[c,b] ) (+ bias[group[b], v]),  off = off_in if v is in listed[b,:]
//   else off_ex   (C == 1: s = z + off, no exp / log); 1 <= C <= 4, d % 4 == 0, d <= 1024, L <= 64, cs / off_* / listed /
//   bias nullable.  A (session, row) pair is ELIGIBLE unless the row is >= V, the item is listed under SREC_LISTED_DROP
//   (off_in is then not read), or its bias is -INFINITY (not in the catalogue of this session - a condition of its own, not
//   a consequence of the score), or the session is >= B (left out where the caller writes its result, or in its test).
// The pass: workgroup = 32 sessions x one item range (pick_ranges), 4 wavefronts; per 128-item chunk the tile product of
//   score_tile.h leaves the C raw dot products of a (session, item) pair in one lane, which SCORE_PASS_ITEM_SCORE turns into
//   s; SCORE_PASS_ELIGIBLE is the eligibility rule.  Listed items are resolved INSIDE the pass: SCORE_PASS_PROLOGUE compacts
//   the ids of a session that fall into the workgroup's range to the front of its LDS row once; SCORE_PASS_CHUNK_MASK builds
//   a 128-bit membership mask per session and chunk from them (usually zero to two entries).  The caller owns the barriers around the mask - what it does with the scores decides
//   how many it needs - its LDS layout (PassLds points into it) and everything after s.
//   BIAS: 0 = none; 1 = one row for all sessions (the lane that owns item v loads bias[v] once per chunk beside its column
//   scale); 2 = G rows (the 32 sessions' row offsets are staged in LDS, 256 bytes; a lane loads its item's bias for its 16
//   sessions ahead of the tile product, every load coalesced over the 32 items of a half-wavefront).
#pragma once
#include <type_traits>
#include "score_tile.h"
#include "../../include/srec.h"

namespace score_tile {

struct PassArgs {
    const float* sr; int ld_sr; long comp_stride;
    const float* E; int ld_e;
    const float* cs;
    const float* off_ex; const float* off_in;
    const int* listed; int L; int drop;
    long id_lo;
    int B, V, d;
    int items_per_range;
    const float* bias; long ld_bias;
    const int* group; int G;
};

inline bool bad_shape(int B, int V, int d, int C, int L) {
    return B <= 0 || V <= 0 || d <= 0 || (d & 3) || d > 1024 || C < 1 || C > MAXCOMP || L < 0 || L > MAXL;
}

// The checks every entry point makes on its descriptor (include/srec.h: srec_served, a HOST struct), then the argument block
// (items_per_range: split_ranges).  An entry point has refused a NULL descriptor and returned 0 for B <= 0 before it comes
// here.  ids_fit_int: refuse a shard whose last global id does not fit an int (every entry point but srec_score_rank, which
// never forms such an id).
inline int pass_args(PassArgs& a, const srec_served& s, bool ids_fit_int) {
    if (bad_shape(s.B, s.V, s.d, s.C, s.L) || (s.ld_sr & 3) || (s.ld_e & 3) || (s.comp_stride & 3) || ((uintptr_t)s.E & 15) ||
        ((uintptr_t)s.sr & 15) || s.id_lo < 0 || (ids_fit_int && s.id_lo + (long)s.V > 0x7fffffffL) ||
        (s.listed_mode != SREC_LISTED_SCORE && s.listed_mode != SREC_LISTED_DROP) || s.G < 1 || (s.group == nullptr && s.G > 1) ||
        (s.bias != nullptr && s.G > 1 && s.ld_bias < (long)s.V) || ((uintptr_t)s.bias & 3) || ((uintptr_t)s.group & 3))
        return SREC_BAD_ARG;
    a.sr = s.sr; a.ld_sr = s.ld_sr; a.comp_stride = s.comp_stride; a.E = s.E; a.ld_e = s.ld_e; a.cs = s.cs;
    a.off_ex = s.off_ex; a.off_in = s.off_in; a.listed = s.L > 0 ? s.listed : nullptr; a.L = a.listed != nullptr ? s.L : 0;
    a.drop = s.listed_mode; a.id_lo = s.id_lo; a.B = s.B; a.V = s.V; a.d = s.d; a.items_per_range = 0;
    a.bias = s.bias; a.ld_bias = s.ld_bias; a.group = s.group; a.G = s.G;
    return 0;
}

// item ranges of a launch: about wg_target workgroups in all, at least min_chunks chunks per range
inline int pick_ranges(int B, int V, int wg_target, int min_chunks) {
    int R = cdiv(wg_target, cdiv(B, SB));
    const int maxR = cdiv(V, min_chunks * CHUNK);
    if (R > maxR) R = maxR;
    return R < 1 ? 1 : R;
}
// whole chunks per range; returns the number of ranges that hold a row (<= R, grid.x)
inline int split_ranges(PassArgs& a, int R) {
    a.items_per_range = cdiv(cdiv(a.V, R), CHUNK) * CHUNK;
    return cdiv(a.V, a.items_per_range);
}

template <class F>
int switch_c(int C, F f) {
    switch (C) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

// Kern<C, SR_LDS, BIAS>::kernel takes Args by value; lds(C, sr_lds, grouped) is its dynamic LDS size.  The session tiles go
// to LDS when the whole of it stays within LDS_BYTES, else they are read through the cache.
template <template <int, bool, int> class Kern, int C, bool SR_LDS, int BIAS, class Args>
int launch_one(const Args& a, dim3 grid, size_t lds, hipStream_t st) {
    static std::atomic<unsigned long long> optin{0};
    if (int rc = srec_lds_optin((const void*)Kern<C, SR_LDS, BIAS>::kernel, LDS_BYTES, optin)) return rc;
    hipLaunchKernelGGL((Kern<C, SR_LDS, BIAS>::kernel), grid, dim3(256), lds, st, a);
    return 0;
}
template <template <int, bool, int> class Kern, int C, int BIAS, class Args, class Lds>
int launch_placed(const Args& a, dim3 grid, Lds lds, hipStream_t st) {
    return lds(C, true, BIAS == 2) <= (size_t)LDS_BYTES ? launch_one<Kern, C, true, BIAS>(a, grid, lds(C, true, BIAS == 2), st)
                                                        : launch_one<Kern, C, false, BIAS>(a, grid, lds(C, false, BIAS == 2), st);
}
// BIASED = false: the kernel has BIAS = 0 instances only
template <template <int, bool, int> class Kern, bool BIASED, int C, class Args, class Lds>
int launch_pass(const Args& a, dim3 grid, Lds lds, hipStream_t st) {
    if constexpr (BIASED) {
        if (a.bias != nullptr) return a.G == 1 ? launch_placed<Kern, C, 1>(a, grid, lds, st) : launch_placed<Kern, C, 2>(a, grid, lds, st);
    }
    return launch_placed<Kern, C, 0>(a, grid, lds, st);
}

// where the caller keeps the shared state of the pass in ITS dynamic LDS.  LISTS = false compiles the listed set out (every
// item scores with off_ex; only offs is used)
template <bool LISTS>
struct PassLds {
    float* offs;                // [MAXCOMP][SB] off_ex
    float* offi;                // [MAXCOMP][SB] off_in (SCORE mode)
    unsigned* inm;              // [SB][4] listed items of this chunk
    int* nin;                   // [SB] listed ids inside this workgroup's range
    int* lst;                   // [SB][L] listed ids as local rows, in-range ones first
    unsigned long long* goff;   // [SB] bias row offsets (BIAS == 2 only)
    bool has_list, drop;        // L > 0; SREC_LISTED_DROP
    static constexpr bool lists = LISTS;
};
inline size_t pass_lds(int L, bool grouped) {
    return (size_t)(2 * MAXCOMP * SB + SB * 4 + SB + SB * L + (grouped ? SB * 2 : 0)) * 4;
}

// this lane's item of the chunk (filled by SCORE_PASS_LANE_ITEM)
template <int BIAS>
struct LaneItem {
    int v; bool vok;
    const float* brow;            // its table row + 4 * half (clamped: rows >= V are never eligible)
    float csv;
    float bv;                     // BIAS == 1: this item, all sessions
    float bg[BIAS == 2 ? 16 : 1]; // BIAS == 2: this item, the lane's 16 sessions (under way during the tile product)
};

}  // namespace score_tile

// The device blocks of the pass are TEXT, not functions.  A __forceinline__ callee is simplified on its own before it is
// inlined, and the kernels that came out were not the ones the in-line code gives: norm_part_kernel<1, true, 1> lost its
// fourth wave per SIMD (114 + 16 registers for 112 + 16) with the offsets staged by a function, select_part_kernel's
// threshold test grew by 16 scalar mask operations per chunk with the score in one, and rows of the timing tools moved by
// 1 - 2 %.  As text the blocks compile to what the in-line code compiled to (profiles/score_pass_refactor.md).  Each macro
// names every variable of the kernel it reads or declares; ps is the kernel's PassLds, a its argument block.
//
// all 256 threads, first thing in the kernel: off_ex / off_in of the workgroup's 32 sessions -> ps.offs / ps.offi
#define SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)                                                                          \
    for (int i_ = tid; i_ < C * score_tile::SB; i_ += 256) {                                                                 \
        const int c_ = i_ / score_tile::SB, b_ = b0 + i_ % score_tile::SB;                                                   \
        (ps).offs[i_] = ((a).off_ex != nullptr && b_ < (a).B) ? (a).off_ex[(size_t)c_ * (a).B + b_] : 0.f;                   \
        if constexpr (decltype(ps)::lists)                                                                                   \
            (ps).offi[i_] = ((a).off_in != nullptr && b_ < (a).B && !(ps).drop) ? (a).off_in[(size_t)c_ * (a).B + b_] : 0.f; \
    }

// all 256 threads, ahead of the barrier that follows stage_tiles: the mask zeroed, the bias row offsets (sessions past the
// batch read row 0; a group id outside [0, G) is the caller's error and is held inside the operand), and the session's
// listed ids inside [v0, v1) compacted to the front of its row in list order (ballot prefix)
#define SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)                                                        \
    if constexpr (decltype(ps)::lists) {                                                                                     \
        if (tid < score_tile::SB * 4) (ps).inm[tid] = 0u;                                                                    \
    }                                                                                                                        \
    if constexpr (BIAS == 2) {                                                                                               \
        if (tid < score_tile::SB)                                                                                            \
            (ps).goff[tid] =                                                                                                 \
                b0 + tid < (a).B ? (unsigned long long)min(max((a).group[b0 + tid], 0), (a).G - 1) * (a).ld_bias : 0ull;     \
    }                                                                                                                        \
    if (decltype(ps)::lists && (ps).has_list) {                                                                              \
        for (int j_ = wave; j_ < score_tile::SB; j_ += 4) {                                                                  \
            const int b_ = b0 + j_;                                                                                          \
            bool ok_ = false;                                                                                                \
            int loc_ = 0;                                                                                                    \
            if (lane < (a).L && b_ < (a).B) {                                                                                \
                const long u_ = (a).listed[(size_t)b_ * (a).L + lane];                                                       \
                const long lr_ = u_ - (a).id_lo;                                                                             \
                ok_ = u_ >= 0 && lr_ >= (long)v0 && lr_ < (long)v1;                                                          \
                loc_ = (int)lr_;                                                                                             \
            }                                                                                                                \
            const unsigned long long mk = __ballot(ok_);                                                                    \
            if (ok_) (ps).lst[j_ * (a).L + __popcll(mk & ((1ull << lane) - 1ull))] = loc_;                                  \
            if (lane == 0) (ps).nin[j_] = __popcll(mk);                                                                     \
        }                                                                                                                    \
    }

// thread (session, 32-item word) of the first 128: membership bits of the chunk at `base` (the caller owns the barriers)
#define SCORE_PASS_CHUNK_MASK(ps, L, base, tid)                                                                              \
    if ((ps).has_list && tid < score_tile::SB * 4) {                                                                         \
        const int j_ = tid >> 2, w_ = tid & 3, n_ = (ps).nin[j_];                                                            \
        unsigned bits_ = 0u;                                                                                                 \
        for (int i_ = 0; i_ < n_; ++i_) {                                                                                    \
            const int o_ = (ps).lst[j_ * L + i_] - base - 32 * w_;                                                           \
            if (o_ >= 0 && o_ < 32) bits_ |= 1u << o_;                                                                       \
        }                                                                                                                    \
        (ps).inm[tid] = bits_;                                                                                               \
    }

// declares `it`, this lane's item of the chunk at `base`; its loads are issued here, ahead of dots()
#define SCORE_PASS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)                                                     \
    score_tile::LaneItem<BIAS> it;                                                                                           \
    it.v = base + wave * 32 + l31;                                                                                           \
    it.vok = it.v < v1;                                                                                                      \
    it.brow = (a).E + (size_t)min(it.v, (a).V - 1) * (a).ld_e + 4 * half;                                                    \
    it.csv = ((a).cs != nullptr && it.vok) ? (a).cs[it.v] : 1.f;                                                             \
    it.bv = 0.f;                                                                                                             \
    if constexpr (BIAS == 1) it.bv = it.vok ? (a).bias[it.v] : 0.f;                                                          \
    if constexpr (BIAS == 2) {                                                                                               \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_)                                                                    \
            it.bg[r_] = (a).bias[(ps).goff[score_tile::session_of(r_, half)] + min(it.v, (a).V - 1)];                        \
    }

// inside `for (r < 16)`: declares sl = session_of(r, half), in (the lane's item `it` is listed for that session), s (the
// served score of the pair from accumulator register r) and bias_ok (its bias leaves the item in that session's catalogue)
#define SCORE_PASS_ITEM_SCORE(C, BIAS, it, acc, r, ps, wave, l31, half, sl, in, s, bias_ok)                                  \
    const int sl = score_tile::session_of(r, half);                                                                          \
    const bool in = decltype(ps)::lists && (ps).has_list && (((ps).inm[sl * 4 + wave] >> l31) & 1u);                         \
    const float* of_ = in ? (ps).offi : (ps).offs;                                                                           \
    float z_[C];                                                                                                             \
    _Pragma("unroll") for (int c_ = 0; c_ < C; ++c_) z_[c_] = (it).csv * acc[c_][r] + of_[c_ * score_tile::SB + sl];         \
    float s = score_tile::mix<C>(z_);                                                                                        \
    bool bias_ok = true;                                                                                                     \
    if constexpr (BIAS != 0) {                                                                                               \
        const float bb_ = BIAS == 1 ? (it).bv : (it).bg[BIAS == 2 ? r : 0];                                                  \
        s += bb_;                                                                                                            \
        bias_ok = bb_ != -INFINITY;                                                                                          \
    }

// THE eligibility rule, an expression for the caller's own condition (live: what it knows about session < B at that point)
#define SCORE_PASS_ELIGIBLE(it, in, ps, live, bias_ok) ((it).vok && (live) && !((in) && (ps).drop) && (bias_ok))
