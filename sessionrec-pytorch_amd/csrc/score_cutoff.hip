// srec_score_cutoff*: the per-session score CUTOFF of truncated sampling (top-k of any size / top-p / min-p; include/srec.h has
// the contract) over the served score of score_pass.h, WITHOUT the (B, V) score matrix: floor[b], the number of eligible rows
// at or above it, and the log of the probability mass they hold at the draw's temperature.
//
// The score s' + 0.0f maps to an order-preserving 32-bit key; the key of the k-th largest score (top_k) and of the nucleus
// boundary (top_p) are found by radix search, 8 bits per pass of the catalogue.
// Histogram pass (cutoff_hist_kernel, pass 0 .. 3): the pass of score_pass.h.  Every workgroup keeps, per session, 256 bins
//   over digit `pass` of the key in LDS - COUNTS (u32) for the top_k search, MASS (u64) for the top_p search - and an eligible
//   pair whose higher digits equal the session's prefix of that search adds to its bin with an LDS integer atomic.  Mass is
//   FIXED-POINT: x = (u64)(min(expf((s' - m) / T), 1) * 2^44), so every sum is an integer sum - order-free: the result does
//   not depend on the item-range split, and row shards add exactly.  A workgroup covers at most 2^19 items (ranges()), so a
//   bin stays below 2^63.  At the end the workgroup adds its NON-EMPTY bins to hist [B][3][256] (counts, mass mod 2^32, mass
//   >> 32: two int64 limbs, since the sum over 2^24 items of weight 1 needs 68 bits) with global integer atomics.
// Advance (cutoff_advance_kernel): one workgroup per session, one thread per bin, sums the 3 x 256 bins from the top down on
//   top of the carried (count above, mass above), fixes the next digit of either search and writes the new state; after pass 3 the
//   keys are known to the bit and the floor is written.  "mass >= p W" is the integer test mass * 2^32 >= P * W with
//   P = round(p * 2^32) in [1, 2^32 - 1], in 128-bit arithmetic.  No host synchronisation between the passes.
// Tail (the TAIL instances of the histogram kernel, pass = 4): two bins per session, below / at-or-above the floor - the kept
//   count, the kept mass and the mass below (their sum is W) for the final floor, whatever criteria produced it.  Every pair
//   lands in one of the two bins, so a lane sums its 16 sessions in registers and the workgroup folds them once.  cutoff_finish_kernel: count and log_kept from the summed bins.
// No float atomics anywhere: the outputs are a pure function of the inputs.
// LDS (cut_lds): the pass's 1.6 KB of offsets, mask and counts, 32 L ids (and 256 bytes of bias row offsets with G rows) + 384
// bytes of per-session maxima and prefixes + 32 KB of count bins (top_k) + 64 KB of mass bins (top_p) + the session tiles when
// the sum stays within 160 KB (both searches, d = 256: C = 1 130.5 KB without a list, 138.8 KB with L = 64 and G rows; C = 3
// would be 195.5 KB), else the tiles are
// read through the cache.  The tail keeps 2 bins per session: 768 bytes.
#include "common.h"
#include "score_key.h"
#include "score_pass.h"

namespace {

using namespace score_tile;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int NPASS = 4;            // SREC_CUTOFF_PASSES: 8 bits of the key per pass
constexpr int NSTATE = 8;           // SREC_CUTOFF_STATE
constexpr int NBIN = 256;
constexpr int MASS_SHIFT = 44;      // fixed-point weights: quantum 2^-44
constexpr int WG_ITEMS = 1 << 19;   // items of one workgroup at most: a u64 bin holds 2^19 weights of 2^44
enum { ST_PREFK, ST_PREFP, ST_CABOVE, ST_MABOVE_LO, ST_MABOVE_HI, ST_W_LO, ST_W_HI, ST_FLAGS };
enum { FEWER_THAN_K = 1, NO_MASS = 2 };

struct CutArgs : PassArgs {
    float inv_t;
    int do_k, do_p;                 // the searches that take part (tail: both - count and mass)
    int pass;                       // 0 .. 3: the digit; NPASS: the tail
    const float* top;               // [B] m_b
    const long long* state;         // [B][NSTATE] (pass 1 .. 3)
    const float* floor;             // [B] (tail)
    u64* hist;                      // [B][3][NBIN]
};

// key_of / score_of: score_key.h (s + 0.0f as a key whose unsigned order is the order of the floats)
// the fixed-point weight of a score under the session's maximum m (m == -inf: every weight is 0, never exp(nan))
__device__ __forceinline__ u64 weight_of(float s, float m, float inv_t) {
    if (m == -INFINITY) return 0ull;
    return (u64)(fminf(expf((s - m) * inv_t), 1.f) * 0x1p44f);
}
static_assert(MASS_SHIFT == 44, "weight_of scales by 0x1p44f");

inline size_t cut_lds(int C, int d, int L, bool sr_lds, bool grouped, int nbin, bool do_k, bool do_p) {
    return pass_lds(L, grouped) + (size_t)3 * SB * 4 + (do_p ? (size_t)SB * nbin * 8 : 0) + (do_k ? (size_t)SB * nbin * 4 : 0) +
           (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS, int BIAS, bool TAIL>
__global__ __launch_bounds__(256) void cutoff_hist_kernel(CutArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d, L = a.L;
    constexpr bool tail = TAIL;
    constexpr int nbin = TAIL ? 2 : NBIN;
    float* offs = smem;                                             // the pass's arrays (PassLds) among this kernel's:
    float* offi = offs + MAXCOMP * SB;
    unsigned* inm = reinterpret_cast<unsigned*>(offi + MAXCOMP * SB);
    int* nin = reinterpret_cast<int*>(inm + SB * 4);
    float* topm = reinterpret_cast<float*>(nin + SB);               // [SB] m_b
    unsigned* prefk = reinterpret_cast<unsigned*>(topm + SB);       // [SB] prefix of the top_k search (tail: the floor's key)
    unsigned* prefp = prefk + SB;                                   // [SB] prefix of the top_p search
    int* lst = reinterpret_cast<int*>(prefp + SB);
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(lst + SB * L);
    u64* mass = reinterpret_cast<u64*>(goff + (BIAS == 2 ? SB : 0));    // [SB][nbin] (do_p); 8-byte aligned: all counts above are multiples of 4
    unsigned* cnt = reinterpret_cast<unsigned*>(mass + (a.do_p ? SB * nbin : 0));   // [SB][nbin] (do_k)
    float* Ss = reinterpret_cast<float*>(cnt + (a.do_k ? SB * nbin : 0));           // [C][SB][LD] (SR_LDS); 16-byte aligned

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB, range = blockIdx.x;
    const int v0 = range * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const PassLds<true> ps{offs, offi, inm, nin, lst, goff, L > 0, a.drop != 0};

    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    if (tid < SB) {
        const int b = b0 + tid;
        const bool live = b < a.B;
        topm[tid] = live ? a.top[b] + 0.f : -INFINITY;
        unsigned pk = 0u, pp = 0u;
        if (tail) {
            pk = key_of(live ? a.floor[b] : -INFINITY);
        } else if (a.pass > 0 && live) {
            pk = (unsigned)a.state[(size_t)b * NSTATE + ST_PREFK];
            pp = (unsigned)a.state[(size_t)b * NSTATE + ST_PREFP];
        }
        prefk[tid] = pk; prefp[tid] = pp;
    }
    if (a.do_p) for (int i = tid; i < SB * nbin; i += 256) mass[i] = 0ull;
    if (a.do_k) for (int i = tid; i < SB * nbin; i += 256) cnt[i] = 0u;
    SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);

    // pass j looks at digit j from the top; the digits above it must equal the search's prefix
    const int shift = tail ? 0 : 24 - 8 * a.pass;
    const unsigned himask = (tail || a.pass == 0) ? 0u : 0xffffffffu << (32 - 8 * a.pass);
    const float inv_t = a.inv_t;
    // TAIL: two bins per session and every pair lands in one of them - LDS atomics would meet 32 to an address, so a lane
    // keeps its 16 sessions' sums in registers across the chunks and the workgroup adds them up once
    [[maybe_unused]] unsigned tn[TAIL ? 16 : 1];
    [[maybe_unused]] u64 tkept[TAIL ? 16 : 1], tbelow[TAIL ? 16 : 1];
    if constexpr (TAIL) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { tn[r] = 0u; tkept[r] = 0ull; tbelow[r] = 0ull; }
    }

    for (int base = v0; base < v1; base += CHUNK) {
        if (ps.has_list) {
            __syncthreads();          // the epilogue of the previous chunk has read its membership bits
            SCORE_PASS_CHUNK_MASK(ps, L, base, tid)
        }
        SCORE_PASS_LANE_ITEM(BIAS, it, a, ps, base, v1, wave, l31, half)
        f32x16 acc[C];
        dots<C, SR_LDS>(arow, it.brow, d, half, acc);
        if (ps.has_list) __syncthreads(); // membership bits written

        // per-lane epilogue: item v (this lane's column) against 16 sessions
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            SCORE_PASS_ITEM_SCORE(C, BIAS, it, acc, r, ps, wave, l31, half, sl, in, s, bias_ok)
            if (SCORE_PASS_ELIGIBLE(it, in, ps, b0 + sl < a.B, bias_ok)) {
                const unsigned key = key_of(s);
                if constexpr (TAIL) {
                    const bool ge = key >= prefk[sl];
                    const u64 x = weight_of(s, topm[sl], inv_t);
                    tn[r] += ge ? 1u : 0u;
                    tkept[r] += ge ? x : 0ull;
                    tbelow[r] += ge ? 0ull : x;
                } else {
                    const int bin = sl * NBIN + (int)((key >> shift) & 255u);
                    if (a.do_k && ((key ^ prefk[sl]) & himask) == 0u) atomicAdd(&cnt[bin], 1u);
                    if (a.do_p && ((key ^ prefp[sl]) & himask) == 0u) {
                        const u64 x = weight_of(s, topm[sl], inv_t);
                        if (x != 0ull) atomicAdd(&mass[bin], x);
                    }
                }
            }
        }
    }
    if constexpr (TAIL) {
        // the 32 item lanes of a half-wavefront -> one sum per session (integers: any order), then 4 wavefronts through LDS
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            unsigned n = tn[r];
            u64 k = tkept[r], w = tbelow[r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                n += __shfl_xor(n, o, 64);
                k += __shfl_xor(k, o, 64);
                w += __shfl_xor(w, o, 64);
            }
            if (l31 == 0) {
                const int sl = session_of(r, half);
                if (n != 0u) atomicAdd(&cnt[sl * 2 + 1], n);
                if (k != 0ull) atomicAdd(&mass[sl * 2 + 1], k);
                if (w != 0ull) atomicAdd(&mass[sl * 2], w);
            }
        }
    }
    __syncthreads();
    // the workgroup's non-empty bins -> hist (integer atomics: the sum does not depend on who arrives first)
    for (int i = tid; i < SB * nbin; i += 256) {
        const int j = i / nbin, dg = i % nbin, b = b0 + j;
        if (b >= a.B) continue;
        u64* h = a.hist + (size_t)b * 3 * NBIN + dg;
        if (a.do_k && cnt[i] != 0u) atomicAdd(h, (u64)cnt[i]);
        if (a.do_p && mass[i] != 0ull) {
            const u64 x = mass[i];
            if ((x & 0xffffffffull) != 0ull) atomicAdd(h + NBIN, x & 0xffffffffull);
            if ((x >> 32) != 0ull) atomicAdd(h + 2 * NBIN, x >> 32);
        }
    }
}

__device__ __forceinline__ u128 limbs(u64 lo, u64 hi) { return ((u128)hi << 32) + (u128)lo; }

// one workgroup per session, one thread per bin.  pass 0 .. 3: inclusive sums from the top bin down (8 doubling steps in LDS),
// then the digit of either search is the LARGEST bin whose sum from the top reaches the target (the sums grow downwards, and
// the bin above it falls short, so that bin is not empty); pass >= 3: write the floor
__global__ __launch_bounds__(256) void cutoff_advance_kernel(int pass, int do_k, int do_p, long long top_k, u64 P, float gap,
                                                             const long long* __restrict__ hist, long long* __restrict__ state,
                                                             float* __restrict__ top, float* __restrict__ floor_out) {
    __shared__ long long sc[2][NBIN];
    __shared__ u128 sm[2][NBIN];
    __shared__ int digit[2];
    const int b = blockIdx.x, t = threadIdx.x;
    const bool scan = pass < NPASS;
    long long* st = state + (size_t)b * NSTATE;
    unsigned prefk = 0u, prefp = 0u;
    long long flags = 0, cabove = 0;
    u128 mabove = 0, W = 0;
    if (scan) {
        const long long* h = hist + (size_t)b * 3 * NBIN;
        const long long c = h[t];
        const u128 v = limbs((u64)h[NBIN + t], (u64)h[2 * NBIN + t]);
        if (pass > 0) {
            prefk = (unsigned)st[ST_PREFK]; prefp = (unsigned)st[ST_PREFP]; cabove = st[ST_CABOVE];
            mabove = limbs((u64)st[ST_MABOVE_LO], (u64)st[ST_MABOVE_HI]);
            W = limbs((u64)st[ST_W_LO], (u64)st[ST_W_HI]);
            flags = st[ST_FLAGS];
        }
        if (t < 2) digit[t] = -1;
        sc[0][t] = c; sm[0][t] = v;
        __syncthreads();                    // (every thread has read the state: thread 0 rewrites it below)
        int cur = 0;
        for (int o = 1; o < NBIN; o <<= 1) {        // sum over the bins >= t
            sc[cur ^ 1][t] = sc[cur][t] + (t + o < NBIN ? sc[cur][t + o] : 0);
            sm[cur ^ 1][t] = sm[cur][t] + (t + o < NBIN ? sm[cur][t + o] : (u128)0);
            cur ^= 1;
            __syncthreads();
        }
        const long long cge = sc[cur][t];
        const u128 mge = sm[cur][t];
        if (pass == 0) W = sm[cur][0];              // the pass-0 total is W
        const bool live_k = do_k && !(flags & FEWER_THAN_K);
        const bool live_p = do_p && !(flags & NO_MASS) && W != 0;
        // mass * 2^32 >= P * W  <=>  mass / W >= P / 2^32; both sides below 2^101
        if (live_k && cabove + cge >= top_k) atomicMax(&digit[0], t);
        if (live_p && ((mabove + mge) << 32) >= (u128)P * W) atomicMax(&digit[1], t);
        __syncthreads();
        const int dk = digit[0], dp = digit[1];
        if (dk == t) sc[cur ^ 1][0] = cabove + cge - c;         // what lies strictly above the chosen bin
        if (dp == t) sm[cur ^ 1][0] = mabove + mge - v;
        __syncthreads();
        if (t != 0) return;
        const int shift = 24 - 8 * pass;
        if (do_k && !(flags & FEWER_THAN_K)) {
            if (dk >= 0) { prefk |= (unsigned)dk << shift; cabove = sc[cur ^ 1][0]; }
            else flags |= FEWER_THAN_K;             // (pass 0 only: afterwards the chosen bin holds the k-th)
        }
        if (do_p && !(flags & NO_MASS)) {
            if (W == 0) flags |= NO_MASS;
            else if (dp >= 0) { prefp |= (unsigned)dp << shift; mabove = sm[cur ^ 1][0]; }
        }
        st[ST_PREFK] = (long long)prefk; st[ST_PREFP] = (long long)prefp; st[ST_CABOVE] = cabove;
        st[ST_MABOVE_LO] = (long long)(u64)(mabove & 0xffffffffull); st[ST_MABOVE_HI] = (long long)(u64)(mabove >> 32);
        st[ST_W_LO] = (long long)(u64)(W & 0xffffffffull); st[ST_W_HI] = (long long)(u64)(W >> 32);
        st[ST_FLAGS] = flags;
    }
    if (t != 0) return;
    if (pass >= NPASS - 1) {
        const float m = top[b] + 0.f;
        top[b] = m;
        float f = -INFINITY;
        if (scan && do_k && !(flags & FEWER_THAN_K)) f = fmaxf(f, score_of(prefk));
        if (scan && do_p && !(flags & NO_MASS)) f = fmaxf(f, score_of(prefp));
        if (gap != INFINITY && m != -INFINITY) f = fmaxf(f, m - gap);
        floor_out[b] = f + 0.f;
    }
}

// the summed tail bins (0: below the floor, 1: kept) -> count, log(kept mass / W)
__global__ __launch_bounds__(256) void cutoff_finish_kernel(int B, const long long* __restrict__ hist, int* __restrict__ count,
                                                            float* __restrict__ log_kept) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const long long* h = hist + (size_t)b * 3 * NBIN;
    const long long n = h[1];
    const u128 kept = limbs((u64)h[NBIN + 1], (u64)h[2 * NBIN + 1]);
    const u128 W = kept + limbs((u64)h[NBIN], (u64)h[2 * NBIN]);
    count[b] = (int)n;
    float lk;
    if (n == 0) lk = -INFINITY;                         // nothing eligible
    else if (W == 0) lk = 0.f;                          // every eligible row scores -inf: floor = -inf keeps them all
    else if (kept == 0) lk = -INFINITY;                 // (cannot happen: the floor never exceeds the maximum, whose weight is 2^44)
    else {
        // normalised limbs convert exactly (lo < 2^32, hi < 2^37); one rounding in the sum
        const double k = (double)(u64)(kept >> 32) * 4294967296.0 + (double)(u64)(kept & 0xffffffffull);
        const double w = (double)(u64)(W >> 32) * 4294967296.0 + (double)(u64)(W & 0xffffffffull);
        lk = fminf((float)log(k / w), 0.f);
    }
    log_kept[b] = lk;
}

template <int C, bool SR_LDS, int BIAS>
struct CutHist { static constexpr auto kernel = cutoff_hist_kernel<C, SR_LDS, BIAS, false>; };
template <int C, bool SR_LDS, int BIAS>
struct CutTail { static constexpr auto kernel = cutoff_hist_kernel<C, SR_LDS, BIAS, true>; };

// the histogram passes hold 32 - 96 KB of bins: one or two workgroups per CU; the tail is as light as the norm pass
inline int ranges(int B, int V, bool tail) {
    const int R = pick_ranges(B, V, tail ? 1024 : 512, 2);
    const int need = cdiv(V, WG_ITEMS);
    return R < need ? need : R;
}

inline bool bad_inv_t(float inv_t) { return !(inv_t > 0.f) || !(inv_t <= 3.402823466e+38f); }
inline bool bad_criteria(int top_k, float top_p, float gap) { return top_k < 0 || !(top_p > 0.f) || !(gap >= 0.f); }
inline bool has_p(float top_p) { return top_p < 1.f; }

// s: not NULL
int hist_launch(const srec_served& s, float inv_t, bool do_k, bool do_p, int pass, const float* top, const long long* state,
                const float* floor, long long* hist, void* stream) {
    if (s.B <= 0) return 0;
    CutArgs a{};
    const bool tail = pass == NPASS;
    const int B = s.B, V = s.V, d = s.d, C = s.C;
    if (pass_args(a, s, true) || bad_inv_t(inv_t) || pass < 0 || pass > NPASS || top == nullptr || hist == nullptr || (tail && floor == nullptr) ||
        (!tail && pass > 0 && state == nullptr) || (!do_k && !do_p) || ((uintptr_t)top & 3) || ((uintptr_t)floor & 3) ||
        ((uintptr_t)state & 7) || ((uintptr_t)hist & 7))
        return SREC_BAD_ARG;
    const dim3 grid(split_ranges(a, ranges(B, V, tail)), cdiv(B, SB));
    a.inv_t = inv_t; a.do_k = do_k; a.do_p = do_p; a.pass = pass;
    a.top = top; a.state = state; a.floor = floor; a.hist = (u64*)hist;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * 3 * NBIN * 8, st); e != hipSuccess) return (int)e;
    const int nbin = tail ? 2 : NBIN;
    const auto lds = [&](int c, bool sr_lds, bool grouped) { return cut_lds(c, d, a.L, sr_lds, grouped, nbin, do_k, do_p); };
    if (int rc = switch_c(C, [&](auto c) {
            return tail ? launch_pass<CutTail, true, c.value>(a, grid, lds, st) : launch_pass<CutHist, true, c.value>(a, grid, lds, st);
        }))
        return rc;
    SREC_LAUNCH_CHECK();
    return 0;
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

// ws of srec_score_cutoff: hist | state | the K = 1 selection's ids | its scratch
extern "C" int srec_score_cutoff_ws(int B, int V, int d, int C, int L, long* bytes) {
    long sel = 0;
    if (bytes == nullptr) return SREC_BAD_ARG;
    if (int rc = srec_score_select_ws(B, V, d, C, L, 1, &sel)) return rc;
    *bytes = (long)((size_t)B * 3 * NBIN * 8 + (size_t)B * NSTATE * 8 + align16((size_t)B * 4) + (size_t)sel);
    return 0;
}

extern "C" int srec_score_cutoff_hist(const void* served, float inv_temperature, int top_k, float top_p, int pass,
                                      const float* top, const long long* state, long long* hist, void* stream) {
    if (served == nullptr || bad_criteria(top_k, top_p, 0.f) || pass < 0 || pass >= NPASS) return SREC_BAD_ARG;
    return hist_launch(*(const srec_served*)served, inv_temperature, top_k > 0, has_p(top_p), pass, top, state, nullptr, hist,
                       stream);
}

extern "C" int srec_score_cutoff_tail(const void* served, float inv_temperature, const float* top, const float* floor,
                                      long long* hist, void* stream) {
    if (served == nullptr) return SREC_BAD_ARG;
    return hist_launch(*(const srec_served*)served, inv_temperature, true, true, NPASS, top, nullptr, floor, hist, stream);
}

extern "C" int srec_score_cutoff_advance(int B, int pass, int top_k, float top_p, float min_gap, const long long* hist,
                                         long long* state, float* top, float* floor, void* stream) {
    if (B <= 0) return 0;
    const bool do_k = top_k > 0, do_p = has_p(top_p), scan = pass < NPASS;
    if (bad_criteria(top_k, top_p, min_gap) || pass < 0 || pass > NPASS || (scan && !do_k && !do_p) || (!scan && (do_k || do_p)) ||
        (scan && (hist == nullptr || state == nullptr)) || (pass >= NPASS - 1 && (top == nullptr || floor == nullptr)) ||
        ((uintptr_t)hist & 7) || ((uintptr_t)state & 7) || ((uintptr_t)top & 3) || ((uintptr_t)floor & 3))
        return SREC_BAD_ARG;
    u64 P = 0;
    if (do_p) {                                                     // p as P / 2^32, P = round(p 2^32) held in [1, 2^32 - 1]
        const double x = __builtin_rint((double)top_p * 4294967296.0);
        P = x < 1.0 ? 1ull : (x > 4294967295.0 ? 4294967295ull : (u64)x);
    }
    hipLaunchKernelGGL(cutoff_advance_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pass, (int)do_k, (int)do_p,
                       (long long)top_k, P, min_gap, hist, state, top, floor);
    SREC_LAUNCH_CHECK();
    return 0;
}

extern "C" int srec_score_cutoff_finish(int B, const long long* hist, int* count, float* log_kept, void* stream) {
    if (B <= 0) return 0;
    if (hist == nullptr || count == nullptr || log_kept == nullptr || ((uintptr_t)hist & 7) || ((uintptr_t)count & 3) ||
        ((uintptr_t)log_kept & 3))
        return SREC_BAD_ARG;
    hipLaunchKernelGGL(cutoff_finish_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, B, hist, count, log_kept);
    SREC_LAUNCH_CHECK();
    return 0;
}

extern "C" int srec_score_cutoff(const void* served, float inv_temperature, int top_k, float top_p, float min_gap, float* floor,
                                 int* count, float* log_kept, float* top, void* ws, void* stream) {
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    const int B = s->B;
    if (B <= 0) return 0;
    PassArgs chk{};
    if (pass_args(chk, *s, true) || bad_inv_t(inv_temperature) || bad_criteria(top_k, top_p, min_gap) || floor == nullptr || count == nullptr ||
        log_kept == nullptr || top == nullptr || ws == nullptr || ((uintptr_t)ws & 15) || ((uintptr_t)floor & 3) ||
        ((uintptr_t)top & 3) || ((uintptr_t)count & 3) || ((uintptr_t)log_kept & 3))
        return SREC_BAD_ARG;
    long long* hist = (long long*)ws;
    long long* state = hist + (size_t)B * 3 * NBIN;
    int* top_id = (int*)(state + (size_t)B * NSTATE);
    void* sel_ws = (char*)top_id + align16((size_t)B * 4);
    // m_b: the value of the K = 1 selection (an eligible row that scores -inf, and nothing eligible, both give -inf)
    if (int rc = srec_score_select(served, 1, nullptr, top, top_id, sel_ws, stream)) return rc;
    if (top_k > 0 || has_p(top_p)) {
        for (int pass = 0; pass < NPASS; ++pass) {
            if (int rc = srec_score_cutoff_hist(served, inv_temperature, top_k, top_p, pass, top, state, hist, stream)) return rc;
            if (int rc = srec_score_cutoff_advance(B, pass, top_k, top_p, min_gap, hist, state, top, floor, stream)) return rc;
        }
    } else if (int rc = srec_score_cutoff_advance(B, NPASS, 0, 1.f, min_gap, nullptr, nullptr, top, floor, stream)) {
        return rc;
    }
    if (int rc = srec_score_cutoff_tail(served, inv_temperature, top, floor, hist, stream)) return rc;
    return srec_score_cutoff_finish(B, hist, count, log_kept, stream);
}
