// srec_score_norm: the log-normaliser of the served score over the ELIGIBLE catalogue, one fp32 number per session, WITHOUT
// the (B, V) score matrix:
//   Z[b] = logsumexp over eligible rows v of ( logsumexp_{c<C}( cs[v] * <sr_c[b], E_v> + off[c,b] ) + bias[group[b], v] )
// Score, layouts, limits and eligibility are those of srec_score_select_biased (recommend.hip): off = off_in if v is in
// listed[b,:] else off_ex (SREC_LISTED_SCORE); under SREC_LISTED_DROP a listed item does not contribute and off_in is not
// read; an item whose bias is -INFINITY does not contribute; rows >= V and sessions >= B never contribute.  Subtracting Z
// from the offsets the select / items kernels take renormalises their values: logsumexp_c(z_c + off_c - Z) = s - Z.
//
// Pass 1 (norm_part_kernel): workgroup = 32 sessions x one item range, 4 wavefronts, the tile product of rank.hip /
//   recommend.hip (score_tile.h: session tiles in LDS or through the cache, item rows streamed into the MFMA B operand, a
//   (session, item) score in one lane).  A lane holds 16 (session, item) scores per chunk and keeps a running online
//   log-sum-exp (m[r], l[r]) per accumulator register across the chunks of its range: one expf per score.  Membership in
//   listed[b,:] is resolved INSIDE the pass with recommend.hip's per-session, per-chunk 128-bit mask (built from the ids
//   compacted into the workgroup's range) - no subtract-and-re-add fix-up: a session's own items routinely hold most of
//   the mass, and exp(Z_all) - exp(s_ex) + exp(s_in) cancels.
//   The partials reduce in a fixed order: across the 32 item lanes of a half-wavefront (max, rescale once, butterfly sum),
//   across the 4 wavefronts through LDS (wave order), then one (m, l) pair per (range, session) goes to the workspace.
// Pass 2 (norm_merge_kernel): one thread per session folds the R partials in range order and writes Z = m + logf(l).
// No float atomics: the result is a pure function of the inputs.  Every merge guards m == -INFINITY (an empty lane, chunk,
// range or session is (-INFINITY, 0), never exp(-inf - -inf)); a session with no eligible row ends as exactly -INFINITY.
// LDS: 1 KB of offsets + 0.6 KB of masks and counts + 32 L ids + 1 KB of wave partials (+ 256 bytes of bias row offsets) +
// the session tiles when the sum stays within 160 KB (C = 3, d = 256, L = 64, groups: 108.4 KB; C = 1, d = 1024: 139.4 KB), else
// the tiles are read through the cache.
#include "common.h"
#include "score_tile.h"

namespace {

using namespace score_tile;

struct NormArgs {
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
    float* part;                    // [R][B][2] per-range (m, l)
};

inline size_t norm_lds(int C, int d, int L, bool sr_lds, bool grouped) {
    const size_t head = (size_t)(2 * MAXCOMP * SB + SB * 4 + SB + 4 * SB * 2) * 4;
    return head + (size_t)SB * L * 4 + (grouped ? (size_t)SB * 8 : 0) + (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS, int BIAS>
__global__ __launch_bounds__(256) void norm_part_kernel(NormArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d, L = a.L;
    float* offs = smem;                                             // [MAXCOMP][SB] off_ex
    float* offi = offs + MAXCOMP * SB;                              // [MAXCOMP][SB] off_in (SCORE mode)
    unsigned* inm = reinterpret_cast<unsigned*>(offi + MAXCOMP * SB);   // [SB][4] listed items of this chunk
    int* nin = reinterpret_cast<int*>(inm + SB * 4);                // [SB] listed ids inside this workgroup's range
    float* red = reinterpret_cast<float*>(nin + SB);                // [4][SB][2] (m, l) of every wavefront
    int* lst = reinterpret_cast<int*>(red + 4 * SB * 2);            // [SB][L] listed ids as local rows, in-range ones first
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

    float m[16], l[16];             // running log-sum-exp of (session session_of(r, half), this lane's items)
#pragma unroll
    for (int r = 0; r < 16; ++r) { m[r] = -INFINITY; l[r] = 0.f; }

    for (int base = v0; base < v1; base += CHUNK) {
        if (has_list) {
            __syncthreads();          // the epilogue of the previous chunk has read its membership bits
            if (tid < SB * 4) {       // thread (session, 32-item word): membership bits
                const int j = tid >> 2, w = tid & 3, n = nin[j];
                unsigned bits = 0u;
                for (int i = 0; i < n; ++i) {
                    const int o = lst[j * L + i] - base - 32 * w;
                    if (o >= 0 && o < 32) bits |= 1u << o;
                }
                inm[tid] = bits;
            }
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
        if (has_list) __syncthreads();    // membership bits written

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
            bool elig = vok && !(in && drop);       // (sessions >= B are dropped when the partials are written)
            if constexpr (BIAS != 0) {
                const float bb = BIAS == 1 ? bv : bg[BIAS == 2 ? r : 0];
                s += bb;
                elig = elig && bb != -INFINITY;     // not in the catalogue of this session
            }
            // one expf: the smaller of (m, s) relative to the larger.  s == -inf adds nothing and must not meet m == -inf.
            const bool add = elig && s != -INFINITY;
            const float hi = fmaxf(m[r], s);
            const float e = expf(fminf(m[r], s) - hi);
            const float ln = s > m[r] ? l[r] * e + 1.f : l[r] + e;
            l[r] = add ? ln : l[r];
            m[r] = add ? hi : m[r];
        }
    }

    // 32 item lanes of a half-wavefront -> one (m, l) per session: max, one rescale, butterfly sum (a fixed order)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float mm = m[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o, 64));
        float ll = m[r] == -INFINITY ? 0.f : l[r] * expf(m[r] - mm);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) ll += __shfl_xor(ll, o, 64);
        if (l31 == 0) {
            const int sl = session_of(r, half);
            red[(wave * SB + sl) * 2] = mm;
            red[(wave * SB + sl) * 2 + 1] = ll;
        }
    }
    __syncthreads();
    if (tid < SB && b0 + tid < a.B) {                               // the 4 wavefronts, in wave order
        float mm = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) mm = fmaxf(mm, red[(w * SB + tid) * 2]);
        float ll = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = red[(w * SB + tid) * 2];
            if (mw != -INFINITY) ll += red[(w * SB + tid) * 2 + 1] * expf(mw - mm);
        }
        float* p = a.part + ((size_t)range * a.B + b0 + tid) * 2;
        p[0] = mm; p[1] = ll;
    }
}

__global__ __launch_bounds__(256) void norm_merge_kernel(const float* __restrict__ part, int R, int B, float* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float mm = -INFINITY;
    for (int r = 0; r < R; ++r) mm = fmaxf(mm, part[((size_t)r * B + b) * 2]);
    float ll = 0.f;
    for (int r = 0; r < R; ++r) {                                   // range order
        const float mr = part[((size_t)r * B + b) * 2];
        if (mr != -INFINITY) ll += part[((size_t)r * B + b) * 2 + 1] * expf(mr - mm);
    }
    out[b] = mm == -INFINITY ? -INFINITY : mm + logf(ll);
}

inline int pick_ranges(int B, int V) {
    const int tiles = cdiv(B, SB);
    int R = cdiv(1024, tiles);                                  // ~4 workgroups per CU (as rank.hip)
    const int maxR = cdiv(V, 2 * CHUNK);                        // at least 2 chunks per range
    if (R > maxR) R = maxR;
    return R < 1 ? 1 : R;
}

template <int C, bool SR_LDS, int BIAS>
int launch_part(const NormArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    static std::atomic<unsigned long long> optin{0};
    if (int rc = srec_lds_optin((const void*)norm_part_kernel<C, SR_LDS, BIAS>, LDS_BYTES, optin)) return rc;
    hipLaunchKernelGGL((norm_part_kernel<C, SR_LDS, BIAS>), grid, dim3(256), lds, st, a);
    return 0;
}

template <int C, int BIAS>
int run_part(const NormArgs& a, dim3 grid, hipStream_t st) {
    const bool fits = norm_lds(C, a.d, a.L, true, BIAS == 2) <= (size_t)LDS_BYTES;
    return fits ? launch_part<C, true, BIAS>(a, grid, norm_lds(C, a.d, a.L, true, BIAS == 2), st)
                : launch_part<C, false, BIAS>(a, grid, norm_lds(C, a.d, a.L, false, BIAS == 2), st);
}

template <int C>
int run(const NormArgs& a, int R, float* out, hipStream_t st) {
    const dim3 grid(R, cdiv(a.B, SB));
    const int rc = a.bias == nullptr ? run_part<C, 0>(a, grid, st)
                   : a.G == 1        ? run_part<C, 1>(a, grid, st)
                                     : run_part<C, 2>(a, grid, st);
    if (rc) return rc;
    hipLaunchKernelGGL(norm_merge_kernel, dim3(cdiv(a.B, 256)), dim3(256), 0, st, a.part, R, a.B, out);
    SREC_LAUNCH_CHECK();
    return 0;
}

bool bad_shape(int B, int V, int d, int C, int L) {
    return B <= 0 || V <= 0 || d <= 0 || (d & 3) || d > 1024 || C < 1 || C > MAXCOMP || L < 0 || L > MAXL;
}

}  // namespace

// ws: one (m, l) pair per (range, session)
extern "C" int srec_score_norm_ws(int B, int V, int d, int C, int L, long* bytes) {
    if (bad_shape(B, V, d, C, L) || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = (long)pick_ranges(B, V) * B * 8;
    return 0;
}

extern "C" int srec_score_norm(const float* sr, int ld_sr, long comp_stride, const float* E, int ld_e, const float* cs,
                               const float* off_ex, const float* off_in, const int* listed, int L, int listed_mode,
                               long id_lo, int B, int V, int d, int C, const float* bias, long ld_bias,
                               const int* group, int G, float* out, void* ws, void* stream) {
    if (B <= 0) return 0;
    if (bad_shape(B, V, d, C, L) || (ld_sr & 3) || (ld_e & 3) || (comp_stride & 3) || ((uintptr_t)E & 15) ||
        ((uintptr_t)sr & 15) || out == nullptr || ws == nullptr || id_lo < 0 || id_lo + (long)V > 0x7fffffffL ||
        (listed_mode != 0 && listed_mode != 1) || G < 1 || (group == nullptr && G > 1) ||
        (bias != nullptr && G > 1 && ld_bias < (long)V) || ((uintptr_t)bias & 3) || ((uintptr_t)group & 3))
        return SREC_BAD_ARG;
    NormArgs a{};
    a.sr = sr; a.ld_sr = ld_sr; a.comp_stride = comp_stride; a.E = E; a.ld_e = ld_e; a.cs = cs;
    a.off_ex = off_ex; a.off_in = off_in; a.listed = L > 0 ? listed : nullptr; a.L = a.listed != nullptr ? L : 0;
    a.drop = listed_mode; a.id_lo = id_lo; a.B = B; a.V = V; a.d = d;
    a.bias = bias; a.ld_bias = ld_bias; a.group = group; a.G = G;
    const int R = pick_ranges(B, V);
    a.items_per_range = cdiv(cdiv(V, R), CHUNK) * CHUNK;
    const int Ract = cdiv(V, a.items_per_range);
    a.part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: return run<1>(a, Ract, out, st);
        case 2: return run<2>(a, Ract, out, st);
        case 3: return run<3>(a, Ract, out, st);
        default: return run<4>(a, Ract, out, st);
    }
}
