// srec_score_norm: the log-normaliser of the served score (score_pass.h: score, eligibility, layouts and limits) over the
// ELIGIBLE catalogue, one fp32 number per session, WITHOUT the (B, V) score matrix:
//   Z[b] = logsumexp over eligible rows v of s[b,v]
// Subtracting Z from the offsets the select / items kernels take renormalises their values:
// logsumexp_c(z_c + off_c - Z) = s - Z.
//
// Pass 1 (norm_part_kernel): the pass of score_pass.h.  A lane holds 16 (session, item) scores per chunk and keeps a running
//   online log-sum-exp (m[r], l[r]) per accumulator register across the chunks of its range: one expf per score.  Listed
//   items are resolved by the pass's in-range mask - no subtract-and-re-add fix-up: a session's own items routinely hold
//   most of the mass, and exp(Z_all) - exp(s_ex) + exp(s_in) cancels.  Nothing separates one chunk's epilogue from the next
//   chunk's mask, so the mask takes two barriers per chunk (none without a listed set).
//   The partials reduce in a fixed order: across the 32 item lanes of a half-wavefront (max, rescale once, butterfly sum),
//   across the 4 wavefronts through LDS (wave order), then one (m, l) pair per (range, session) goes to the workspace.
// Pass 2 (norm_merge_kernel): one thread per session folds the R partials in range order and writes Z = m + logf(l).
// No float atomics: the result is a pure function of the inputs.  Every merge guards m == -INFINITY (an empty lane, chunk,
// range or session is (-INFINITY, 0), never exp(-inf - -inf)); a session with no eligible row ends as exactly -INFINITY.
// LDS (norm_lds): the pass's 1.6 KB of offsets, mask and counts, 32 L ids (and 256 bytes of bias row offsets with G rows) +
// 1 KB of wave partials + the session tiles when the sum stays within 160 KB (L = 64, groups: C = 3, d = 256 108.4 KB; C = 1,
// d = 1024 139.4 KB), else the tiles are read through the cache.
#include "common.h"
#include "score_pass.h"

namespace {

using namespace score_tile;

struct NormArgs : PassArgs {
    float* part;                    // [R][B][2] per-range (m, l)
};

inline size_t norm_lds(int C, int d, int L, bool sr_lds, bool grouped) {
    return pass_lds(L, grouped) + (size_t)4 * SB * 2 * 4 + (sr_lds ? tile_bytes(C, d) : 0);
}

template <int C, bool SR_LDS, int BIAS>
__global__ __launch_bounds__(256) void norm_part_kernel(NormArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d, L = a.L;
    float* offs = smem;                                             // the pass's arrays (PassLds) among this kernel's:
    float* offi = offs + MAXCOMP * SB;
    unsigned* inm = reinterpret_cast<unsigned*>(offi + MAXCOMP * SB);
    int* nin = reinterpret_cast<int*>(inm + SB * 4);
    float* red = reinterpret_cast<float*>(nin + SB);                // [4][SB][2] (m, l) of every wavefront
    int* lst = reinterpret_cast<int*>(red + 4 * SB * 2);
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(lst + SB * L);
    float* Ss = reinterpret_cast<float*>(goff + (BIAS == 2 ? SB : 0));  // [C][SB][LD] (SR_LDS); 16-byte aligned: all counts above are multiples of 4

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b0 = blockIdx.y * SB, range = blockIdx.x;
    const int v0 = range * a.items_per_range, v1 = min(a.V, v0 + a.items_per_range);
    const PassLds<true> ps{offs, offi, inm, nin, lst, goff, L > 0, a.drop != 0};

    SCORE_PASS_STAGE_OFFSETS(C, a, ps, b0, tid)
    SCORE_PASS_PROLOGUE(BIAS, a, ps, b0, v0, v1, tid, lane, wave)
    if (SR_LDS) stage_tiles<C>(Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, tid);
    __syncthreads();

    const float* arow[C];
    a_rows<C, SR_LDS>(arow, Ss, a.sr, a.ld_sr, a.comp_stride, b0, a.B, d, l31, half);

    float m[16], l[16];             // running log-sum-exp of (session session_of(r, half), this lane's items)
#pragma unroll
    for (int r = 0; r < 16; ++r) { m[r] = -INFINITY; l[r] = 0.f; }

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
            const bool elig = SCORE_PASS_ELIGIBLE(it, in, ps, true, bias_ok);   // (sessions >= B: dropped with the partials)
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

template <int C, bool SR_LDS, int BIAS>
struct NormPart { static constexpr auto kernel = norm_part_kernel<C, SR_LDS, BIAS>; };

inline int ranges(int B, int V) { return pick_ranges(B, V, 1024, 2); }  // ~4 workgroups per CU (as rank.hip)

}  // namespace

// ws: one (m, l) pair per (range, session)
extern "C" int srec_score_norm_ws(int B, int V, int d, int C, int L, long* bytes) {
    if (bad_shape(B, V, d, C, L) || bytes == nullptr) return SREC_BAD_ARG;
    *bytes = (long)ranges(B, V) * B * 8;
    return 0;
}

extern "C" int srec_score_norm(const void* served, float* out, void* ws, void* stream) {
    const srec_served* s = (const srec_served*)served;
    if (s == nullptr) return SREC_BAD_ARG;
    if (s->B <= 0) return 0;
    NormArgs a{};
    if (pass_args(a, *s, true) || out == nullptr || ws == nullptr) return SREC_BAD_ARG;
    const int B = s->B, V = s->V, d = s->d, C = s->C;
    const dim3 grid(split_ranges(a, ranges(B, V)), cdiv(B, SB));
    a.part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    const auto lds = [&](int c, bool sr_lds, bool grouped) { return norm_lds(c, d, a.L, sr_lds, grouped); };
    if (int rc = switch_c(C, [&](auto c) { return launch_pass<NormPart, true, c.value>(a, grid, lds, st); })) return rc;
    hipLaunchKernelGGL(norm_merge_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, a.part, (int)grid.x, B, out);
    SREC_LAUNCH_CHECK();
    return 0;
}
