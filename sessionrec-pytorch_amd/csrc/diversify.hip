// srec_diversify: greedy MMR (maximal marginal relevance) re-rank of a pool of M <= 128 slots per session, and the intra-list
// diversity of what it picked - WITHOUT the [B, M, d] gather, the [B, M, M] Gram matrix and the K-step host loop of launches
// that the composition in PyTorch needs.
//   slot i of a session: row[i] into X (fp32, leading dimension ld_x; row[i] < 0 or >= n_rows: the slot is UNFILLED and X is
//     never read for it) and a value s[i].
//   sim(i, j) = <X_i, X_j> / (max(|X_i|, 1e-12) max(|X_j|, 1e-12)); a zero row has similarity 0 to everything, never NaN.
//   for t = 0 .. K-1:  m_t(i) = s[i] - theta * pen_t(i) over the filled slots not yet picked, pen_0 = 0, pen_t(i) = max of
//     sim(i, j) over the slots j picked so far (the RAW maximum: a negative cosine raises m); the pick is the largest m_t,
//     ties to the lower slot.  theta == 0: m_t = s[i] and the rows are not looked at for the order.
//   pick [B, K] slot numbers in pick order (-1 once the filled slots run out), val [B, K] = s[pick] COPIED (-inf in the
//     tail), mmr [B, K] the winning m_t (-inf in the tail), ild [B] = 1 - mean_{a<b} sim(pick_a, pick_b) over the filled picks
//     (0 with fewer than two) - the loop holds every one of those cosines already.
//
// One workgroup (256 threads) per session, no atomics, nothing shared between workgroups: a session's result is the same
// bits in any batch.  The cosines are taken LAZILY - M dot products against the row just picked per step, K M d
// multiply-adds in all - not from an up-front M x M Gram matrix on the MFMA tile: at the serving shape (M 128, K 20) that is
// 6.4 times fewer multiply-adds, and the Gram matrix itself (64 KB) would not fit beside the rows (133 KB) in LDS.  Work and
// measured time: DESIGN.md section 4.
//   rows: staged once into LDS as fp32 [M][ld], ld = d or d + 4 so that ld / 4 is odd, when M ld 4 bytes plus the slot state
//     fit LDS_BYTES (M 128, d 256: 133 120 + 4 608 bytes); otherwise read in place through the cache - same code, same
//     order of every sum, same result.
//   a dot product: thread (slot i = tid & 127, half h = tid >> 7) takes the 16-byte column groups h, h + 2, ... of row i
//     against the picked row, four accumulators, summed (x + y) + (z + w); the halves meet in LDS as half 0 + half 1.  All
//     64 lanes of a wavefront read the SAME column group of 64 consecutive rows: with ld / 4 odd the 16 lanes of every
//     ds_read_b128 group fall on 16 different 16-byte slots (conflict-free), and the picked row's group is one address
//     (a broadcast).
//   arg-max: wavefront 0, two slots per lane, a butterfly on (value, slot) - lower slot on equal values.
//   ild: after the cosines against pick t are there, wavefront 0 adds sim(pick_a, pick_t) for a < t (lane a, butterfly sum),
//     step sums accumulated in double: a fixed order.
#include "common.h"
#include "score_pass.h"

namespace {

using score_tile::LDS_BYTES;

constexpr int MAXM = 128;               // SREC_SELECT_MAXK: the pools are recommend()'s lists
constexpr int STATE_WORDS = 9 * MAXM;   // srow, sval, inv, pen, sim, part[2], taken, picks

struct DivArgs {
    const float* X; int ld_x; long n_rows;
    const int* row; const float* s;
    int M, K, d;
    float theta;
    int* pick; float* val; float* mmr; float* ild;
};

// row stride of the LDS copy: 16-byte aligned, an odd number of 16-byte slots
__host__ __device__ __forceinline__ int row_ld(int d) { return ((d >> 2) & 1) ? d : d + 4; }
inline size_t div_lds(int M, int d, bool rows) { return (size_t)STATE_WORDS * 4 + (rows ? (size_t)M * row_ld(d) * 4 : 0); }

// this thread's half of <x, y>: the column groups half, half + 2, ... of nq
__device__ __forceinline__ float half_dot(const float* x, const float* y, int half, int nq) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int c = half; c < nq; c += 2) {
        const float4 u = *reinterpret_cast<const float4*>(x + 4 * c);
        const float4 v = *reinterpret_cast<const float4*>(y + 4 * c);
        acc.x = fmaf(u.x, v.x, acc.x);
        acc.y = fmaf(u.y, v.y, acc.y);
        acc.z = fmaf(u.z, v.z, acc.z);
        acc.w = fmaf(u.w, v.w, acc.w);
    }
    return (acc.x + acc.y) + (acc.z + acc.w);
}

// (C and BIAS: the template shape of score_pass.h's launch_placed; one instance each)
template <int C, bool ROWS_LDS, int BIAS>
__global__ __launch_bounds__(256) void diversify_kernel(DivArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int* srow = reinterpret_cast<int*>(smem);                       // [MAXM] row of X, -1: unfilled
    float* sval = smem + MAXM;                                      // [MAXM] s
    float* inv = sval + MAXM;                                       // [MAXM] 1 / max(|X_i|, 1e-12)
    float* pen = inv + MAXM;                                        // [MAXM] max cosine to the picks so far
    float* sim = pen + MAXM;                                        // [MAXM] cosine to the latest pick
    float* part = sim + MAXM;                                       // [2][MAXM] the halves of a dot product
    int* taken = reinterpret_cast<int*>(part + 2 * MAXM);           // [MAXM] picked, or unfilled
    int* picks = taken + MAXM;                                      // [MAXM] slot of pick t
    float* R = reinterpret_cast<float*>(picks + MAXM);              // [M][LD] (ROWS_LDS)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.M, K = a.K, d = a.d, nq = d >> 2, LD = row_ld(d);
    const size_t b = blockIdx.x;
    const float theta = a.theta;

    if (tid < MAXM) {
        int r = -1;
        float v = -INFINITY;
        if (tid < M) {
            const int x = a.row[b * M + tid];
            if (x >= 0 && (long)x < a.n_rows) r = x;                // anything else is an unfilled slot: never dereferenced
            v = a.s[b * M + tid];
        }
        srow[tid] = r;
        sval[tid] = v;
        pen[tid] = 0.f;
        sim[tid] = 0.f;
        taken[tid] = r < 0;
    }
    __syncthreads();
    if (ROWS_LDS) {
#pragma unroll 4
        for (int i = tid; i < M * nq; i += 256) {
            const int sl = i / nq, c = i - sl * nq, r = srow[sl];
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r >= 0) x = *reinterpret_cast<const float4*>(a.X + (size_t)r * a.ld_x + 4 * c);
            *reinterpret_cast<float4*>(R + (size_t)sl * LD + 4 * c) = x;
        }
        __syncthreads();
    }

    const int slot = tid & (MAXM - 1), half = tid >> 7;
    const bool live = slot < M && srow[slot] >= 0;
    const float* mine = ROWS_LDS ? R + (size_t)slot * LD : a.X + (size_t)(live ? srow[slot] : 0) * a.ld_x;

    if (live) part[half * MAXM + slot] = half_dot(mine, mine, half, nq);
    __syncthreads();
    if (half == 0 && live) inv[slot] = 1.f / fmaxf(sqrtf(part[slot] + part[MAXM + slot]), 1e-12f);

    double pairs = 0.0;                                             // wavefront 0: sum of sim over the pairs of picks so far
    int n = 0;                                                      // picks made
    for (int t = 0; t < K; ++t) {
        __syncthreads();                                            // inv, pen, sim of the previous step
        if (wave == 0) {
            if (t > 1) {                                            // pick t-1 against the picks before it
                float v = 0.f;
                for (int q = lane; q < t - 1; q += 64) v += sim[picks[q]];
                pairs += (double)wave_sum(v);
            }
            float bv = -INFINITY;
            int bi = -1;
            for (int j = lane; j < M; j += 64) {
                if (!taken[j]) {
                    const float m = theta == 0.f ? sval[j] : fmaf(-theta, pen[j], sval[j]);
                    if (bi < 0 || m > bv) { bv = m; bi = j; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            if (lane == 0) {
                picks[t] = bi;
                if (bi >= 0) {
                    taken[bi] = 1;
                    a.pick[b * K + t] = bi;
                    a.val[b * K + t] = sval[bi];
                    if (a.mmr != nullptr) a.mmr[b * K + t] = bv;
                }
            }
        }
        __syncthreads();
        const int p = picks[t];
        if (p < 0) break;                                           // (uniform) the filled slots ran out
        n = t + 1;
        const float* prow = ROWS_LDS ? R + (size_t)p * LD : a.X + (size_t)srow[p] * a.ld_x;
        if (live) part[half * MAXM + slot] = half_dot(mine, prow, half, nq);
        __syncthreads();
        if (half == 0 && live) {
            const float c = (part[slot] + part[MAXM + slot]) * inv[slot] * inv[p];
            sim[slot] = c;
            pen[slot] = t == 0 ? c : fmaxf(pen[slot], c);
        }
    }
    __syncthreads();
    if (wave == 0) {
        if (n == K && K > 1) {                                      // the last pick's cosines (a break has added its own)
            float v = 0.f;
            for (int q = lane; q < K - 1; q += 64) v += sim[picks[q]];
            pairs += (double)wave_sum(v);
        }
        for (int t = n + lane; t < K; t += 64) {
            a.pick[b * K + t] = -1;
            a.val[b * K + t] = -INFINITY;
            if (a.mmr != nullptr) a.mmr[b * K + t] = -INFINITY;
        }
        if (lane == 0 && a.ild != nullptr)
            a.ild[b] = n >= 2 ? (float)(1.0 - pairs / (0.5 * (double)n * (double)(n - 1))) : 0.f;
    }
}

template <int C, bool ROWS_LDS, int BIAS>
struct Diversify { static constexpr auto kernel = diversify_kernel<C, ROWS_LDS, BIAS>; };

}  // namespace

extern "C" int srec_diversify(const float* X, int ld_x, long n_rows, const int* row, const float* s, int B, int M, int K, int d,
                              float theta, int* pick, float* val, float* mmr, float* ild, void* stream) {
    if (B <= 0) return 0;
    if (M < 1 || M > MAXM || K < 1 || K > M || d <= 0 || (d & 3) || d > 1024 || (ld_x & 3) || ld_x < d || n_rows < 0 ||
        X == nullptr || ((uintptr_t)X & 15) || row == nullptr || s == nullptr || pick == nullptr || val == nullptr ||
        ((uintptr_t)row & 3) || ((uintptr_t)s & 3) || ((uintptr_t)pick & 3) || ((uintptr_t)val & 3) || ((uintptr_t)mmr & 3) ||
        ((uintptr_t)ild & 3) || !(theta >= 0.f) || theta > 3.4028234664e38f)
        return SREC_BAD_ARG;
    const DivArgs a{X, ld_x, n_rows, row, s, M, K, d, theta, pick, val, mmr, ild};
    const auto lds = [&](int, bool rows, bool) { return div_lds(M, d, rows); };
    if (int rc = score_tile::launch_placed<Diversify, 1, 0>(a, dim3(B), lds, (hipStream_t)stream)) return rc;
    SREC_LAUNCH_CHECK();
    return 0;
}
