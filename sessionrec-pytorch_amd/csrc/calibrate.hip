// srec_calibrate: the greedy CALIBRATED re-rank (Steck, "Calibrated Recommendations", RecSys 2018) of a pool of M <= 128 slots
// per session - a list whose category mix follows a target distribution - WITHOUT the K-step host loop of small launches over
// [B, M, categories] temporaries that the composition in PyTorch needs.  The soft counterpart of cap_select.hip's hard caps.
//   slot i of a session: ids[i] (FILLED iff 0 <= id < n_items; anything else is never dereferenced), a value s[i] and the
//     category c_i = category[ids[i]] (< 0: the item has none).
//   target: T pairs (tcat[j], tw[j]) of a CATEGORY id and a weight; tcat < 0 or !(tw > 0): an empty pair; duplicates add up.
//     P_c = the sum of the weights of category c, S = {c: P_c > 0}, W = the sum of P_c over S, p_c = P_c / W.  W > 0 fails
//     (T == 0, every pair empty): the session has NO TARGET and its calibration term is 0.
//   state: n_c picks of category c, N picks with ANY category >= 0 (in S or not; uncategorised picks count nowhere).
//     KL(n, N) = sum_{c in S} p_c log(p_c / ((1 - a) n_c / max(N, 1) + a p_c)),  a = smooth in (0, 1).
//   for t = 0 .. K-1:  m_t(i) = (1 - w) s_i - w KL(state with slot i added) over the filled slots not yet picked; the pick is the
//     largest m_t, ties to the lower slot.  w == 0: m = s_i and the target is not looked at; s_i == -inf: m = -inf (never NaN).
//   pick [B, K] slot numbers in pick order (-1 once the filled slots run out), val [B, K] = s[pick] COPIED (-inf in the tail),
//     obj [B, K] the winning m_t (-inf in the tail), kl [B] = KL of the final picks (0 without a target).
//
// One workgroup (256 threads) per session, no atomics, nothing shared between workgroups: a session's result is the same bits
// in any batch.  Category ids are only COMPARED - no table indexed by them, no upper bound on them:
//   entries: the M slots (entry i) and the T pairs (entry 128 + j), one per thread.  An all-pairs compare gives every entry
//     the index of the FIRST entry with its category: its class, at most 256 of them.  Every thread sums the weights of its
//     own category over the pairs in pair order (double), so all entries of a category hold the same P, and W in pair order.
//   a step: adding slot i changes the state in one of three ways only - not at all (uncategorised), N + 1 (a category outside
//     S), N + 1 and n_c + 1 (c in S).  The first thread of every class in S holds n_c in a register and evaluates its term at
//     (n_c, max(N, 1)), (n_c, N + 1) and (n_c + 1, N + 1): two fixed-order workgroup sums give KL for the first two ways, and
//     KL of the third is the second sum plus the class's own difference.  The calibration term is thus formed ONCE PER
//     CATEGORY (3 |S| logs per step), and two slots of one category - or two outside S, or two uncategorised ones - with the
//     same s get the same bits: their tie goes to the lower slot.
//   everything the order depends on is double: the weights' sums, the terms, m_t and its comparison - a float64 loop on the
//     host reproduces the picks with == wherever its two best candidates are further apart than double round-off.
//   arg-max: wavefront 0, two slots per lane (their s, kind and class in registers), a butterfly on (m, slot).
#include "common.h"

namespace {

constexpr int MAXM = 128;               // SREC_SELECT_MAXK: the pools are recommend()'s lists
constexpr int MAXT = 128;               // SREC_CALIB_MAXT
constexpr int NE = MAXM + MAXT;         // entries = threads

struct CalArgs {
    const int* ids; const float* s;
    int M, K;
    const int* category; long n_items;
    const int* tcat; const float* tw; int T;
    float weight, smooth;
    int* pick; float* val; float* obj; float* kl;
};

enum { UNFILLED = -1, NOCAT = 0, OUTSIDE = 1, INSIDE = 2 };     // what adding a slot does to the state

static __device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// p log(p / ((1 - a) n / D + a p)): the term of a category of S with n of the D categorised picks
static __device__ __forceinline__ double kl_term(double p, double a, int n, int D) {
    return p * log(p / ((1.0 - a) * (double)n / (double)D + a * p));
}

__global__ __launch_bounds__(NE) void calibrate_kernel(CalArgs a) {
    __shared__ int ecat[NE];            // the category of an entry, -1: none (unfilled, uncategorised, an empty pair)
    __shared__ float etw[MAXT];         // the weight of pair j, 0: empty
    __shared__ int skind[MAXM];         // UNFILLED / NOCAT / OUTSIDE / INSIDE
    __shared__ int scls[MAXM];          // the class of a slot of kind INSIDE
    __shared__ float sval[MAXM];
    __shared__ int picks[MAXM];
    __shared__ double delta[NE];        // per class: term(n + 1, N + 1) - term(n, N + 1)
    __shared__ double part[2][4];       // the wavefronts' sums of term(n, max(N, 1)) and term(n, N + 1)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.M, K = a.K, T = a.T;
    const size_t b = blockIdx.x;
    const double w = (double)a.weight, sm = (double)a.smooth;

    // ---- entries
    int cat = -1;
    bool filled = false;
    if (tid < MAXM) {
        float v = -INFINITY;
        if (tid < M) {
            const int x = a.ids[b * M + tid];
            if (x >= 0 && (long)x < a.n_items) {                   // anything else is an unfilled slot: never dereferenced
                filled = true;
                const int c = a.category[x];
                cat = c < 0 ? -1 : c;
            }
            v = a.s[b * M + tid];
        }
        sval[tid] = v;
    } else {
        const int j = tid - MAXM;
        float x = 0.f;
        if (j < T) {
            const int c = a.tcat[b * T + j];
            const float y = a.tw[b * T + j];
            if (c >= 0 && y > 0.f) { cat = c; x = y; }             // (NaN > 0 is false: an empty pair)
        }
        etw[j] = x;
    }
    ecat[tid] = cat;
    __syncthreads();

    // ---- classes and the target distribution
    int cls = tid;
    double P = 0.0, W = 0.0;
    if (cat >= 0)
        for (int e = NE - 1; e >= 0; --e) cls = ecat[e] == cat ? e : cls;
    for (int j = 0; j < T; ++j) {                                   // pair order: the same bits in every thread of a category
        const double x = (double)etw[j];
        W += x;
        P += (cat >= 0 && ecat[MAXM + j] == cat) ? x : 0.0;
    }
    const bool target = W > 0.0;                                    // (uniform)
    const bool head = target && cat >= 0 && cls == tid && P > 0.0;  // this thread owns a class of S
    const double p = head ? P / W : 0.0;
    if (tid < MAXM) {
        skind[tid] = !filled ? UNFILLED : cat < 0 ? NOCAT : (target && P > 0.0) ? INSIDE : OUTSIDE;
        scls[tid] = cls;
    }
    __syncthreads();

    // wavefront 0: slots lane and lane + 64
    float s0 = 0.f, s1 = 0.f;
    int k0 = UNFILLED, k1 = UNFILLED, c0 = 0, c1 = 0;
    if (wave == 0) {
        s0 = sval[lane]; k0 = skind[lane]; c0 = scls[lane];
        s1 = sval[lane + 64]; k1 = skind[lane + 64]; c1 = scls[lane + 64];
    }

    const bool look = target && w != 0.0;                           // (uniform) the order depends on the target
    int n_c = 0, N = 0, n = 0;                                      // picks of my class (head), categorised picks, picks
    for (int t = 0; t <= K; ++t) {
        // the terms of the classes of S under the state so far; t == K, or the slots ran out: only KL of the final picks
        const bool last = t == K || (t > 0 && picks[t - 1] < 0);
        if (look || (last && target)) {
            double t0 = 0.0, t1 = 0.0;
            if (head) {
                t0 = kl_term(p, sm, n_c, N > 1 ? N : 1);
                if (!last) {
                    t1 = N > 0 ? kl_term(p, sm, n_c, N + 1) : t0;
                    delta[tid] = kl_term(p, sm, n_c + 1, N + 1) - t1;
                }
            }
            t0 = wave_sum_f64(t0);
            t1 = wave_sum_f64(t1);
            if (lane == 0) { part[0][wave] = t0; part[1][wave] = t1; }
        }
        __syncthreads();
        if (last) {
            if (tid == 0 && a.kl != nullptr)
                a.kl[b] = target ? (float)(((part[0][0] + part[0][1]) + (part[0][2] + part[0][3]))) : 0.f;
            break;
        }
        if (wave == 0) {
            double kl0 = 0.0, kl1 = 0.0;
            if (look) {
                kl0 = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
                kl1 = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
            }
            double bv = -INFINITY;
            int bi = -1;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kind = h ? k1 : k0, j = lane + 64 * h;
                if (kind != UNFILLED) {
                    const float s = h ? s1 : s0;
                    double m;
                    if (s == -INFINITY) m = -INFINITY;
                    else if (w == 0.0) m = (double)s;
                    else {
                        double kl = kind == NOCAT ? kl0 : kl1;
                        if (look && kind == INSIDE) kl += delta[h ? c1 : c0];
                        m = (1.0 - w) * (double)s - w * kl;
                    }
                    if (bi < 0 || m > bv) { bv = m; bi = j; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            if (lane == 0) {
                picks[t] = bi;
                if (bi >= 0) {
                    a.pick[b * K + t] = bi;
                    a.val[b * K + t] = sval[bi];
                    if (a.obj != nullptr) a.obj[b * K + t] = (float)bv;
                }
            }
        }
        __syncthreads();
        const int pk = picks[t];
        if (pk < 0) continue;                                       // (uniform) the filled slots ran out: the next round is the last
        n = t + 1;
        if (wave == 0) {
            if (pk == lane) k0 = UNFILLED;
            if (pk == lane + 64) k1 = UNFILLED;
        }
        if (skind[pk] != NOCAT) {
            ++N;
            if (skind[pk] == INSIDE && scls[pk] == tid) ++n_c;
        }
    }
    if (wave == 0)
        for (int t = n + lane; t < K; t += 64) {
            a.pick[b * K + t] = -1;
            a.val[b * K + t] = -INFINITY;
            if (a.obj != nullptr) a.obj[b * K + t] = -INFINITY;
        }
}

}  // namespace

extern "C" int srec_calibrate(const int* ids, const float* s, int B, int M, int K, const int* category, long n_items,
                              const int* tcat, const float* tw, int T, float weight, float smooth, int* pick, float* val,
                              float* obj, float* kl, void* stream) {
    if (B <= 0) return 0;
    if (M < 1 || M > MAXM || K < 1 || K > M || T < 0 || T > MAXT || n_items < 0 || !(weight >= 0.f && weight <= 1.f) ||
        !(smooth > 0.f && smooth < 1.f) || ids == nullptr || s == nullptr || category == nullptr || pick == nullptr ||
        val == nullptr || (T > 0 && (tcat == nullptr || tw == nullptr)) || ((uintptr_t)ids & 3) || ((uintptr_t)s & 3) ||
        ((uintptr_t)category & 3) || ((uintptr_t)tcat & 3) || ((uintptr_t)tw & 3) || ((uintptr_t)pick & 3) ||
        ((uintptr_t)val & 3) || ((uintptr_t)obj & 3) || ((uintptr_t)kl & 3))
        return SREC_BAD_ARG;
    const CalArgs a{ids, s, M, K, category, n_items, tcat, tw, T, weight, smooth, pick, val, obj, kl};
    hipLaunchKernelGGL(calibrate_kernel, dim3(B), dim3(NE), 0, (hipStream_t)stream, a);
    SREC_LAUNCH_CHECK();
    return 0;
}
