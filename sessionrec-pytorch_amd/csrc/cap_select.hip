// srec_cap_select: the capped top-K of an ORDERED pool - "at most caps[c] items of category c in the list" - WITHOUT the
// [B, P] host read and the Python loop per session that the rule costs otherwise.  Caps per category form a partition
// matroid, so walking the served order and skipping an item once its category is full IS the optimum, and the pool's order
// already exists: everything here is integer logic on it, the values are copied.
//   slot i of session b: ids[b, i] (FILLED iff 0 <= id < n_items; anything else is never dereferenced) and a value s[b, i].
//   c_i = category[ids[b, i]]; c_i < 0 or >= G: the item has no category and is always accepted (caps and the counters are
//     never indexed with it).  Otherwise the slot is accepted iff the number of EARLIER filled slots of the session with
//     the same category is < caps[c_i] - which equals "earlier ACCEPTED ones < cap", so every slot is decided on its own.
//   pick [B, K] the slot numbers of the first K accepted slots in slot order (-1 once they run out), val [B, K] = s[pick]
//     copied (-inf in the tail), kept [B] = min(K, accepted), scanned [B] = the index after the K-th accepted slot, or P.
//
// One workgroup (256 threads) per session, nothing shared between workgroups: a session's result is the same bits in any
// batch.  The pool is walked in chunks of 256 slots, one slot per thread:
//   - a thread resolves its slot once: id -> filled -> category -> counted (filled, 0 <= c < G);
//   - the count of earlier same-category slots INSIDE its wavefront: 64 v_readlane steps, which also give the wavefront's
//     total of the category and its first lane, the LEADER;
//   - the wavefronts then take turns in slot order (a barrier apart): the leader of every category reads the session's
//     counter cnt[c] in LDS (G words, the only ones zeroed) - the count over all earlier slots - advances it by the
//     wavefront's total and hands what it read to its lanes by a shuffle.  No two lanes of a turn touch the same word, so
//     a plain integer read and write do: no atomics at all, a fixed order, nothing left to arrival;
//   - a ballot and the wavefront totals of `accepted` hand out the output positions;
//   - the loop ends (uniformly) with the chunk in which the K-th item is accepted: a list that fills from the first 40
//     slots of a 4096-slot pool costs one chunk.
#include "common.h"

namespace {

constexpr int MAXP = 4096;              // SREC_CAP_MAXP
constexpr int MAXG = 16384;             // SREC_CAP_MAXG
constexpr int CHUNK = 256;
constexpr int STATE_WORDS = 8;          // wtot[2][4]: the wavefronts' accepted counts, by chunk parity

struct CapArgs {
    const int* ids; const float* s;
    int P, K;
    const int* category; long n_items;
    const int* caps; int G;
    int* pick; float* val; int* kept; int* scanned;
};

inline size_t cap_lds(int G) { return (size_t)(STATE_WORDS + G) * 4; }

__global__ __launch_bounds__(CHUNK) void cap_select_kernel(CapArgs a) {
    extern __shared__ __attribute__((aligned(16))) int cap_smem[];
    int* wtot = cap_smem;                                           // [2][4]
    int* cnt = cap_smem + STATE_WORDS;                              // [G] filled slots of category c so far

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = a.P, K = a.K, G = a.G;
    const size_t b = blockIdx.x;
    const int* ids = a.ids + b * (size_t)P;
    const float* s = a.s + b * (size_t)P;
    int* pick = a.pick + b * (size_t)K;
    float* val = a.val + b * (size_t)K;

    for (int i = tid; i < G; i += CHUNK) cnt[i] = 0;
    __syncthreads();

    int n = 0;                                                      // accepted so far (uniform)
    for (int base = 0, par = 0; base < P && n < K; base += CHUNK, par ^= 1) {
        const int slot = base + tid;
        bool filled = false;
        int c = -1;                                                 // the category when it counts, else -1
        if (slot < P) {
            const int id = ids[slot];
            if (id >= 0 && (long)id < a.n_items) {
                filled = true;
                const int x = a.category[id];
                if (x >= 0 && x < G) c = x;
            }
        }
        // inside the wavefront: earlier lanes of my category, all lanes of it, the first of them
        int rank = 0, total = 0, leader = 64;
#pragma unroll 8
        for (int j = 0; j < 64; ++j) {                              // (unrolled by 64 the lane values overflow the SGPRs)
            const bool same = __builtin_amdgcn_readlane(c, j) == c;
            rank += (same && j < lane) ? 1 : 0;
            total += same ? 1 : 0;
            leader = (same && j < leader) ? j : leader;
        }
        bool ok = filled;                                           // (no category: always accepted)
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
                int start = 0;
                if (c >= 0 && leader == lane) {
                    start = cnt[c];
                    cnt[c] = start + total;
                }
                start = __shfl(start, leader & 63, 64);
                if (c >= 0) ok = start + rank < a.caps[c];
                const unsigned long long mk = __ballot(ok);
                if (lane == 0) wtot[par * 4 + w] = __popcll(mk);
                // my position among the accepted of the wavefront
                rank = __popcll(mk & ((1ull << lane) - 1ull));
            }
            __syncthreads();
        }
        int pos = n + rank;
        for (int w = 0; w < wave; ++w) pos += wtot[par * 4 + w];
        if (ok && pos < K) {
            pick[pos] = slot;
            val[pos] = s[slot];
            if (pos == K - 1) a.scanned[b] = slot + 1;
        }
        n += wtot[par * 4] + wtot[par * 4 + 1] + wtot[par * 4 + 2] + wtot[par * 4 + 3];
    }
    for (int t = n + tid; t < K; t += CHUNK) {
        pick[t] = -1;
        val[t] = -INFINITY;
    }
    if (tid == 0) {
        a.kept[b] = n < K ? n : K;
        if (n < K) a.scanned[b] = P;
    }
}

}  // namespace

extern "C" int srec_cap_select(const int* ids, const float* s, int B, int P, int K, const int* category, long n_items,
                               const int* caps, int G, int* pick, float* val, int* kept, int* scanned, void* stream) {
    if (B <= 0) return 0;
    if (P < 1 || P > MAXP || K < 1 || K > P || G < 1 || G > MAXG || n_items < 0 || ids == nullptr || s == nullptr ||
        category == nullptr || caps == nullptr || pick == nullptr || val == nullptr || kept == nullptr || scanned == nullptr ||
        ((uintptr_t)ids & 3) || ((uintptr_t)s & 3) || ((uintptr_t)category & 3) || ((uintptr_t)caps & 3) ||
        ((uintptr_t)pick & 3) || ((uintptr_t)val & 3) || ((uintptr_t)kept & 3) || ((uintptr_t)scanned & 3))
        return SREC_BAD_ARG;
    const CapArgs a{ids, s, P, K, category, n_items, caps, G, pick, val, kept, scanned};
    static std::atomic<unsigned long long> optin{0};                // MAXG counters: 64 KiB + the state needs the opt-in
    if (int rc = srec_lds_optin((const void*)cap_select_kernel, (int)cap_lds(MAXG), optin)) return rc;
    hipLaunchKernelGGL(cap_select_kernel, dim3(B), dim3(CHUNK), cap_lds(G), (hipStream_t)stream, a);
    SREC_LAUNCH_CHECK();
    return 0;
}
