// srec_personal_merge: the top-K of a session's ORDERED pool after a sparse per-session list of items changed its scores -
// "never show these", "lift what is in the cart" - WITHOUT a dense [B, V] bias and without another catalogue pass.  If M
// items of a session change their value, the new top-K is the top-K of (the pool without those items) and (those items with
// their new values): everything here is integer logic on 64-bit keys, the values are copied or formed by ONE fp32 add.
//   pool slot i of session b: pool_ids[b, i] (FILLED iff >= 0) and pool_s[b, i], the filled ones in served order (value
//     descending, id ascending), unfilled ones anywhere;
//   list slot j: items[b, j] (FILLED iff >= 0; an id met again in a later slot is ignored), t_j = base[b, j] + bias[b, j]
//     (bias == NULL: -inf); a CANDIDATE iff t_j > -inf;
//   a filled pool slot SURVIVES iff its id is in no filled list slot; hit[b] = the filled pool slots that do not;
//   the first K of survivors and candidates by (value descending, id ascending) go out: ids_out, val_out (the pool's bits or
//     t_j), src (pool slot i, or P + j for list slot j), the tail (-1, -inf, -1); kept[b] = the filled output slots.
//
// One workgroup (256 threads) per session, nothing shared between workgroups: a session's result is the same bits in any
// batch.  No atomics, no workspace.
//   1. the list's (id << 32 | slot) pairs are sorted in LDS (bitonic, a power of two of at most 1024 keys, unfilled slots as
//      all-ones at the end); an entry whose id equals its predecessor's is a repeat;
//   2. the first occurrences with t > -inf become the candidate keys ~key_of(t) << 32 | id (score_key.h, the order key of
//      select_many.hip's order kernel), everything else all-ones, and the same network sorts them: nc candidates in order;
//   3. the pool is walked in chunks of 256 slots, one per thread: membership by binary search in the sorted list, a ballot
//      and the wavefronts' totals (double-buffered by chunk parity: one barrier per chunk) compact the survivors in slot
//      order; the first K are kept as (key, slot).  The whole pool is walked: hit counts every slot of it;
//   4. survivor i lands at i + (candidates ahead of it), candidate j at j + (survivors ahead of it), both by binary search;
//      ids are distinct between the two sets, so the keys are and the positions are a bijection.  A slot is written when
//      its position is below K: nothing is written out of bounds whatever the pool's order or the list holds.
// LDS: 16 bytes per list key (two arrays) and 10 per kept survivor: 56 KB at M = 1024, K = 4096.
#include "common.h"
#include "score_key.h"

namespace {

using score_tile::key_of;
typedef unsigned long long u64;

constexpr int MAXP = 4096;              // SREC_CAP_MAXP
constexpr int MAXM = 1024;              // SREC_PERSONAL_MAXM
constexpr int CHUNK = 256;
constexpr u64 NONE = ~0ull;

struct PersonalArgs {
    const int* pool_ids; const float* pool_s;
    int P;
    const int* items; const float* base; const float* bias;
    int M, M2, K;                       // M2: M rounded up to a power of two
    int* ids_out; float* val_out; int* src; int* hit; int* kept;
};

inline int pow2_of(int m) {
    int m2 = 1;
    while (m2 < m) m2 <<= 1;
    return m2;
}

// the survivors kept: min(K, P)
inline size_t personal_lds(int M2, int keep) { return (size_t)M2 * 16 + (size_t)keep * 8 + (((size_t)keep * 2 + 15) & ~(size_t)15) + 64; }

// the number of keys below `key` among the n ascending keys of a
__device__ __forceinline__ int keys_below(const u64* a, int n, u64 key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void sort_keys(u64* keys, int m2, int tid) {
    for (int k = 2; k <= m2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (m2 >> 1); t += CHUNK) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const u64 x = keys[i], y = keys[p];
                if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[p] = x; }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(CHUNK) void personal_merge_kernel(PersonalArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 personal_smem[];
    const int P = a.P, M = a.M, M2 = a.M2, K = a.K;
    const int keep = K < P ? K : P;
    u64* lkey = personal_smem;                                      // [M2] id << 32 | list slot, ascending
    u64* ckey = lkey + M2;                                          // [M2] ~key_of(t) << 32 | id, ascending
    u64* skey = ckey + M2;                                          // [keep] the survivors' keys, in pool order
    unsigned short* sslot = reinterpret_cast<unsigned short*>(skey + keep);                        // [keep] their pool slots
    int* wtot = reinterpret_cast<int*>(reinterpret_cast<char*>(sslot) + (((size_t)keep * 2 + 15) & ~(size_t)15));  // [2][4]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t b = blockIdx.x;
    const int* pool_ids = a.pool_ids + b * (size_t)P;
    const float* pool_s = a.pool_s + b * (size_t)P;
    const int* items = a.items + b * (size_t)M;
    const float* base = a.base + b * (size_t)M;
    const float* bias = a.bias != nullptr ? a.bias + b * (size_t)M : nullptr;
    int* ids_out = a.ids_out + b * (size_t)K;
    float* val_out = a.val_out + b * (size_t)K;
    int* src = a.src != nullptr ? a.src + b * (size_t)K : nullptr;

    // 1. the list by (id, slot); unfilled slots and the padding last
    for (int i = tid; i < M2; i += CHUNK) {
        const int id = i < M ? items[i] : -1;
        lkey[i] = id >= 0 ? ((u64)(unsigned)id << 32) | (u64)(unsigned)i : NONE;
    }
    __syncthreads();
    sort_keys(lkey, M2, tid);
    const int nl = keys_below(lkey, M2, 1ull << 63);                // filled list slots (uniform)

    // 2. the candidates by (value descending, id ascending)
    for (int i = tid; i < M2; i += CHUNK) {
        u64 key = NONE;
        if (i < nl) {
            const u64 e = lkey[i];
            const unsigned id = (unsigned)(e >> 32);
            const bool first = i == 0 || (unsigned)(lkey[i - 1] >> 32) != id;
            const int slot = (int)(unsigned)e;
            const float t = bias != nullptr ? base[slot] + bias[slot] : -INFINITY;
            if (first && t > -INFINITY) key = ((u64)~key_of(t) << 32) | (u64)id;
        }
        ckey[i] = key;
    }
    __syncthreads();
    sort_keys(ckey, M2, tid);
    const int nc = keys_below(ckey, M2, NONE);                      // candidates (uniform)

    // 3. the pool's survivors in slot order, the first `keep` of them kept
    int n = 0, nh = 0;                                              // survivors, hits so far (uniform)
    for (int c0 = 0, par = 0; c0 < P; c0 += CHUNK, par ^= 1) {
        const int slot = c0 + tid;
        int id = -1;
        if (slot < P) id = pool_ids[slot];
        bool listed = false;
        if (id >= 0) {
            const int at = keys_below(lkey, nl, (u64)(unsigned)id << 32);
            listed = at < nl && (unsigned)(lkey[at] >> 32) == (unsigned)id;
        }
        const bool surv = id >= 0 && !listed;
        const u64 ms = __ballot(surv), mh = __ballot(listed);
        if (lane == 0) wtot[par * 4 + wave] = __popcll(ms) | (__popcll(mh) << 16);
        __syncthreads();
        int pos = n + __popcll(ms & ((1ull << lane) - 1ull));
        for (int w = 0; w < 4; ++w) {
            const int t = wtot[par * 4 + w];
            if (w < wave) pos += t & 0xffff;
            n += t & 0xffff;
            nh += t >> 16;
        }
        if (surv && pos < keep) {
            skey[pos] = ((u64)~key_of(pool_s[slot]) << 32) | (u64)(unsigned)id;
            sslot[pos] = (unsigned short)slot;
        }
    }
    __syncthreads();
    const int ns = n < keep ? n : keep;

    // 4. every survivor and every candidate to its place
    for (int i = tid; i < ns; i += CHUNK) {
        const u64 key = skey[i];
        const int pos = i + keys_below(ckey, nc, key);
        if (pos < K) {
            const int slot = sslot[i];
            ids_out[pos] = (int)(unsigned)key;
            val_out[pos] = pool_s[slot];
            if (src != nullptr) src[pos] = slot;
        }
    }
    for (int j = tid; j < nc; j += CHUNK) {
        const u64 key = ckey[j];
        const int pos = j + keys_below(skey, ns, key);
        if (pos < K) {
            const unsigned id = (unsigned)key;
            const int slot = (int)(unsigned)lkey[keys_below(lkey, nl, (u64)id << 32)];   // (its first occurrence: in the list)
            ids_out[pos] = (int)id;
            val_out[pos] = base[slot] + bias[slot];                 // (nc > 0 only with a bias)
            if (src != nullptr) src[pos] = P + slot;
        }
    }
    const int total = ns + nc < K ? ns + nc : K;
    for (int r = total + tid; r < K; r += CHUNK) {
        ids_out[r] = -1;
        val_out[r] = -INFINITY;
        if (src != nullptr) src[r] = -1;
    }
    if (tid == 0) {
        a.hit[b] = nh;
        a.kept[b] = total;
    }
}

}  // namespace

extern "C" int srec_personal_merge(const int* pool_ids, const float* pool_s, int B, int P, const int* items, const float* base,
                                   const float* bias, int M, int K, int* ids_out, float* val_out, int* src, int* hit, int* kept,
                                   void* stream) {
    if (B <= 0) return 0;
    if (P < 1 || P > MAXP || M < 1 || M > MAXM || K < 1 || K > MAXP || pool_ids == nullptr || pool_s == nullptr ||
        items == nullptr || base == nullptr || ids_out == nullptr || val_out == nullptr || hit == nullptr || kept == nullptr ||
        ((uintptr_t)pool_ids & 3) || ((uintptr_t)pool_s & 3) || ((uintptr_t)items & 3) || ((uintptr_t)base & 3) ||
        ((uintptr_t)bias & 3) || ((uintptr_t)ids_out & 3) || ((uintptr_t)val_out & 3) || ((uintptr_t)src & 3) ||
        ((uintptr_t)hit & 3) || ((uintptr_t)kept & 3))
        return SREC_BAD_ARG;
    const int M2 = pow2_of(M);
    const PersonalArgs a{pool_ids, pool_s, P, items, base, bias, M, M2, K, ids_out, val_out, src, hit, kept};
    hipLaunchKernelGGL(personal_merge_kernel, dim3(B), dim3(CHUNK), personal_lds(M2, K < P ? K : P), (hipStream_t)stream, a);
    SREC_LAUNCH_CHECK();
    return 0;
}
