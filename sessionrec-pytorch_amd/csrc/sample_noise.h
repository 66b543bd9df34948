// The counter-based noise of srec_score_sample (recommend.hip): a pure function of (seed, session key q, global item id),
// the same on the host (srec_sample_uniform, the tests' pin of the stream) and in the kernel.  seed = hi:lo 32-bit words.
//   skey = h32(lo ^ h32(q * 0x9E3779B9 + hi * 0x85EBCA6B + 0x165667B1))       once per session (srec_rng_key's mix)
//   h    = h32(skey ^ (gid * 0x9E3779B1 + 0x7F4A7C15))                         per pair (srec_keep's mix); for a fixed session a
//                                                                              bijection of the 32-bit gid
//   w    = min(fma((float)h, 2^-32, 2^-33), 1 - 2^-24)                         in (0, 1); relative precision kept near 0
//   g    = -log(-log1p(-w))                                                    Gumbel(0, 1), in [-2.82, 22.9], always finite
// All 32 bits and log1p on purpose: the UPPER tail of g decides who wins a draw, and it comes from the SMALL w.  (h >> 8) /
// 2^24 with log(u) would leave it a few dozen levels.  h32 is common.h's srec_hash32 ("lowbias32"), restated here for the host.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SREC_HD __host__ __device__
#else
#define SREC_HD
#endif

SREC_HD inline unsigned srec_sample_h32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
SREC_HD inline unsigned srec_sample_skey(unsigned long long seed, unsigned q) {
    const unsigned lo = (unsigned)seed, hi = (unsigned)(seed >> 32);
    return srec_sample_h32(lo ^ srec_sample_h32(q * 0x9E3779B9u + hi * 0x85EBCA6Bu + 0x165667B1u));
}
SREC_HD inline unsigned srec_sample_hash(unsigned skey, unsigned gid) {
    return srec_sample_h32(skey ^ (gid * 0x9E3779B1u + 0x7F4A7C15u));
}
SREC_HD inline float srec_sample_w(unsigned h) { return fminf(fmaf((float)h, 0x1p-32f, 0x1p-33f), 0x1.fffffep-1f); }
// precise logf / log1pf: this file is never built with fast-math
SREC_HD inline float srec_sample_gumbel(unsigned h) { return -logf(-log1pf(-srec_sample_w(h))); }
