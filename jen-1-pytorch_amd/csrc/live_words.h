// The reserved-word protocol of the persistent kernels (deep_kernel.hip, long_kernel.hip): the data is its own flag.
//
// Every tensor a phase of a launch produces is POISONED before the launch (all bytes 0xFF: jen1_deep_poison, a node of the
// step's graph well ahead of the launch).  A producer stores its results as 8-byte single-copy-atomic write-through words and does
// nothing else: no drain, no arrival counter.  A consumer WAVE loads the vectors it needs with agent-scope (L1-bypassing) loads
// and repeats the loads until none of their 8-byte words is the sentinel: the load that finds the data complete is the load that
// delivers it.  (A finite activation never encodes as four bf16 / two float32 NaNs with all mantissa bits set.)  Measured on
// 256 workgroups (tools/microbench/flagchain.hip): 1.2 - 1.35 us per all-to-all stage against 3.05 us for
// stores -> drain -> counter -> poll -> barrier -> load, the protocol of round 2.  Every spin is bounded: a wave that gives up
// raises the error word (1 + phase), which releases every other waiter; results are garbage then and the host raises.
#pragma once
#include "common.h"

typedef unsigned long long u64;
typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
constexpr u64 POISON = ~0ull;

__device__ __forceinline__ gu64* g64(const void* p) { return (gu64*)(u64)p; }
__device__ __forceinline__ gu32* g32(const void* p) { return (gu32*)(u64)p; }
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---- 8-element vectors through agent-scope (sc1) accesses: data another workgroup produced in THIS launch --------
template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> { u64 d[2]; };
template <> struct Raw8<float> { u64 d[4]; };

// how ld_live reads a word; a translation unit may define it before this header (a timing experiment of that kernel alone)
#ifndef JEN1_LIVE_LOAD
#define JEN1_LIVE_LOAD(p) __hip_atomic_load(p, RLX_AGENT)
#endif
__device__ __forceinline__ void ld_live(Raw8<bf16_t>& r, const bf16_t* p) {
  r.d[0] = JEN1_LIVE_LOAD(g64(p));
  r.d[1] = JEN1_LIVE_LOAD(g64(p) + 1);
}
__device__ __forceinline__ void ld_live(Raw8<float>& r, const float* p) {
#pragma unroll
  for (int i = 0; i < 4; ++i) r.d[i] = JEN1_LIVE_LOAD(g64(p) + i);
}
// the same words of a tensor that was complete before the launch
__device__ __forceinline__ void ld_plain(Raw8<bf16_t>& r, const bf16_t* p) {
  const u32x4 v = *reinterpret_cast<const u32x4*>(p);
  r.d[0] = ((u64)v[1] << 32) | v[0];
  r.d[1] = ((u64)v[3] << 32) | v[2];
}
__device__ __forceinline__ void ld_plain(Raw8<float>& r, const float* p) {
  const u32x4 a = *reinterpret_cast<const u32x4*>(p);
  const u32x4 b = *reinterpret_cast<const u32x4*>(p + 4);
  r.d[0] = ((u64)a[1] << 32) | a[0];
  r.d[1] = ((u64)a[3] << 32) | a[2];
  r.d[2] = ((u64)b[1] << 32) | b[0];
  r.d[3] = ((u64)b[3] << 32) | b[2];
}
__device__ __forceinline__ bool raw_bad(const Raw8<bf16_t>& r) { return (r.d[0] == POISON) | (r.d[1] == POISON); }
__device__ __forceinline__ bool raw_bad(const Raw8<float>& r) {
  return (r.d[0] == POISON) | (r.d[1] == POISON) | (r.d[2] == POISON) | (r.d[3] == POISON);
}
__device__ __forceinline__ void raw_to_float(const Raw8<bf16_t>& r, float (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const unsigned lo = (unsigned)r.d[i], hi = (unsigned)(r.d[i] >> 32);
    o[4 * i + 0] = __uint_as_float(lo << 16);
    o[4 * i + 1] = __uint_as_float(lo & 0xffff0000u);
    o[4 * i + 2] = __uint_as_float(hi << 16);
    o[4 * i + 3] = __uint_as_float(hi & 0xffff0000u);
  }
}
__device__ __forceinline__ void raw_to_float(const Raw8<float>& r, float (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __uint_as_float((unsigned)r.d[i]);
    o[2 * i + 1] = __uint_as_float((unsigned)(r.d[i] >> 32));
  }
}

// 4 consecutive channels (a residual operand) as raw words
template <typename T> struct Raw4;
template <> struct Raw4<bf16_t> { u64 d[1]; };
template <> struct Raw4<float> { u64 d[2]; };
__device__ __forceinline__ void ld_live4r(Raw4<bf16_t>& r, const bf16_t* p) { r.d[0] = __hip_atomic_load(g64(p), RLX_AGENT); }
__device__ __forceinline__ void ld_live4r(Raw4<float>& r, const float* p) {
  r.d[0] = __hip_atomic_load(g64(p), RLX_AGENT);
  r.d[1] = __hip_atomic_load(g64(p) + 1, RLX_AGENT);
}
__device__ __forceinline__ bool raw_bad(const Raw4<bf16_t>& r) { return r.d[0] == POISON; }
__device__ __forceinline__ bool raw_bad(const Raw4<float>& r) { return (r.d[0] == POISON) | (r.d[1] == POISON); }
__device__ __forceinline__ void raw4_to_float(const Raw4<bf16_t>& r, float (&o)[4]) {
  const unsigned lo = (unsigned)r.d[0], hi = (unsigned)(r.d[0] >> 32);
  o[0] = __uint_as_float(lo << 16); o[1] = __uint_as_float(lo & 0xffff0000u);
  o[2] = __uint_as_float(hi << 16); o[3] = __uint_as_float(hi & 0xffff0000u);
}
__device__ __forceinline__ void raw4_to_float(const Raw4<float>& r, float (&o)[4]) {
  o[0] = __uint_as_float((unsigned)r.d[0]); o[1] = __uint_as_float((unsigned)(r.d[0] >> 32));
  o[2] = __uint_as_float((unsigned)r.d[1]); o[3] = __uint_as_float((unsigned)(r.d[1] >> 32));
}

// Reserved word.  The all-ones 8-byte word is RESERVED (it means "not stored yet").  A finite result never encodes as it; four bf16
// (two float32) NaNs with sign and every mantissa bit set would -- e.g. NaN weights whose payload propagates.  Every live store
// therefore breaks exactly that pattern (the lowest payload bit of the word's first element is cleared: still a NaN, no longer
// the sentinel): the consumer sees NaNs, as the reference's consumer would, and no data a producer can compute makes a consumer
// wait (include/jen1_deep.h "Reserved word").  Three vector instructions per store.
// LOC: every reader of the word runs on the XCD of the writer (a sample's group of workgroups on one XCD): a PLAIN store -- the line
// stays in that XCD's L2, where the readers' L1-bypassing polls find it (0.30 us hand-off against 0.47 - 0.60 written through,
// tools/xcd_handoff_probe.hip; a plain store never arrives on ANOTHER XCD before the kernel ends)
template <bool LOC, typename G>
__device__ __forceinline__ void st_word(G* p, int i, unsigned lo, unsigned hi) {
  lo -= ((lo & hi) == 0xffffffffu) ? 1u : 0u;
  if constexpr (LOC) *(g64(p) + i) = ((u64)hi << 32) | lo;
  else __hip_atomic_store(g64(p) + i, ((u64)hi << 32) | lo, RLX_AGENT);
}
// 4 consecutive output channels of one position
template <bool LOC>
__device__ __forceinline__ void st_live4(bf16_t* p, const float (&v)[4]) {
  bf16x4 a;
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = (bf16_t)v[i];
  const u32x2 w = __builtin_bit_cast(u32x2, a);
  st_word<LOC>(p, 0, w[0], w[1]);
}
template <bool LOC>
__device__ __forceinline__ void st_live4(float* p, const float (&v)[4]) {
  st_word<LOC>(p, 0, __float_as_uint(v[0]), __float_as_uint(v[1]));
  st_word<LOC>(p, 1, __float_as_uint(v[2]), __float_as_uint(v[3]));
}

// Behind a round of loads of one wave: `bad` = this lane saw a sentinel word.  Returns true when the wave has to load again
// (wave-uniform; the error word is looked at every 64th failed poll).  SYNC: the kernel's record of the wait -- `err` the error word,
// `dead` this wave: a wait timed out somewhere: stop waiting, finish with whatever is there, `p` the current phase.  LIMIT: failed
// polls of one wait before the wave gives up; SLEEP: s_sleep count (units of 64 clocks) between polls.
template <unsigned LIMIT, int SLEEP, typename SYNC>
__device__ __forceinline__ bool live_poll_again(SYNC& sy, bool bad, unsigned& spins) {
  if (!__builtin_amdgcn_ballot_w64(bad) || sy.dead) return false;
  ++spins;
  if ((spins & 63u) == 0u) {
    const unsigned ev = __hip_atomic_load(g32(sy.err), RLX_AGENT);
    if (rfl((int)ev) != 0) { sy.dead = true; return false; }
  }
  if (spins > LIMIT) {
    if ((threadIdx.x & 63) == 0) __hip_atomic_store(g32(sy.err), (unsigned)(sy.p + 1), RLX_AGENT);
    sy.dead = true;
    return false;
  }
  if constexpr (SLEEP > 0) __builtin_amdgcn_s_sleep(SLEEP);
  return true;
}
