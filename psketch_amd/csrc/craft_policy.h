// craft_policy.h — the policy head (include/craft.h "The head rule"): a slot's action chosen from
// its six logits inside the tick, the first maximum (CRAFT_HEAD_ARGMAX) or a draw from the softmax
// keyed by (seed, global env id, tick) (CRAFT_HEAD_SAMPLE).  One device function for the tile
// kernel's MODE_TICK_HEAD / MODE_STREAM_HEAD / MODE_LANG_HEAD / MODE_LANG_STREAM_HEAD, tick2_kernel's
// head instantiations and craft_policy_actions' own small kernel; and the ask rule ("The ask
// rule": policy_ask, craft_policy_ask's kernel).  craft_cpu.cpp keeps its own copy on purpose
// (craft_episode.h says why); the two must agree bit for bit, so everything here is +, *, explicit
// fmaf, rintf, comparisons and integer bit operations (and, in the ask rule, one IEEE division):
// nothing a compiler may contract or approximate differently.
#pragma once
#include "craft_device.h"

namespace craft {

// A slot's row: 24 bytes at an 8-byte aligned address, as three 8-byte loads the caller issues
// in its batch (no result is used here).
struct LogitRow {
  float2 a, b, c;
};
__device__ __forceinline__ LogitRow load_logit_row(const float* logits, int64_t slot) {
  const float2* p = reinterpret_cast<const float2*>(logits + 6 * slot);
  LogitRow r;
  r.a = p[0];
  r.b = p[1];
  r.c = p[2];
  return r;
}

// e^x for -80 <= x <= 0 (craft.h): range reduction by ln 2 in two pieces, a degree-6 Horner
// polynomial, the exponent added to the bits.  Within 2^-21 relative of exp (measured: 8.9e-8).
__device__ __forceinline__ float craft_expf(float x) {
  const float k = rintf(x * __uint_as_float(0x3FB8AA3Bu));
  float r = fmaf(k, __uint_as_float(0xBF317200u), x);
  r = fmaf(k, __uint_as_float(0xB5BFBE8Eu), r);
  float p = __uint_as_float(0x3AB566C5u);
  p = fmaf(p, r, __uint_as_float(0x3C0936C6u));
  p = fmaf(p, r, __uint_as_float(0x3D2AAC3Fu));
  p = fmaf(p, r, __uint_as_float(0x3E2AAA05u));
  p = fmaf(p, r, __uint_as_float(0x3EFFFFFDu));
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  return __uint_as_float(__float_as_uint(p) + ((uint32_t)(int32_t)k << 23));
}

// The head of the slot with global id `gid` at `tick`: 0..5, or -1 for a row with a NaN or +inf
// or nothing but -inf.  mode, seed and tick by reference: kernel-argument words read where used.
__device__ __forceinline__ int policy_head(const LogitRow& row, const int32_t& mode, const uint64_t& seed,
                                           uint64_t gid, const int64_t& tick) {
  const float l[6] = {row.a.x, row.a.y, row.b.x, row.b.y, row.c.x, row.c.y};
  const float inf = __uint_as_float(0x7F800000u);
  bool bad = !(l[0] < inf);
  float m = l[0];
#pragma unroll
  for (int k = 1; k < 6; ++k) {
    bad = bad || !(l[k] < inf);
    m = (l[k] > m) ? l[k] : m;
  }
  if (bad || m == -inf) return -1;
  int act = 5;
  if (mode == CRAFT_HEAD_ARGMAX) {
#pragma unroll
    for (int k = 4; k >= 0; --k) act = (l[k] == m) ? k : act;
    return act;
  }
  const uint64_t h = splitmix64(seed ^ (gid << 20) ^ (uint64_t)tick);
  const float u = (float)(uint32_t)(h >> 40) * __uint_as_float(0x33800000u);   // 2^-24
  float w[6], c[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float d = l[k] - m;
    w[k] = (l[k] == -inf) ? 0.0f : craft_expf(d > -80.0f ? d : -80.0f);
    c[k] = k == 0 ? w[0] : c[k - 1] + w[k];
  }
  const float thr = u * c[5];
  int last = 0;
  act = -1;
#pragma unroll
  for (int k = 5; k >= 0; --k) act = (c[k] > thr) ? k : act;       // the smallest such k
#pragma unroll
  for (int k = 1; k < 6; ++k) last = (w[k] > 0.0f) ? k : last;     // the largest k with weight
  return act < 0 ? last : act;
}

// The ask rule (include/craft.h "The ask rule"): 1 where the entropy of softmax(row), over ln 6,
// exceeds `threshold` (0 <= threshold <= 1), 0 otherwise and for a row the head calls bad.  No log:
// H = ln S - A / S > T is decided as S > e^(T + A / S), with craft_expf on whichever side keeps its
// argument in [-80, 0].  The division is IEEE's (__fdiv_rn), the one operation here a fast-math
// build could approximate.
__device__ __forceinline__ int policy_ask(const LogitRow& row, float threshold) {
  const float l[6] = {row.a.x, row.a.y, row.b.x, row.b.y, row.c.x, row.c.y};
  const float inf = __uint_as_float(0x7F800000u);
  bool bad = !(l[0] < inf);
  float m = l[0];
#pragma unroll
  for (int k = 1; k < 6; ++k) {
    bad = bad || !(l[k] < inf);
    m = (l[k] > m) ? l[k] : m;
  }
  if (bad || m == -inf) return 0;
  float S = 0.0f, A = 0.0f;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float d = l[k] - m;
    const float dk = d > -80.0f ? d : -80.0f;
    const bool masked = l[k] == -inf;
    const float w = masked ? 0.0f : craft_expf(dk);
    S = k == 0 ? w : S + w;
    A = masked ? A : fmaf(w, dk, A);
  }
  // (a product feeding a sum: __fmul_rn / __fadd_rn keep the two roundings the rule has)
  const float T = __fmul_rn(threshold, __uint_as_float(0x3FE55860u));      // ln 6
  const float x = __fadd_rn(T, __fdiv_rn(A, S));
  if (!(x > 0.0f)) return S > craft_expf(x > -80.0f ? x : -80.0f) ? 1 : 0;
  return S * craft_expf(-x) > 1.0f ? 1 : 0;
}

}  // namespace craft
