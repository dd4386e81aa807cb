// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the word -> uniform mapping of the
// seeded draw (decode.hip).  Counter based: every output is a pure function of (counter, key), so the kernel and the host entry
// gill_decode_uniforms compute the same words from the same code, and no generator state lives anywhere.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GILL_HD __host__ __device__ __forceinline__
#else
#define GILL_HD inline
#endif

struct Philox4 {
  uint32_t w[4];
};

GILL_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;     // round multipliers
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;     // key increments (golden ratio, sqrt(3) - 1)
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kM0 * c0, p1 = (uint64_t)kM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kW0;
    k1 += kW1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// The 23 high bits of a word to the odd multiples of 2^-24: exact in fp32, symmetric about 1/2, never 0 and never 1 (so
// -log(u) is finite and positive).
GILL_HD float philox_uniform(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * 5.9604644775390625e-8f; }

// The uniform of column c in the draw's stream: counter (c >> 2, row, draw, 0), key (seed low, seed high), output word c & 3.
GILL_HD float decode_uniform(uint64_t seed, uint32_t row, uint32_t draw, uint32_t c) {
  const Philox4 p = philox4x32_10(c >> 2, row, draw, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t lo = c & 1 ? p.w[1] : p.w[0], hi = c & 1 ? p.w[3] : p.w[2];    // selects, not an indexed read: registers on the device
  return philox_uniform(c & 2 ? hi : lo);
}
