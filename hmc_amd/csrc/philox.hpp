// philox.hpp — Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC'11), the counter-based generator of the
// posterior draws (hmc_posterior_draws).
//
// A draw's random numbers are a pure function of (seed, individual, draw
// index, step): no generator state is stored anywhere, so the bits cannot
// depend on launch shapes, on the other draws of a call or on sharding.  One
// body serves device code (exact_posterior_draws) and host code (the CPU-side
// test hook hmc_test_draw_uniform), the way select.hpp does it.
#pragma once
#include <cstdint>

#ifndef HMC_HD
#if defined(__HIPCC__)
#define HMC_HD __host__ __device__ __forceinline__
#else
#define HMC_HD inline
#endif
#endif

namespace hmc {

struct Philox4 {
  uint32_t w[4];
};

// Ten rounds; the key is bumped by the Weyl constants between rounds (nine times).
HMC_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// The uniform of one decision of one draw: key = the two halves of the seed
// (low, high), counter = (step, draw index, panel index of the individual, 0);
// u = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53 in [0, 1), 53 random bits.
HMC_HD double draw_uniform(uint64_t seed, uint32_t indiv, uint32_t draw, uint32_t step) {
  const Philox4 x = philox4x32_10(step, draw, indiv, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  return ((double)(x.w[0] >> 5) * 67108864.0 + (double)(x.w[1] >> 6)) * (1.0 / 9007199254740992.0);
}

}  // namespace hmc
