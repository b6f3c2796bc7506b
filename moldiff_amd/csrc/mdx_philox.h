// Philox4x32-10 (Salmon et al., SC'11): the counter-based generator of the sampler's noise (mdx_transition.hip: philox_noise_kernel)
// and of the embedding's starting coordinates (mdx_embed.hip).  Integer arithmetic only; tests/philox_ref.py and moldiff_amd/embed.py
// restate it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct u4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u4 philox4x32_10(u4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    u4 n = {hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    c = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
