/*
 * sample_noise.h — the noise of temperature sampling (sampling.hip: Gumbel-max), written once and compiled twice: as
 * __device__ code into the sampler kernels and as host code behind the wht_sample_* entries of ktest.cpp, so that a test
 * can ask for any hash and any uniform without a launch (tests/sampling_oracle.py restates them bit for bit).
 *
 *   h = sample_hash(seed_lo, seed_hi, step, row, token)      counter based: no generator state
 *   u = sample_uniform_of_hash(h)                            uses the top SAMPLE_UNIFORM_BITS bits of h
 *   g = -log(-log u)                                         standard Gumbel noise; the key of an entry is x / T + g
 *
 * u = (n + 0.5) * 2^-23 with n = h >> 9 < 2^23: n + 0.5 = (2n + 1) / 2 has a 24-bit numerator and the scaling is by a
 * power of two, so every step is exact in fp32, u is strictly increasing in n and lies in [2^-24, 1 - 2^-24].  Hence
 * -log(-log u) is finite for every h: about [-2.81, 16.64].
 * (A 24-bit n does not do: for n >= 2^23 the sum n + 0.5 is not representable and rounds to even, at n = 2^24 - 1 to 2^24,
 * which gives u == 1.0f, g = +inf and an entry that is drawn whatever its logit is.  Adding 2^-25 after the scaling, or
 * in an fmaf, rounds to 1.0f at the top in the same way.)
 */
#ifndef WH_SAMPLE_NOISE_H
#define WH_SAMPLE_NOISE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SAMPLE_FN __host__ __device__ static inline
#else
#define SAMPLE_FN static inline
#endif

enum { SAMPLE_UNIFORM_BITS = 23 };     /* the bits of a hash the uniform uses: its top ones */

SAMPLE_FN uint32_t sample_fmix32(uint32_t h) {       /* the finaliser of MurmurHash3 */
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

SAMPLE_FN uint32_t sample_hash(uint32_t seed_lo, uint32_t seed_hi, int step, int row, int token) {
  uint32_t h = sample_fmix32((uint32_t)row * 0x9E3779B1u + (uint32_t)step) ^ seed_lo;
  h = sample_fmix32(h ^ (uint32_t)token * 0x85EBCA77u);
  return sample_fmix32(h + seed_hi);
}

SAMPLE_FN float sample_uniform_of_hash(uint32_t h) {
  return ((float)(h >> (32 - SAMPLE_UNIFORM_BITS)) + 0.5f) * (1.0f / (float)(1u << SAMPLE_UNIFORM_BITS));
}

#endif
