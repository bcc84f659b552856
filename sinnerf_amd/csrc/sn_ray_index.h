// sn_ray_index.h -- the ray index p / S of the 32 consecutive points of a wave without a per-lane 64-bit division (host and device).
//
// A wave's points are p_wave + j, j = 0..31, p_wave a multiple of 32 and wave-uniform.  Their ray is
//     ray(p_wave + j) = q + carry(r + j),   q = p_wave / S,   r = p_wave % S   (both wave-uniform: integer SALU work, free beside the MFMAs)
// with q by multiplication: for every n < 2^DIVIDEND_BITS and 1 <= S < 2^31, with l = ceil(log2 S) and m = floor(2^(DIVIDEND_BITS + l) / S) + 1,
//     floor(n / S) = floor(n m / 2^(DIVIDEND_BITS + l))
// (Granlund & Montgomery 1994, theorem 4.2: 2^(N+l) <= m S <= 2^(N+l) + 2^l, here m S - 2^(N+l) = S - (2^(N+l) mod S) in [1, S]).
// m < 2^(DIVIDEND_BITS + 1) + 1 fits 64 bits; the product takes 128.  The carry of a lane is (r + j) / S: one compare for S >= 32 (r + j < 2 S),
// a 32-bit division of a number below 63 for the short rays.  tests/test_ray_index_cpu.py checks all of it against p / S.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SN_RAY_HD __host__ __device__ inline
#else
#define SN_RAY_HD inline
#endif

namespace snr {

constexpr int DIVIDEND_BITS = 40;
// the largest point count the kernels built on this accept: 2^31 - 1 units of 32 points (unit tickets are 32-bit words)
constexpr long MAX_POINTS = ((1L << 31) - 1) * 32;
static_assert(MAX_POINTS + 32 < (1L << DIVIDEND_BITS), "every p_wave is a valid dividend");

struct RayDiv {
  uint64_t m;      // multiplier
  uint32_t sh;     // shift of the 128-bit product
};

// host side, once per launch; S in [1, 2^31)
inline RayDiv make_ray_div(int S) {
  int l = 0;
  while ((1L << l) < (long)S) ++l;
  RayDiv d;
  d.sh = (uint32_t)(DIVIDEND_BITS + l);
  d.m = (uint64_t)((((unsigned __int128)1) << d.sh) / (unsigned)S) + 1;
  return d;
}

// q = p_wave / S
SN_RAY_HD uint64_t wave_ray(uint64_t p_wave, uint64_t m, uint32_t sh) {
  return (uint64_t)((((unsigned __int128)p_wave) * m) >> sh);
}
// r = p_wave % S (below 2^31: the low words decide)
SN_RAY_HD uint32_t wave_rem(uint64_t p_wave, uint64_t q, int S) { return (uint32_t)p_wave - (uint32_t)q * (uint32_t)S; }
// (r + j) / S for j <= 31
SN_RAY_HD uint32_t lane_carry(uint32_t r_plus_j, int S) {
  return S >= 32 ? (r_plus_j >= (uint32_t)S ? 1u : 0u) : r_plus_j / (uint32_t)S;
}

}  // namespace snr
