// Host check of csrc/sn_ray_index.h (compiled and run by tests/test_ray_index_cpu.py): the ray index the fp32 inference kernel
// computes for the 32 points of a wave -- one multiplication per wave, one carry per lane -- against p / S.
// Covers every S in 1..1024 and a few large ones, every lane, wave starts around multiples of S (small, middle, near 2^32 and at
// the end of the largest point count the launcher accepts).  Prints the number of comparisons; exit status 1 on the first mismatch.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../sinnerf_amd/csrc/sn_ray_index.h"

static long n_checked = 0;

static bool check_wave(uint64_t p_wave, int S, const snr::RayDiv& d) {
  const uint64_t q = snr::wave_ray(p_wave, d.m, d.sh);
  const uint32_t r = snr::wave_rem(p_wave, q, S);
  if (q != p_wave / (uint64_t)S || r != p_wave % (uint64_t)S) {
    std::printf("wave: S=%d p_wave=%llu q=%llu r=%u\n", S, (unsigned long long)p_wave, (unsigned long long)q, r);
    return false;
  }
  for (uint32_t j = 0; j < 32; ++j, ++n_checked) {
    const uint64_t ray = q + snr::lane_carry(r + j, S);
    if (ray != (p_wave + j) / (uint64_t)S) {
      std::printf("lane: S=%d p_wave=%llu j=%u ray=%llu\n", S, (unsigned long long)p_wave, j, (unsigned long long)ray);
      return false;
    }
  }
  return true;
}

int main() {
  const uint64_t last_wave = (uint64_t)(snr::MAX_POINTS - 1) / 32 * 32;        // the last unit of the largest launch
  std::vector<int> sizes;
  for (int S = 1; S <= 1024; ++S) sizes.push_back(S);
  for (int S : {1025, 4095, 4096, 4097, 65535, 65536, 1 << 20, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 2147483646, 2147483647}) sizes.push_back(S);
  for (int S : sizes) {
    const snr::RayDiv d = snr::make_ray_div(S);
    const uint64_t mults[] = {0, 1, 2, 3, 31, 32, 33, 1000, (1ull << 32) / (uint64_t)S, last_wave / (uint64_t)S / 2, last_wave / (uint64_t)S};
    for (uint64_t k : mults)
      for (int off = -96; off <= 96; off += 32) {                              // wave starts around k S
        const int64_t p = (int64_t)(k * (uint64_t)S / 32 * 32) + off;
        if (p < 0 || (uint64_t)p > last_wave) continue;
        if (!check_wave((uint64_t)p, S, d)) return 1;
      }
    for (uint64_t p = 0; p < 4096 && p <= last_wave; p += 32)                  // the first units, all of them
      if (!check_wave(p, S, d)) return 1;
    if (!check_wave(last_wave, S, d)) return 1;
  }
  std::printf("ray index: %ld comparisons equal p / S\n", n_checked);
  return 0;
}
