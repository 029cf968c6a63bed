// Prints, from the stand-in engine and distribution (standin/thrust/random.h),
// the known-answer vectors that tests/golden/gen_rng_kat.cpp printed from
// rocThrust itself: the same seeds, pixels and JSON keys, so that a test can
// compare the two documents entry by entry (tests/golden/rng_kat.json).
#include <thrust/random.h>
#include <thrust/random/uniform_real_distribution.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

static uint32_t hashSeeds(uint32_t *s0, uint32_t *s1)
{
  *s0 = 36969u * ((*s0) & 65535u) + ((*s0) >> 16);
  *s1 = 18000u * ((*s1) & 65535u) + ((*s1) >> 16);
  return *s0 * *s1;
}

static void printUniforms(uint32_t seed, int n)
{
  thrust::default_random_engine rng(seed);
  thrust::uniform_real_distribution<float> u(0, 1);
  std::printf("{\"seed\": %u, \"u_bits\": [", seed);
  for(int k = 0; k < n; ++k)
  {
    const float v = u(rng);
    uint32_t b;
    std::memcpy(&b, &v, 4);
    std::printf("%u%s", b, k < n - 1 ? ", " : "");
  }
  std::printf("]}");
}

int main()
{
  const uint32_t seeds[] = { 0u, 1u, 2u, 12345u, 2147483646u, 2147483647u, 2147483648u,
                             4294967295u, 0x88266ba4u, 0xcfc8cb90u, 0x19cbe700u, 0xdeadbeefu };
  const int n = sizeof(seeds) / sizeof(seeds[0]);
  std::printf("{\n  \"engine\": [\n");
  for(int i = 0; i < n; ++i)
  {
    std::printf("    ");
    printUniforms(seeds[i], 8);
    std::printf("%s\n", i < n - 1 ? "," : "");
  }
  std::printf("  ],\n  \"pixel\": [\n");
  const uint32_t px[][4] = { { 100, 50, 1, 12345 }, { 640, 360, 2, 12345 }, { 0, 7, 3, 12345 },
                             { 1279, 719, 7, 1792098289u }, { 511, 0, 4, 99 } };
  const int np = sizeof(px) / sizeof(px[0]);
  for(int i = 0; i < np; ++i)
  {
    uint32_t s0 = px[i][0] * px[i][2], s1 = px[i][1] * px[i][3];
    std::printf("    {\"x\": %u, \"y\": %u, \"frame\": %u, \"time\": %u, \"samples\": [", px[i][0], px[i][1], px[i][2], px[i][3]);
    for(int s = 0; s < 2; ++s)
    {
      printUniforms(hashSeeds(&s0, &s1), 3);
      std::printf("%s", s == 0 ? ", " : "");
    }
    std::printf("]}%s\n", i < np - 1 ? "," : "");
  }
  std::printf("  ]\n}\n");
  return 0;
}
