// Stand-in for <thrust/random.h>: the engine and the distribution the
// reference's kernel uses, written from Thrust's documented definitions.
// rocThrust's own header cannot be used beside the CUDA stand-in: it includes
// the HIP runtime, whose float4 (and the operators on it) collide with the
// stand-in's vector types.  oracle/ref/rng_kat.cpp checks this file against
// vectors that rocThrust itself produced (tests/golden/rng_kat.json).
#pragma once
#include <cstdint>

namespace thrust
{
namespace random
{
// linear_congruential_engine<UIntType, a, c, m>: x <- (a * x + c) mod m; a
// seed congruent to 0 becomes 1 when c is congruent to 0.
template <typename UIntType, UIntType a, UIntType c, UIntType m> class linear_congruential_engine
{
public:
  typedef UIntType result_type;
  static const result_type multiplier = a;
  static const result_type increment = c;
  static const result_type modulus = m;
  static const result_type min = c == 0u ? 1u : 0u;
  static const result_type max = m - 1u;
  static const result_type default_seed = 1u;
  explicit linear_congruential_engine(result_type s = default_seed) { seed(s); }
  void seed(result_type s = default_seed)
  {
    if(c % m == 0 && s % m == 0)
      m_x = 1 % m;
    else
      m_x = s % m;
  }
  result_type operator()()
  {
    m_x = (result_type)(((uint64_t)a * m_x + c) % m);
    return m_x;
  }
private:
  result_type m_x;
};
typedef linear_congruential_engine<uint32_t, 16807, 0, 2147483647> minstd_rand0;
typedef linear_congruential_engine<uint32_t, 48271, 0, 2147483647> minstd_rand;
typedef minstd_rand default_random_engine;

// uniform_real_distribution<RealType>(a, b): (urng() - min) / (1 + (max - min))
// evaluated in RealType, scaled to [a, b).
template <typename RealType = double> class uniform_real_distribution
{
public:
  typedef RealType result_type;
  explicit uniform_real_distribution(RealType a = 0.0, RealType b = 1.0) : m_a(a), m_b(b) {}
  template <typename Urng> result_type operator()(Urng &urng)
  {
    result_type result = static_cast<result_type>(urng() - Urng::min);
    result /= (result_type(1) + static_cast<result_type>(Urng::max - Urng::min));
    return (result * (m_b - m_a)) + m_a;
  }
private:
  RealType m_a, m_b;
};
}
using random::default_random_engine;
using random::minstd_rand;
using random::minstd_rand0;
using random::uniform_real_distribution;
}
