/* Stand-in for <hip/hip_runtime.h> (written for this repository) that lets a
 * host compiler read vrenderer_pathtracer_amd/csrc/vr_math.hpp in its
 * VR_DK_HOISTED form (tests/libm_host.cpp, tests/test_libm_cpu.py): empty
 * qualifiers, the bit casts, a one-lane __ballot, the two amdgcn builtins as
 * the IEEE operations, and the constant-pinning asm removed. */
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#define __device__
#define __forceinline__ inline

static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline long long __double_as_longlong(double d) { long long u; memcpy(&u, &d, 8); return u; }
static inline double __longlong_as_double(long long u) { double d; memcpy(&d, &u, 8); return d; }

#define __ballot(x) ((x) ? 1ull : 0ull)
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#define __builtin_amdgcn_sqrtf(x) sqrtf(x)

/* asm volatile("" : "+s"(c)) has no host meaning: both words expand to nothing */
#define asm
#define volatile(...)
