// Host stand-in for the CUDA runtime interface the reference path tracer is
// written against, so that its kernel source compiles as plain C++ and runs
// one emulated thread at a time (oracle/ref/README.md).  It describes a
// third-party interface only; no file of the reference is replaced by it.
//
// Semantics chosen where a host compiler and CUDA differ:
//   * the float overloads CUDA puts in the global namespace (sin, sqrt, fabs,
//     min, max ... on float stay in float) are reproduced here;
//   * min/max on float follow the device instruction: a NaN operand is
//     ignored and -0 orders below +0;
//   * rsqrtf(x) is 1/sqrtf(x), the oracle's choice (CUDA's is an
//     approximation within 2 ulp, so no host build matches it bit for bit);
//   * with -DVRO_REF_PORTABLE, sinf cosf acosf atan2f powf are the portable
//     libm of oracle/vro_math.c instead of the host's.
#pragma once

#include <math.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#ifdef VRO_REF_PORTABLE
extern "C" {
#include "vro_math.h"
}
#endif

#define __device__
#define __host__
#define __global__
#define __constant__
#define __forceinline__ inline

typedef unsigned int uint;

// ---- vector types ----------------------------------------------------------
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct uint2 { unsigned int x, y; };
struct uchar4 { unsigned char x, y, z, w; };
struct uint3 { unsigned int x, y, z; };
struct dim3
{
  unsigned int x, y, z;
  dim3(unsigned int _x = 1, unsigned int _y = 1, unsigned int _z = 1) : x(_x), y(_y), z(_z) {}
};

static inline float2 make_float2(float x, float y) { float2 v = { x, y }; return v; }
static inline float3 make_float3(float x, float y, float z) { float3 v = { x, y, z }; return v; }
static inline float4 make_float4(float x, float y, float z, float w) { float4 v = { x, y, z, w }; return v; }
static inline int2 make_int2(int x, int y) { int2 v = { x, y }; return v; }
static inline uint2 make_uint2(unsigned int x, unsigned int y) { uint2 v = { x, y }; return v; }
static inline uchar4 make_uchar4(unsigned char x, unsigned char y, unsigned char z, unsigned char w)
{
  uchar4 v = { x, y, z, w };
  return v;
}

// ---- the emulated thread's coordinates -------------------------------------
extern thread_local uint3 threadIdx, blockIdx;
extern thread_local dim3 blockDim, gridDim;

// ---- bit casts ---------------------------------------------------------------
static inline int __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
static inline float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }

// ---- global-namespace math as CUDA declares it -------------------------------
// <math.h> of a C++ library already gives ::sin(float), ::sqrt(float),
// ::fabs(float) ... returning float; CUDA adds min/max and rsqrtf.
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
static inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
static inline float min(float a, float b)
{
  if(a != a) return b;
  if(b != b) return a;
  if(a < b) return a;
  if(b < a) return b;
  return std::signbit(a) ? a : b;
}
static inline float max(float a, float b)
{
  if(a != a) return b;
  if(b != b) return a;
  if(a > b) return a;
  if(b > a) return b;
  return std::signbit(a) ? b : a;
}
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }

#ifdef VRO_REF_PORTABLE
// The five libm functions whose host results differ between C libraries.
// A call on a float argument resolves to the portable function whether it is
// spelled sinf(x) or, through CUDA's overload set, sin(x).
static inline float vro_ref_sin(float x) { return vro_p_sinf(x); }
static inline double vro_ref_sin(double x) { return ::sin(x); }
static inline float vro_ref_cos(float x) { return vro_p_cosf(x); }
static inline double vro_ref_cos(double x) { return ::cos(x); }
static inline float vro_ref_acos(float x) { return vro_p_acosf(x); }
static inline double vro_ref_acos(double x) { return ::acos(x); }
static inline float vro_ref_atan2(float y, float x) { return vro_p_atan2f(y, x); }
static inline double vro_ref_atan2(double y, double x) { return ::atan2(y, x); }
static inline float vro_ref_pow(float x, float y) { return vro_p_powf(x, y); }
static inline double vro_ref_pow(double x, double y) { return ::pow(x, y); }
static inline float vro_ref_powf(float x, float y) { return vro_p_powf(x, y); }
// Plain global names, so that a translation unit may add overloads of its
// own to them (as it may to powf).  No standard header may follow this one.
#define sinf vro_p_sinf
#define cosf vro_p_cosf
#define acosf vro_p_acosf
#define atan2f vro_p_atan2f
#define powf vro_ref_powf
#define sin vro_ref_sin
#define cos vro_ref_cos
#define acos vro_ref_acos
#define atan2 vro_ref_atan2
#define pow vro_ref_pow
#endif

// ---- symbols -------------------------------------------------------------------
typedef int cudaError_t;
template <typename T> static inline cudaError_t cudaMemcpyToSymbol(T &sym, const void *src, size_t n)
{
  std::memcpy(&sym, src, n);
  return 0;
}
template <typename T> static inline cudaError_t cudaMemcpyFromSymbol(void *dst, const T &sym, size_t n)
{
  std::memcpy(dst, &sym, n);
  return 0;
}

// ---- linear textures -------------------------------------------------------------
enum cudaTextureReadMode { cudaReadModeElementType = 0 };
struct cudaChannelFormatDesc { int bytes; };
template <typename T> static inline cudaChannelFormatDesc cudaCreateChannelDesc()
{
  cudaChannelFormatDesc d = { (int)sizeof(T) };
  return d;
}
template <typename T, int Dim, cudaTextureReadMode Mode> struct texture
{
  const T *ptr = nullptr;
  size_t count = 0;
};
template <typename T, int Dim, cudaTextureReadMode Mode>
static inline cudaError_t cudaBindTexture(size_t *, texture<T, Dim, Mode> *tex, const void *dev, const cudaChannelFormatDesc *,
                                          size_t bytes)
{
  tex->ptr = static_cast<const T *>(dev);
  tex->count = bytes / sizeof(T);
  return 0;
}
template <typename T, int Dim, cudaTextureReadMode Mode> static inline cudaError_t cudaUnbindTexture(texture<T, Dim, Mode> &tex)
{
  tex.ptr = nullptr;
  tex.count = 0;
  return 0;
}
// A fetch outside the bound range returns zero on the device; here it ends
// the run, so that a fixture can never hold such a value unnoticed.
template <typename T, int Dim, cudaTextureReadMode Mode> static inline T tex1Dfetch(const texture<T, Dim, Mode> &tex, int i)
{
  if(i < 0 || (size_t)i >= tex.count)
  {
    std::fprintf(stderr, "vro_ref: tex1Dfetch index %d outside [0,%zu)\n", i, tex.count);
    std::abort();
  }
  return tex.ptr[i];
}

// ---- surfaces: a handle to a host image ---------------------------------------------
typedef unsigned long long cudaSurfaceObject_t;
namespace vro_ref
{
struct Surface
{
  uchar4 *pixels;
  unsigned int width, height;
};
static inline cudaSurfaceObject_t surfaceHandle(Surface *s) { return (cudaSurfaceObject_t)(uintptr_t)s; }
}
static inline void surf2Dwrite(uchar4 v, cudaSurfaceObject_t surf, int xBytes, int y)
{
  vro_ref::Surface *s = (vro_ref::Surface *)(uintptr_t)surf;
  const unsigned int x = (unsigned int)xBytes / sizeof(uchar4);
  if(x >= s->width || (unsigned int)y >= s->height)
  {
    std::fprintf(stderr, "vro_ref: surf2Dwrite outside the image\n");
    std::abort();
  }
  s->pixels[(size_t)y * s->width + x] = v;
}

// ---- what oracle/ref/rewrite.py turns the two non-C++ constructs into -------------------
namespace vro_ref
{
// kernel<<<grid, block>>>(args): every thread of every block in turn.
template <typename F> static inline void launch(dim3 grid, dim3 block, F body)
{
  gridDim = grid;
  blockDim = block;
  for(unsigned int by = 0; by < grid.y; ++by)
    for(unsigned int bx = 0; bx < grid.x; ++bx)
      for(unsigned int ty = 0; ty < block.y; ++ty)
        for(unsigned int tx = 0; tx < block.x; ++tx)
        {
          blockIdx.x = bx; blockIdx.y = by; blockIdx.z = 0;
          threadIdx.x = tx; threadIdx.y = ty; threadIdx.z = 0;
          body();
        }
}

// asm("<PTX>" : "=r"(out) : "r"(in)...): interprets the PTX text for one lane.
// Known: the SIMD video min/max with a secondary min/max
// (v{min,max}.s32.s32.s32.{min,max} d, a, b, c) and a predicate ballot
// (setp.ge.s32 p, a, 0; vote.ballot.b32 d, p).  With one emulated lane the
// ballot is that lane's own predicate in bit 0: a lane leaves the inner
// traversal loop as soon as it alone holds a leaf.
int ptxInt(const char *text, const int *in, int nIn);
template <typename O, typename... I> static inline void ptx(const char *text, O &out, I... in)
{
  const int v[] = { (int)in... };
  out = (O)ptxInt(text, v, (int)sizeof...(I));
}
}
#define VRO_REF_LAUNCH(kernel, grid, block, ...) vro_ref::launch(grid, block, [&]() { kernel(__VA_ARGS__); })
