// vr_selftest_hoisted.hip -- the libm cases of vrhip_selftest_math in the
// hoistable constant form of vr_math.hpp (VR_DK_HOISTED, as the sphere-only
// translation units compile it; selftest_math_kernel in vr_kernel.hip runs
// the per-use form).  A copy of that kernel's cases 0..4, same thread mapping.
#define VR_DK_HOISTED 1
#include "vr_math.hpp"
#include "vr_params.hpp"

namespace vr {

__global__ void selftest_math_hoisted_kernel(int fn, const float* a, const float* b, float* out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s, c, r = 0.f;
    switch (fn) {
    case 0: sincos_p(a[i], &s, &c); r = s; break;
    case 1: sincos_p(a[i], &s, &c); r = c; break;
    case 2: r = acos_p(a[i]); break;
    case 3: r = atan2_p(a[i], b[i]); break;
    case 4: r = pow_p(a[i], b[i]); break;
    default: r = 0.f;
    }
    out[i] = r;
}

int launch_selftest_math_hoisted(int fn, const float* a, const float* b, float* out, size_t n, void* stream)
{
    if (n == 0) return 0;
    if (fn < 0 || fn > 4) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(selftest_math_hoisted_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, fn, a, b, out, n);
    return (int)hipGetLastError();
}

} // namespace vr
