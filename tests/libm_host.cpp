// libm_host.cpp -- vr_math.hpp compiled for the host in its VR_DK_HOISTED form
// behind tests/stubs/hip/hip_runtime.h, with the function codes of
// vrhip_selftest_math: an edit to the header is compared with the oracle
// (tests/test_libm_cpu.py) before a GPU sees it.  Built with -ffp-contract=off.
#define VR_DK_HOISTED 1
#include "vr_math.hpp"
#include <stddef.h>

extern "C" int vrmath_batch(int fn, const float* a, const float* b, float* out, size_t n)
{
    using namespace vr;
    for (size_t i = 0; i < n; ++i) {
        float s, c, r = 0.f;
        switch (fn) {
        case 0: sincos_p(a[i], &s, &c); r = s; break;
        case 1: sincos_p(a[i], &s, &c); r = c; break;
        case 2: r = acos_p(a[i]); break;
        case 3: r = atan2_p(a[i], b[i]); break;
        case 4: r = pow_p(a[i], b[i]); break;
        case 7: r = bitsf((uint32_t)f2i(a[i])); break;
        case 8: r = bitsf((uint32_t)d2i((double)a[i] * (double)b[i])); break;
        case 9: r = (float)f2u8(a[i]); break;
        case 10: r = sqrt_exact(a[i]); break;
        case 11: r = inv_sqrt_exact(a[i]); break;
        default: return -1;
        }
        out[i] = r;
    }
    return 0;
}
