// vr_probe.hip -- the probe query (vr_probe.hpp): the dispatch over the
// feature sets, as launch_ray_radiance picks the radiance kernels', the
// generic set (kFeatAll), the sum of the block partials and the irradiance
// kernel.
#include <hip/hip_runtime.h>

#include "vr_probe_dev.hpp"

namespace vr {

// Word w of probe i: +0 plus its block partials in ascending block order (the
// last word is the count of valid rays, added as uint32).  One word per lane,
// 28 consecutive lanes per probe.
__global__ void __launch_bounds__(256)
probe_sum_kernel(const float* __restrict__ partials, uint32_t n_blocks, uint64_t n_words, float* __restrict__ sh)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= n_words) return;
    const uint64_t i = g / kProbeWords;
    const uint32_t w = (uint32_t)(g - i * kProbeWords);
    const float* src = partials + i * n_blocks * kProbeWords + w;
    if (w == kProbeWords - 1u) {
        uint32_t n = 0u;
        for (uint32_t b = 0; b < n_blocks; ++b) n += __float_as_uint(src[(uint64_t)b * kProbeWords]);
        sh[g] = __uint_as_float(n);
    } else {
        float acc = 0.f;
        for (uint32_t b = 0; b < n_blocks; ++b) acc = acc + src[(uint64_t)b * kProbeWords];
        sh[g] = acc;
    }
}

int launch_probe_sh(const RenderParams& p, const ProbeSH& q, int stack, uint32_t cu_count, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cls = feature_class(p.flags & kFeatAll);
    if (cls == kClassCornellMesh) launch_probe_cornell_mesh(p, q, stack, cu_count, s);
    else if (cls == kClassHdriMesh) launch_probe_hdri_mesh(p, q, stack, cu_count, s);
    else if (cls == kClassCornellSphere || cls == kClassHdriSphere) launch_probe_sphere(p, q, cu_count, s);
    else launch_probe_stack<kFeatAll>(p, q, (p.flags & F_MESH) != 0u ? stack : 16, cu_count, s);
    int e = (int)hipGetLastError();
    const uint32_t n_blocks = probe_blocks(q.n_dirs);
    if (e == 0 && n_blocks > 1u) {
        const uint64_t n_words = (uint64_t)q.n_probes * kProbeWords;
        probe_sum_kernel<<<(uint32_t)((n_words + 255u) / 256u), 256, 0, s>>>(q.partials, n_blocks, n_words, q.sh);
        e = (int)hipGetLastError();
    }
    return e;
}

// One output per lane (include/vrhip.h): the nine band products in fp32, left
// to right in j, every product and sum rounded on its own.
__global__ void __launch_bounds__(256)
sh_irradiance_kernel(const SHIrradiance q)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= q.n) return;
    const uint32_t pi = q.index ? q.index[g] : g;
    vr4 out = mk4(0.f, 0.f, 0.f, 0.f);
    if (pi < q.m) {
        const float* nrm = q.normals + 3ull * g;
        const float x = nrm[0], y = nrm[1], z = nrm[2];
        const float Y[9] = { 0.282094792f, 0.488602512f * y, 0.488602512f * z, 0.488602512f * x,
                             1.09254843f * (x * y), 1.09254843f * (y * z),
                             0.315391565f * (3.f * (z * z) - 1.f), 1.09254843f * (x * z),
                             0.546274215f * (x * x - y * y) };
        const float A[9] = { 3.14159274f, 2.09439516f, 2.09439516f, 2.09439516f,
                             0.785398185f, 0.785398185f, 0.785398185f, 0.785398185f, 0.785398185f };
        const float* sh = q.sh + (uint64_t)kProbeWords * pi;
        float e[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = A[0] * (sh[c] * Y[0]);
#pragma unroll
            for (int j = 1; j < 9; ++j) acc = acc + A[j] * (sh[3 * j + c] * Y[j]);
            e[c] = acc;
        }
        out = mk4(e[0], e[1], e[2], 0.f);
    }
    q.out[g] = out;
}

int launch_sh_irradiance(const SHIrradiance& q, void* stream)
{
    sh_irradiance_kernel<<<(q.n + 255u) / 256u, 256, 0, (hipStream_t)stream>>>(q);
    return (int)hipGetLastError();
}

} // namespace vr
