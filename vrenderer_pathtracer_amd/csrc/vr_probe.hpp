// vr_probe.hpp -- probe radiance projected onto spherical harmonics
// (vrhip_probe_sh) and the irradiance those coefficients give at a normal
// (vrhip_sh_irradiance): the launchers, plain C++ for the host half.  The
// kernel (vr_probe_dev.hpp) is a third entry into the path tracer next to
// ray_radiance_kernel: ray (i, k) = (points[i], dirs[k]) runs the radiance
// query's own per-ray sequence (vr_radiance_dev.hpp radiance_along), and one
// wave per (probe, block of 64 directions) forms the 27 terms of its lanes and
// adds them in the fixed tree of include/vrhip.h.  No buffer of
// n_probes * n_dirs elements exists: with more than one block per probe the
// waves write block partials (probe_scratch_bytes) that a second small kernel
// adds in ascending block order.  No reference counterpart as a call.
// Instantiated per feature set in vr_probe.hip (the generic set, the dispatch,
// the partial sum and the irradiance kernel) and
// vr_probe_{cornell_mesh,hdri_mesh,sphere}.hip, split as vr_radiance*.hip are.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vr_params.hpp"

namespace vr {

constexpr uint32_t kProbeBlock = 64;         // VRHIP_PROBE_BLOCK: the directions one wave reduces
constexpr uint32_t kProbeWords = 28;         // 9 coefficients x rgb, then the count of valid rays
constexpr uint32_t kProbeMaxDirs = 65536;

inline uint32_t probe_blocks(uint32_t n_dirs) { return (n_dirs + kProbeBlock - 1u) / kProbeBlock; }
// The block partials of a call: none when a probe has one block.
inline size_t probe_scratch_bytes(uint32_t n_probes, uint32_t n_dirs)
{
    const uint32_t nb = probe_blocks(n_dirs);
    return nb > 1u ? (size_t)n_probes * nb * (kProbeWords * sizeof(float)) : 0u;
}

// One launch of the probe kernel; every pointer is a device pointer.
struct ProbeSH {
    const float* points;         // float[3 n_probes], used as given
    const float* dirs;           // float[3 n_dirs], shared by all probes, normalised by the kernel
    const float* weights;        // float[n_dirs], or null: every direction weighs w_default
    const uint32_t* probe_seeds; // uint32[2 n_probes]
    const uint32_t* dir_seeds;   // uint32[2 n_dirs]: ray (i, k) starts from probe_seeds[i] ^ dir_seeds[k]
    uint32_t n_probes, n_dirs;   // n_dirs 1..kProbeMaxDirs
    uint32_t n_samples;          // paths per ray, 1..kRadianceMaxSamples
    float w_default;             // 12.566370614f / (float)n_dirs
    float* partials;             // probe_scratch_bytes(n_probes, n_dirs), 16-byte aligned; unused with one block
    float* sh;                   // [28 n_probes], 16-byte aligned
};

// p, stack, cu_count, stream: as launch_ray_radiance.  n_probes > 0.
int launch_probe_sh(const RenderParams& p, const ProbeSH& q, int stack, uint32_t cu_count, void* stream);

// One launch of the irradiance kernel: out[q] from record index ? index[q] : q.
struct SHIrradiance {
    const float* sh;             // [28 m]
    uint32_t m;
    const uint32_t* index;       // uint32[n] or null
    const float* normals;        // float[3 n], used as given
    uint32_t n;
    vr4* out;                    // [n], 16-byte aligned
};
int launch_sh_irradiance(const SHIrradiance& q, void* stream);   // n > 0

} // namespace vr
