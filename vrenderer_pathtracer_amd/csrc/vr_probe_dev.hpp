// vr_probe_dev.hpp -- device half of vr_probe.hpp: the probe kernel and its
// per-feature-set launchers, included by the translation units that
// instantiate it (vr_probe*.hip).
#pragma once
#include "vr_probe.hpp"
#include "vr_radiance_dev.hpp"

namespace vr {

// The fixed tree of include/vrhip.h over the wave's 64 slots:
// for s in 32, 16, 8, 4, 2, 1: for l < s: v[l] = v[l] + v[l + s].  Every lane
// runs every step; a lane at or above s adds something no later step reads, so
// lane 0 ends with the tree's root.  Called with the whole wave active.
__device__ __forceinline__ float probe_tree(float v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = v + __shfl_down(v, s, 64);
    return v;
}

// One wave per (probe, block of 64 directions), in ray_radiance_kernel's
// shape: a block fills its node cache once, then each of its waves takes
// (probe, block) items in a grid-stride loop over at most one resident set of
// blocks; the item is the same in every lane of a wave, so the wave reaches
// the reduction whole.  Lane l holds direction 64 b + l.  Lanes past
// the last direction and lanes holding an invalid ray are classified before
// any scene test and stay out of intersect_scene and trace (the walk's ballots
// count the lanes inside it); their 27 terms are +0.  The terms are formed
// after the lane's last trace has returned, so they are not live across it.
// Lane 0 writes the 28 words as seven 16-byte rows: with one block per probe
// 0 + partial straight to the record, otherwise the partial to the scratch
// that probe_sum_kernel adds up.
template <int STACK, uint32_t FEAT>
__global__ void __launch_bounds__(kBlockThreads, render_waves<FEAT>(STACK))
probe_sh_kernel(const RenderParams p, const ProbeSH q)
{
    constexpr bool MK = (FEAT & F_MESH) != 0u;           // a kernel that may traverse the mesh
    constexpr int CN = MK ? cache_nodes(STACK) : 1;
    __shared__ int lds_stack[MK ? STACK * kBlockThreads : 1];
    __shared__ vr4 lds_nodes[3 * CN];
    __shared__ int2 lds_idx[CN];
    const int tid = threadIdx.x;
    const Lds L = lds_setup<FEAT>(p, lds_stack, lds_nodes, lds_idx, CN, tid);
    constexpr uint32_t kWaves = kBlockThreads / 64;
    const uint32_t n_blocks = (q.n_dirs + kProbeBlock - 1u) / kProbeBlock;
    // item = probe * n_blocks + block, advanced by the grid's waves without a
    // division: the launcher's grid is at most one resident set, far below 2^32 waves
    const uint32_t n_waves = gridDim.x * kWaves;
    const uint32_t step_i = n_waves / n_blocks, step_b = n_waves % n_blocks;
    // the wave's index is the same in its 64 lanes: held as a scalar, so are the item and all that follows from it
    const uint32_t first = blockIdx.x * kWaves + (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const float coef = 1.f / (float)q.n_samples;
    uint64_t i = first / n_blocks;
    uint32_t b = first % n_blocks;
    while (i < (uint64_t)q.n_probes) {
        float t[27];
#pragma unroll
        for (int j = 0; j < 27; ++j) t[j] = 0.f;
        bool valid = false;
        {
            const uint32_t k = b * kProbeBlock + (uint32_t)(tid & 63);
            if (k < q.n_dirs) {
                const float* o = q.points + 3u * i;
                const float* d = q.dirs + 3u * k;
                Ray cam;
                cam.o = mk4(o[0], o[1], o[2], 0.f);
                const vr4 dv = mk4(d[0], d[1], d[2], 0.f);
                uint32_t s1 = q.probe_seeds[2u * i] ^ q.dir_seeds[2u * k];
                uint32_t s2 = q.probe_seeds[2u * i + 1u] ^ q.dir_seeds[2u * k + 1u];
                valid = radiance_ray_valid(cam.o, dv);
                if (valid) {
                    cam.d = normalize4(dv);              // the reference's camera ray (:842-844)
                    const vr4 rec = radiance_along<STACK, FEAT>(p, cam, s1, s2, q.n_samples, coef, L);
                    // the weight is read here, after the last trace, so that it is not live across the walk
                    const float w = q.weights ? q.weights[b * kProbeBlock + (uint32_t)(tid & 63)] : q.w_default;
                    const float x = cam.d.x, y = cam.d.y, z = cam.d.z;
                    const float Y[9] = { 0.282094792f, 0.488602512f * y, 0.488602512f * z, 0.488602512f * x,
                                         1.09254843f * (x * y), 1.09254843f * (y * z),
                                         0.315391565f * (3.f * (z * z) - 1.f), 1.09254843f * (x * z),
                                         0.546274215f * (x * x - y * y) };
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        const float wy = w * Y[j];
                        t[3 * j] = wy * rec.x; t[3 * j + 1] = wy * rec.y; t[3 * j + 2] = wy * rec.z;
                    }
                }
            }
        }
        const uint32_t count = (uint32_t)__popcll(__ballot(valid));
#pragma unroll
        for (int j = 0; j < 27; ++j) t[j] = probe_tree(t[j]);
        if ((tid & 63) == 0) {
            vr4* row;
            if (n_blocks == 1u) {
                // the sum over blocks starts from +0: a partial of -0 becomes +0
#pragma unroll
                for (int j = 0; j < 27; ++j) t[j] = 0.f + t[j];
                row = (vr4*)(q.sh + (uint64_t)kProbeWords * i);
            } else {
                row = (vr4*)(q.partials + (uint64_t)kProbeWords * (i * n_blocks + b));
            }
#pragma unroll
            for (int r = 0; r < 6; ++r) row[r] = mk4(t[4 * r], t[4 * r + 1], t[4 * r + 2], t[4 * r + 3]);
            row[6] = mk4(t[24], t[25], t[26], __uint_as_float(count));
        }
        i += step_i;
        b += step_b;
        if (b >= n_blocks) { b -= n_blocks; ++i; }
    }
}

// One resident set of blocks at the kernel's launch bounds (render_waves
// waves on each of the four SIMDs), or the blocks the items need if fewer.
template <int STACK, uint32_t FEAT>
void launch_probe_one(const RenderParams& p, const ProbeSH& q, uint32_t cu_count, hipStream_t s)
{
    constexpr uint32_t per_cu = (uint32_t)(4 * render_waves<FEAT>(STACK) * 64 / kBlockThreads);
    constexpr uint64_t kWaves = kBlockThreads / 64;
    const uint64_t need = ((uint64_t)q.n_probes * probe_blocks(q.n_dirs) + kWaves - 1u) / kWaves;
    const uint64_t resident = (uint64_t)(cu_count ? cu_count : 1u) * per_cu;
    const uint32_t blocks = (uint32_t)(need < resident ? need : resident);
    probe_sh_kernel<STACK, FEAT><<<blocks, kBlockThreads, 0, s>>>(p, q);
}

// A mesh feature set at every stack size mesh_stack_entries returns.
template <uint32_t FEAT>
void launch_probe_stack(const RenderParams& p, const ProbeSH& q, int stack, uint32_t cu_count, hipStream_t s)
{
    static_assert((FEAT & F_MESH) != 0u, "sphere sets run at 16 entries and no mesh LDS");
    if (stack <= 16) launch_probe_one<16, FEAT>(p, q, cu_count, s);
    else if (stack <= 24) launch_probe_one<24, FEAT>(p, q, cu_count, s);
    else if (stack <= 32) launch_probe_one<32, FEAT>(p, q, cu_count, s);
    else launch_probe_one<64, FEAT>(p, q, cu_count, s);
}

// per feature class, one translation unit each
void launch_probe_cornell_mesh(const RenderParams& p, const ProbeSH& q, int stack, uint32_t cu_count, hipStream_t s);
void launch_probe_hdri_mesh(const RenderParams& p, const ProbeSH& q, int stack, uint32_t cu_count, hipStream_t s);
void launch_probe_sphere(const RenderParams& p, const ProbeSH& q, uint32_t cu_count, hipStream_t s);

} // namespace vr
