// vr_radiance_dev.hpp -- device half of vr_radiance.hpp: the radiance query
// kernel and its per-feature-set launchers, included by the translation units
// that instantiate it (vr_radiance*.hip).
#pragma once
#include "vr_kernel.hpp"
#include "vr_radiance.hpp"

namespace vr {

// The per-ray sequence of the radiance query for a valid ray, shared by every
// kernel that enters the path tracer from a caller's ray (ray_radiance_kernel
// below, probe_sh_kernel in vr_probe_dev.hpp): intersect_scene once, the
// shared escape of HDRI scenes, then trace<> per path and the mean in path
// order.  cam is the normalised ray; s1, s2 are left where the last path ends.
template <int STACK, uint32_t FEAT>
__device__ __forceinline__ vr4 radiance_along(const RenderParams& p, const Ray& cam, uint32_t& s1, uint32_t& s2,
                                              const uint32_t n_samples, const float coef, const Lds& L)
{
    Cnt cnt;
    HitRec hr0;
    const bool hit0 = intersect_scene<STACK, false, FEAT>(p, cam, hr0, L, cnt);
    // render_kernel's shared escape: in an HDRI scene a ray that
    // escapes gives every path the first bounce's miss branch, which
    // draws no random number
    const bool shared_miss = !HAS(F_CORNELL) && !hit0;
    vr4 miss_r = mk4(0.f, 0.f, 0.f, 0.f);
    if (shared_miss) {
        PathState ps;
        uint32_t d0 = 0, d1 = 0;
        path_begin(ps, d0, d1);
        Ray r0 = cam;
        (void)bounce_step<false, FEAT>(p, r0, hr0, ps, miss_r, cnt);
    }
    vr4 io = mk4(0.f, 0.f, 0.f, 0.f);
    float last_w = 0.f;
#pragma unroll 1
    for (uint32_t k = 0; k < n_samples; ++k) {
        float depth = 1.f;
        vr4 result = miss_r;
        // a path leaves its seeds one hash on, where the next one starts (:620-622)
        if (!shared_miss) result = trace<STACK, false, FEAT>(p, cam, hr0, hit0, s1, s2, L, cnt, depth);
        io = add4(io, mul4s(result, coef));
        last_w = result.w;
    }
    return mk4(io.x, io.y, io.z, last_w);
}

// The query's validity rule: false for inf and NaN; a zero direction and one
// whose squared length overflows have no unit vector.
__device__ __forceinline__ bool radiance_ray_valid(const vr4 o, const vr4 dv)
{
    const float big = 3.402823466e38f;
    const float dd = dot4(dv, dv);
    return fabsf(o.x) <= big && fabsf(o.y) <= big && fabsf(o.z) <= big &&
           fabsf(dv.x) <= big && fabsf(dv.y) <= big && fabsf(dv.z) <= big && dd > 0.f && dd <= big;
}

// One ray per lane, in ray_query_kernel's shape: a block fills its node cache
// once, then each of its waves takes 64-ray chunks in a grid-stride loop over
// at most one resident set of blocks.  Lanes past the last ray and lanes
// holding an invalid ray are classified before any scene test and stay out
// of intersect_scene and trace: the walk's ballots count the lanes inside it.
// A lane whose paths end early idles until the slowest lane of its wave has
// finished its last path (no path pool for ray buffers: DESIGN.md 4).
template <int STACK, uint32_t FEAT>
__global__ void __launch_bounds__(kBlockThreads, render_waves<FEAT>(STACK))
ray_radiance_kernel(const RenderParams p, const RayRadiance q)
{
    constexpr bool MK = (FEAT & F_MESH) != 0u;           // a kernel that may traverse the mesh
    constexpr int CN = MK ? cache_nodes(STACK) : 1;
    __shared__ int lds_stack[MK ? STACK * kBlockThreads : 1];
    __shared__ vr4 lds_nodes[3 * CN];
    __shared__ int2 lds_idx[CN];
    const int tid = threadIdx.x;
    const Lds L = lds_setup<FEAT>(p, lds_stack, lds_nodes, lds_idx, CN, tid);
    constexpr uint64_t kWaves = kBlockThreads / 64;
    const uint64_t n_chunks = ((uint64_t)q.n_rays + 63u) / 64u;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    const uint64_t lane = (uint64_t)(tid & 63);
    const float coef = 1.f / (float)q.n_samples;
    for (uint64_t chunk = (uint64_t)blockIdx.x * kWaves + (uint64_t)(tid >> 6); chunk < n_chunks; chunk += n_waves) {
        const uint64_t i = chunk * 64u + lane;
        if (i >= (uint64_t)q.n_rays) continue;
        const float* o = q.origins + 3u * i;
        const float* d = q.dirs + 3u * i;
        Ray cam;
        cam.o = mk4(o[0], o[1], o[2], 0.f);
        const vr4 dv = mk4(d[0], d[1], d[2], 0.f);
        uint32_t s1 = q.seeds[2u * i], s2 = q.seeds[2u * i + 1u];
        const bool valid = radiance_ray_valid(cam.o, dv);
        vr4 rec = mk4(0.f, 0.f, 0.f, 0.f);
        if (valid) {
            cam.d = normalize4(dv);                      // the reference's camera ray (:842-844)
            rec = radiance_along<STACK, FEAT>(p, cam, s1, s2, q.n_samples, coef, L);
        }
        q.radiance[i] = rec;                             // one 16-B store per ray
    }
}

// One resident set of blocks at the kernel's launch bounds (render_waves
// waves on each of the four SIMDs), or the blocks the rays need if fewer.
template <int STACK, uint32_t FEAT>
void launch_radiance_one(const RenderParams& p, const RayRadiance& q, uint32_t cu_count, hipStream_t s)
{
    constexpr uint32_t per_cu = (uint32_t)(4 * render_waves<FEAT>(STACK) * 64 / kBlockThreads);
    const uint64_t need = ((uint64_t)q.n_rays + kBlockThreads - 1u) / kBlockThreads;
    const uint64_t resident = (uint64_t)(cu_count ? cu_count : 1u) * per_cu;
    const uint32_t blocks = (uint32_t)(need < resident ? need : resident);
    ray_radiance_kernel<STACK, FEAT><<<blocks, kBlockThreads, 0, s>>>(p, q);
}

// A mesh feature set at every stack size mesh_stack_entries returns.
template <uint32_t FEAT>
void launch_radiance_stack(const RenderParams& p, const RayRadiance& q, int stack, uint32_t cu_count, hipStream_t s)
{
    static_assert((FEAT & F_MESH) != 0u, "sphere sets run at 16 entries and no mesh LDS");
    if (stack <= 16) launch_radiance_one<16, FEAT>(p, q, cu_count, s);
    else if (stack <= 24) launch_radiance_one<24, FEAT>(p, q, cu_count, s);
    else if (stack <= 32) launch_radiance_one<32, FEAT>(p, q, cu_count, s);
    else launch_radiance_one<64, FEAT>(p, q, cu_count, s);
}

// per feature class, one translation unit each
void launch_radiance_cornell_mesh(const RenderParams& p, const RayRadiance& q, int stack, uint32_t cu_count, hipStream_t s);
void launch_radiance_hdri_mesh(const RenderParams& p, const RayRadiance& q, int stack, uint32_t cu_count, hipStream_t s);
void launch_radiance_sphere(const RenderParams& p, const RayRadiance& q, uint32_t cu_count, hipStream_t s);

} // namespace vr
