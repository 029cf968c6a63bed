// vr_surface_dev.hpp -- device half of vr_surface.hpp: the surface query
// kernel and its per-feature-set launchers, included by the translation units
// that instantiate it (vr_surface*.hip).
#pragma once
#include "vr_kernel.hpp"
#include "vr_rayquery.hpp"
#include "vr_surface.hpp"

namespace vr {

static_assert(kSurfNone == (uint32_t)HK_NONE && kSurfCornell == (uint32_t)HK_CORNELL && kSurfSmall == (uint32_t)HK_SMALL &&
                  kSurfExample == (uint32_t)HK_EXAMPLE && kSurfMesh == (uint32_t)HK_MESH, "kind is written as HitKind");

__device__ __forceinline__ vr_u32x4 surface_row(const vr4& v, float w)
{
    return vr_u32x4{ __float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(w) };
}

// The interpolated texture coordinates of a mesh hit of the triangle at compact
// slot a: fill_hit's interpolated uv, the same operations on the same operands.
__device__ __forceinline__ void surface_mesh_uv(const RenderParams& p, int a, float bu, float bv, float& tu, float& tv)
{
    const float b0 = 1.f - bu - bv;
    const vr2 uv0 = p.uvs[a], uv1 = p.uvs[a + 1], uv2 = p.uvs[a + 2];
    tu = (b0 * uv0.x + bu * uv1.x) + bv * uv2.x;
    tv = (b0 * uv0.y + bu * uv1.y) + bv * uv2.y;
}

// The seven rows of a hit's record (vrhip_surface_hit), and row 0 of a miss,
// whose other rows are zero: the one place the layout is written, for the ray
// query below and the ray-less ones (vr_atlas.hip).
__device__ __forceinline__ void surface_hit_rows(float t, uint32_t kind, uint32_t prim, const Hit& h, float bu, float bv,
                                                 float tu, float tv, vr_u32x4& w0, vr_u32x4& w1, vr_u32x4& w2,
                                                 vr_u32x4& w3, vr_u32x4& w4, vr_u32x4& w5, vr_u32x4& w6)
{
    w0 = vr_u32x4{ __float_as_uint(t), kind, prim, h.type };
    w1 = surface_row(h.hp, bu);
    w2 = surface_row(h.n, bv);
    w3 = surface_row(h.tan, 0.f);
    w4 = surface_row(h.col, tu);
    w5 = surface_row(h.spec, tv);
    w6 = surface_row(h.em, 0.f);
}
__device__ __forceinline__ vr_u32x4 surface_miss_row()
{
    return vr_u32x4{ __float_as_uint(kRayNoHit), (uint32_t)HK_NONE, kRayMiss, 0u };
}

// One ray per lane, in ray_radiance_kernel's shape: a block fills its node
// cache once, then each of its waves takes 64-ray chunks in a grid-stride loop
// over at most one resident set of blocks.  Lanes past the last ray and lanes
// holding an invalid ray are classified before any scene test and stay out of
// intersect_scene: the walk's ballots count the lanes inside it.  An invalid
// ray in range still writes its record, 28 zero words.
template <int STACK, uint32_t FEAT>
__global__ void __launch_bounds__(kBlockThreads, render_waves<FEAT>(STACK))
ray_surface_kernel(const RenderParams p, const RaySurface q)
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
    const float big = 3.402823466e38f;
    for (uint64_t chunk = (uint64_t)blockIdx.x * kWaves + (uint64_t)(tid >> 6); chunk < n_chunks; chunk += n_waves) {
        const uint64_t i = chunk * 64u + lane;
        if (i >= (uint64_t)q.n_rays) continue;
        const float* o = q.origins + 3u * i;
        const float* d = q.dirs + 3u * i;
        Ray r;
        r.o = mk4(o[0], o[1], o[2], 0.f);
        const vr4 dv = mk4(d[0], d[1], d[2], 0.f);
        const float dd = dot4(dv, dv);
        // the radiance query's rule: false for inf and NaN; a zero direction and one whose squared length overflows have no unit vector
        const bool valid = fabsf(r.o.x) <= big && fabsf(r.o.y) <= big && fabsf(r.o.z) <= big &&
                           fabsf(dv.x) <= big && fabsf(dv.y) <= big && fabsf(dv.z) <= big && dd > 0.f && dd <= big;
        const vr_u32x4 zero = vr_u32x4{ 0u, 0u, 0u, 0u };
        vr_u32x4 w0 = zero, w1 = zero, w2 = zero, w3 = zero, w4 = zero, w5 = zero, w6 = zero;
        if (valid) {
            r.d = normalize4(dv);                        // the reference's camera ray (:842-844)
            Cnt cnt;
            HitRec hr;
            if (intersect_scene<STACK, false, FEAT>(p, r, hr, L, cnt)) {
                Hit h;
                fill_hit<FEAT>(p, r, hr, h);             // what bounce 0 of trace sees
                uint32_t prim = (uint32_t)hr.idx;
                float bu = 0.f, bv = 0.f, tu = 0.f, tv = 0.f;
                if (hr.kind == HK_MESH) {
                    const int a = hr.idx;
                    prim = q.prim_id[a / 3];
                    bu = hr.bu; bv = hr.bv;
                    surface_mesh_uv(p, a, bu, bv, tu, tv);
                }
                surface_hit_rows(hr.t, (uint32_t)hr.kind, prim, h, bu, bv, tu, tv, w0, w1, w2, w3, w4, w5, w6);
            } else {
                w0 = surface_miss_row();
            }
        }
        vr_u32x4* rec = reinterpret_cast<vr_u32x4*>(q.hits + i);     // seven 16-B stores per ray
        rec[0] = w0; rec[1] = w1; rec[2] = w2; rec[3] = w3; rec[4] = w4; rec[5] = w5; rec[6] = w6;
    }
}

// One resident set of blocks at the kernel's launch bounds (render_waves
// waves on each of the four SIMDs), or the blocks the rays need if fewer.
template <int STACK, uint32_t FEAT>
void launch_surface_one(const RenderParams& p, const RaySurface& q, uint32_t cu_count, hipStream_t s)
{
    constexpr uint32_t per_cu = (uint32_t)(4 * render_waves<FEAT>(STACK) * 64 / kBlockThreads);
    const uint64_t need = ((uint64_t)q.n_rays + kBlockThreads - 1u) / kBlockThreads;
    const uint64_t resident = (uint64_t)(cu_count ? cu_count : 1u) * per_cu;
    const uint32_t blocks = (uint32_t)(need < resident ? need : resident);
    ray_surface_kernel<STACK, FEAT><<<blocks, kBlockThreads, 0, s>>>(p, q);
}

// A mesh feature set at every stack size mesh_stack_entries returns.
template <uint32_t FEAT>
void launch_surface_stack(const RenderParams& p, const RaySurface& q, int stack, uint32_t cu_count, hipStream_t s)
{
    static_assert((FEAT & F_MESH) != 0u, "sphere sets run at 16 entries and no mesh LDS");
    if (stack <= 16) launch_surface_one<16, FEAT>(p, q, cu_count, s);
    else if (stack <= 24) launch_surface_one<24, FEAT>(p, q, cu_count, s);
    else if (stack <= 32) launch_surface_one<32, FEAT>(p, q, cu_count, s);
    else launch_surface_one<64, FEAT>(p, q, cu_count, s);
}

// per feature class, one translation unit each
void launch_surface_cornell_mesh(const RenderParams& p, const RaySurface& q, int stack, uint32_t cu_count, hipStream_t s);
void launch_surface_hdri_mesh(const RenderParams& p, const RaySurface& q, int stack, uint32_t cu_count, hipStream_t s);
void launch_surface_sphere(const RenderParams& p, const RaySurface& q, uint32_t cu_count, hipStream_t s);

} // namespace vr
