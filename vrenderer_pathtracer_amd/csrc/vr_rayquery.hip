// vr_rayquery.hip -- the ray-query kernel (gfx950): the caller's rays through
// the resident mesh with the path kernels' own traversal (vr_kernel.hpp
// traverse_mesh: the while-while walk, fp16 t-culled or fp32 strict, LDS stacks
// and node cache, tri_test_v and its exact equal-t tie-break), instantiated
// here for a ray buffer instead of camera_ray.  See vr_rayquery.hpp.
#include <hip/hip_runtime.h>

#include "vr_kernel.hpp"
#include "vr_rayquery.hpp"

namespace vr {
namespace {

// blocks of kBlockThreads resident per CU at the kernel's launch bounds
// (min_waves(STACK) waves on each of the four SIMDs)
constexpr uint32_t query_blocks_per_cu(int stack) { return (uint32_t)(4 * min_waves(stack) * 64 / kBlockThreads); }

// One ray per lane.  A block fills its node cache once, then each of its waves
// takes 64-ray chunks in a grid-stride loop; a thread's stack column is its
// own, so the waves of a block never meet again after lds_setup.  Lanes past
// the last ray and lanes holding a non-finite ray are classified before the
// walk and stay out of it, as a path kernel's ended lanes stay out of
// traverse_mesh: the walk's ballots count the lanes inside it.
template <int STACK, uint32_t FEAT>
__global__ void __launch_bounds__(kBlockThreads, min_waves(STACK)) ray_query_kernel(const RenderParams p, const RayQuery q)
{
    constexpr int CN = cache_nodes(STACK);
    __shared__ int lds_stack[STACK * kBlockThreads];
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
        r.d = mk4(d[0], d[1], d[2], 0.f);
        const float t0 = q.tmax ? q.tmax[i] : kRayNoHit;
        // false for inf and NaN; a NaN tmax is refused, an infinite one is a bound like any other
        const bool finite = fabsf(r.o.x) <= big && fabsf(r.o.y) <= big && fabsf(r.o.z) <= big &&
                            fabsf(r.d.x) <= big && fabsf(r.d.y) <= big && fabsf(r.d.z) <= big && t0 == t0;
        HitRec hr;
        hr.t = finite ? t0 : kRayNoHit;
        hr.kind = HK_NONE; hr.idx = 0; hr.bu = hr.bv = 0.f; hr.su = hr.sv = 0.f;
        if (finite) {
            Cnt cnt;
            traverse_mesh<STACK, false, FEAT>(p, r, hr, L, cnt, q.any_hit != 0u);
        }
        const bool hit = hr.kind == HK_MESH;
        vr_u32x4 rec;
        if (hit && q.any_hit) {
            rec = vr_u32x4{ 0u, 0u, 0u, 0u };
        } else {
            rec.x = __float_as_uint(hr.t);
            rec.y = hit ? q.prim_id[hr.idx / 3] : kRayMiss;
            rec.z = __float_as_uint(hit ? hr.bu : 0.f);
            rec.w = __float_as_uint(hit ? hr.bv : 0.f);
        }
        reinterpret_cast<vr_u32x4*>(q.hits)[i] = rec;     // one 16-B store per ray
    }
}

template <int STACK, uint32_t FEAT>
void launch_one(const RenderParams& p, const RayQuery& q, uint32_t cu_count, hipStream_t s)
{
    const uint64_t need = ((uint64_t)q.n_rays + kBlockThreads - 1u) / kBlockThreads;
    const uint64_t resident = (uint64_t)(cu_count ? cu_count : 1u) * query_blocks_per_cu(STACK);
    const uint32_t blocks = (uint32_t)(need < resident ? need : resident);
    ray_query_kernel<STACK, FEAT><<<blocks, kBlockThreads, 0, s>>>(p, q);
}

template <uint32_t FEAT>
void launch_stack(const RenderParams& p, const RayQuery& q, int stack, uint32_t cu_count, hipStream_t s)
{
    if (stack <= 16) launch_one<16, FEAT>(p, q, cu_count, s);
    else if (stack <= 24) launch_one<24, FEAT>(p, q, cu_count, s);
    else if (stack <= 32) launch_one<32, FEAT>(p, q, cu_count, s);
    else launch_one<64, FEAT>(p, q, cu_count, s);
}

} // namespace

int launch_ray_query(const RenderParams& p, const RayQuery& q, int stack, uint32_t cu_count, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if ((p.flags & F_STRICT) != 0u) launch_stack<F_MESH | F_EXACT | F_STRICT>(p, q, stack, cu_count, s);
    else launch_stack<F_MESH | F_EXACT>(p, q, stack, cu_count, s);
    return (int)hipGetLastError();
}

} // namespace vr
