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

// Whether the culled walk may take this ray: whether it returns the strict
// walk's record.  The culled walk's slabs are one fma each over fp16 boxes
// rounded outward, the strict walk's n * inv - o * inv in two roundings over
// the fp32 boxes, so the culled walk tests every triangle the strict one does
// (or has culled it by distance) and some more.  The records are equal as long
// as none of those further triangles is accepted, that is, as long as the
// reference's own walk loses no triangle its triangle test accepts.  It loses
// them by the rounding of its slabs, 2^-23 |inv| max(|o|, |n|) at most, once
// that is no longer small beside the boxes' own width |inv| (hi - lo): the
// three axes' slabs become three roundings of nearly one number and boxes are
// missed at random while the triangle test still accepts.  So the measure is
// the size of the coordinates, the origin's and the mesh's, against the mesh's
// extent, not against each other:
//   - culled_reach is 8 times the root box's largest extent E, and both the
//     origin's and the root box's largest |coordinate| must lie within it: the
//     slab error then stays below 2^-20 E |inv|, a millionth of the mesh.  An
//     origin far outside the mesh fails it, and so does every ray on a small
//     mesh far from zero;
//   - a mesh with a coordinate beyond 65504 has infinite fp16 boxes: the culled
//     walk would be a brute force over them, which finds every triangle the
//     reference loses (and is the slower walk): all its rays walk strictly;
//   - a direction component that is non-zero but within 3e-10: the boxes see
//     the replacement 3e-10, the triangle test the component itself.
// Rays outside these rules take the strict walk inside the culled kernel
// (tests/test_gpu_extreme.py).  Overflow needs no rule: o * inv is
// computed once for both walks, and a plane whose product n * inv overflows
// belongs to a mesh beyond 65504.
// The ray sets of the parity tests stay within 4 E.
// lo, hi: the root's own box.  A negative reach sends every ray strict.
__device__ __forceinline__ float culled_reach(const float lo[3], const float hi[3])
{
    float m = 0.f, e = 0.f;
    for (int a = 0; a < 3; ++a) {
        m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(lo[a]), __builtin_fabsf(hi[a])));
        e = __builtin_fmaxf(e, hi[a] - lo[a]);
    }
    const float reach = 8.f * e;
    return m <= 65504.f && m <= reach ? reach : -1.f;
}
__device__ __forceinline__ bool culled_walk_is_strict(const Ray& r, float reach)
{
    auto axis = [&](float o, float d) {
        const float ad = __builtin_fabsf(d);
        return __builtin_fabsf(o) <= reach && (ad > VR_EPS || ad == 0.f);
    };
    return axis(r.o.x, r.d.x) && axis(r.o.y, r.d.y) && axis(r.o.z, r.d.z);
}

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
    // the root's own box from its child boxes, fp32 (rows: child 0 x y, child 1 x y, both z); wave-uniform
    const vr4 b0 = p.bvh[0], b1 = p.bvh[1], bz = p.bvh[2];
    const float root_lo[3] = { __builtin_fminf(b0.x, b1.x), __builtin_fminf(b0.z, b1.z), __builtin_fminf(bz.x, bz.z) };
    const float root_hi[3] = { __builtin_fmaxf(b0.y, b1.y), __builtin_fmaxf(b0.w, b1.w), __builtin_fmaxf(bz.y, bz.w) };
    const float reach = culled_reach(root_lo, root_hi);
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
            if ((FEAT & F_STRICT) != 0u || culled_walk_is_strict(r, reach)) {
                traverse_mesh<STACK, false, FEAT>(p, r, hr, L, cnt, q.any_hit != 0u);
            } else {
                // the strict walk for these lanes: fp32 nodes from memory (the block's LDS copy holds fp16 nodes)
                Lds Ls = L;
                Ls.n_cached = 0;
                traverse_mesh<STACK, false, FEAT | F_STRICT>(p, r, hr, Ls, cnt, q.any_hit != 0u);
            }
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
