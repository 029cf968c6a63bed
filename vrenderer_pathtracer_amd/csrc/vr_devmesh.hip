// vr_devmesh.hip -- the kernels of the emission stage that need no builder's
// types (gfx950), declared in vr_devmesh_dev.hpp: the node order (the root
// first, the other nodes by descending surface area: a radix sort), the
// per-triangle arrays, and half_directed over an array (vr_devmesh.hpp).
// Nothing depends on the order in which threads or blocks run.
#include <cstring>                                // rocPRIM's iterators call memset without including it
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "vr_devmesh_dev.hpp"

namespace vr {
namespace {

// key: the root first, then descending area (the complement of a non-negative
// float's bits ascends as the float descends), ties by builder node number
__global__ __launch_bounds__(kBlock) void area_keys_kernel(uint32_t n_nodes, uint32_t root,
                                                           const float4* __restrict__ nodebox,
                                                           unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ vals)
{
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= n_nodes) return;
    const DevBox b = load_box(nodebox, id);
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    float area = dx * dy + dy * dz + dz * dx;
    if (!(area >= 0.f)) area = __builtin_inff();  // inf * 0 of an overflowed extent
    const uint32_t inv = ~__float_as_uint(area);
    keys[id] = id == root ? 0ull : ((unsigned long long)inv << 32) | (id + 1u);
    vals[id] = id;
}

__global__ __launch_bounds__(kBlock) void newpos_kernel(uint32_t n_nodes, const uint32_t* __restrict__ order,
                                                        uint32_t* __restrict__ newpos)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n_nodes && order[i] < n_nodes) newpos[order[i]] = i;
}

// one thread per compact triangle, in the builder's final order.  The only
// kernel that follows the caller's indices after validation, so it does
// nothing when a flag is up.
__global__ __launch_bounds__(kBlock) void emit_tris_kernel(TriSource src, const uint32_t* __restrict__ tris,
                                                           uint32_t n_tris, const uint32_t* __restrict__ refs,
                                                           uint32_t n_refs, TriArrays out,
                                                           uint32_t* __restrict__ prim_id, const DevBuildStatus* st)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_refs || st->flags != 0u) return;
    const uint32_t t = refs[k];
    if (t >= n_tris) return;
    prim_id[k] = t;
    const uint32_t vi[3] = { tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2] };
    gather_triangle<true>(src, out, k, vi);
}

__global__ __launch_bounds__(kBlock) void half_box_kernel(const float* __restrict__ in, size_t n,
                                                          uint16_t* __restrict__ down, uint16_t* __restrict__ up)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t u = __float_as_uint(in[i]);
    down[i] = half_directed(u, false);
    up[i] = half_directed(u, true);
}

} // namespace

hipError_t emit_sort_temp_bytes(uint32_t max_nodes, hipStream_t s, size_t& bytes)
{
    return rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                     (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)max_nodes, 0u, 64u, s);
}

hipError_t emit_order(const EmitArgs& a, hipStream_t s)
{
    const EmitScratch& sc = a.scratch;
    area_keys_kernel<<<blocks_for(a.n_nodes), kBlock, 0, s>>>(a.n_nodes, a.root, a.nodebox, sc.keys, sc.vals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = a.temp_bytes;
    e = rocprim::radix_sort_pairs(a.temp, tb, sc.keys, sc.keys_sorted, sc.vals, sc.order, (size_t)a.n_nodes, 0u, 64u, s);
    if (e != hipSuccess) return e;
    newpos_kernel<<<blocks_for(a.n_nodes), kBlock, 0, s>>>(a.n_nodes, sc.order, sc.newpos);
    return hipSuccess;
}

hipError_t emit_tris(const EmitArgs& a, hipStream_t s)
{
    const TriArrays out{ a.out.verts, a.out.tri_e, a.out.normals, a.out.tangents, a.out.uvs, a.out.slot_vert };
    emit_tris_kernel<<<blocks_for(a.n_refs), kBlock, 0, s>>>(a.src, a.tris, a.n_tris, a.refs, a.n_refs, out,
                                                             a.out.prim_id, a.status);
    return hipGetLastError();
}

int launch_half_box(const float* in, size_t n, uint16_t* down, uint16_t* up, void* stream)
{
    if (n == 0) return 0;
    half_box_kernel<<<blocks_for(n), kBlock, 0, (hipStream_t)stream>>>(in, n, down, up);
    return (int)hipGetLastError();
}

} // namespace vr
