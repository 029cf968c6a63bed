// vr_refit.hip -- refit of a device-built mesh and the tree's SAH cost
// (gfx950), declared in vr_refit.hpp.
//
// The tree keeps its topology; only what depends on the vertex positions is
// rewritten, over the arrays the render kernels read:
//   1. a read-only pass over the positions behind the compact slots (flags
//      into the status record, as the builders' validation);
//   2. one thread per compact triangle gathers its vertices through
//      slot_vert and writes verts and tri_e (normals, tangents where given);
//   3. the boxes, one launch per level of the emitted node array, deepest
//      first: a leaf child's box from its triangles' new vertices, an inner
//      child's box from the two boxes in that child's row, which an earlier
//      launch has already rewritten.  A thread writes its own row only.
// Kernel boundaries order every read after the write it needs, so no
// workgroup waits for another and no result depends on scheduling (the only
// atomic is the OR of the validation flags).
#include <hip/hip_runtime.h>

#include "vr_devmesh_dev.hpp"

namespace vr {
namespace {

// the union of the two child boxes in a node's row: the node's own box
__device__ __forceinline__ DevBox own_box(const float4* bvh, size_t node)
{
    const float4 r0 = bvh[4 * node], r1 = bvh[4 * node + 1], r2 = bvh[4 * node + 2];
    return { { fminf(r0.x, r1.x), fminf(r0.z, r1.z), fminf(r2.x, r2.z) },
             { fmaxf(r0.y, r1.y), fmaxf(r0.w, r1.w), fmaxf(r2.y, r2.w) } };
}

// ---- the level of every node ---------------------------------------------------
__global__ __launch_bounds__(kBlock) void refit_level_kernel(const float4* __restrict__ bvh, uint32_t n_nodes,
                                                             uint32_t d, uint32_t* level)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_nodes) return;
    if (d == 0u) {                                // level[] comes filled with ~0: only the root's thread goes on
        if (i != 0u) return;
        level[0] = 0u;
    } else if (level[i] != d) {
        return;
    }
    const float4 r3 = bvh[4 * (size_t)i + 3];
    const int32_t c[2] = { __float_as_int(r3.x), __float_as_int(r3.y) };
    for (int ch = 0; ch < 2; ++ch)
        if (c[ch] > 0 && (uint32_t)c[ch] / 4u < n_nodes) level[(uint32_t)c[ch] / 4u] = d + 1u;
}

// ---- 1. validation ----------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void refit_validate_kernel(const float* __restrict__ pos, uint32_t n_verts,
                                                                const uint32_t* __restrict__ slot_vert, size_t n_slots,
                                                                DevBuildStatus* st)
{
    const size_t s = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_slots) return;
    const uint32_t v = slot_vert[s];
    uint32_t flags = 0u;
    if (v >= n_verts) flags = DEVBVH_BAD_INDEX;
    else if (!finite3(pos[3 * (size_t)v], pos[3 * (size_t)v + 1], pos[3 * (size_t)v + 2])) flags = DEVBVH_NONFINITE;
    if (flags) atomicOr(&st->flags, flags);
}

// ---- 2. triangles -----------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void refit_tris_kernel(const float* __restrict__ pos, const float* __restrict__ nrm,
                                                            const float* __restrict__ tan,
                                                            const uint32_t* __restrict__ slot_vert, uint32_t n_refs,
                                                            vr3* __restrict__ verts, vr3* __restrict__ tri_e,
                                                            vr4* __restrict__ normals, vr4* __restrict__ tangents)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_refs) return;
    const uint32_t vi[3] = { slot_vert[3 * (size_t)k], slot_vert[3 * (size_t)k + 1], slot_vert[3 * (size_t)k + 2] };
    gather_triangle<false>(TriSource{ pos, nrm, tan, nullptr }, TriArrays{ verts, tri_e, normals, tangents, nullptr, nullptr },
                           k, vi);
}

// ---- 3. boxes, one launch per level -------------------------------------------------
// bvh is read (the children's rows, one level down) and written (the thread's
// own row) in the same launch: never the same row, so no restrict on it
__global__ __launch_bounds__(kBlock) void refit_boxes_kernel(uint32_t n_nodes, uint32_t n_refs, uint32_t d,
                                                             const uint32_t* __restrict__ level,
                                                             const vr3* __restrict__ verts, float4* bvh,
                                                             uint4* __restrict__ bvh16)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_nodes || level[i] != d) return;
    const float4 r3 = bvh[4 * (size_t)i + 3];
    const int32_t c[2] = { __float_as_int(r3.x), __float_as_int(r3.y) };
    DevBox b[2];
    for (int ch = 0; ch < 2; ++ch) {
        if (c[ch] < 0) {
            uint32_t first, count;
            leaf_range(c[ch], first, count);
            if (count == 0u || (size_t)first + count > n_refs) return;     // not a tree the builders emit
            b[ch] = empty_box();
            for (size_t s = 3 * (size_t)first; s < 3 * ((size_t)first + count); ++s) {
                const vr3 p = verts[s];
                grow_fminmax(b[ch], p.x, p.y, p.z);
            }
        } else {
            const uint32_t j = (uint32_t)c[ch] / 4u;
            if (j == 0u || j >= n_nodes) return;
            b[ch] = own_box(bvh, j);
        }
    }
    write_node_rows<false>(bvh, bvh16, i, b[0], b[1], c[0], c[1]);       // the index row stays
}

// ---- SAH cost -----------------------------------------------------------------------
__device__ __forceinline__ double area64(const float lo[3], const float hi[3])
{
    const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1],
                 dz = (double)hi[2] - (double)lo[2];
    return dx * dy + dy * dz + dz * dx;
}

// sum of the block's pairs in a fixed order, valid in thread 0
__device__ __forceinline__ Sum2 block_sum(Sum2 v)
{
    __shared__ double part_hi[kBlock], part_lo[kBlock];
    part_hi[threadIdx.x] = v.hi;
    part_lo[threadIdx.x] = v.lo;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            Sum2 a{ part_hi[threadIdx.x], part_lo[threadIdx.x] };
            sum2_add(a, part_hi[threadIdx.x + o], part_lo[threadIdx.x + o]);
            part_hi[threadIdx.x] = a.hi;
            part_lo[threadIdx.x] = a.lo;
        }
        __syncthreads();
    }
    return Sum2{ part_hi[0], part_lo[0] };
}

// per node: the area of its own box, and of each leaf child's box once per
// triangle; partial[2 b], partial[2 b + 1]: block b's pair
__global__ __launch_bounds__(kBlock) void refit_cost_kernel(const float4* __restrict__ bvh, uint32_t n_nodes,
                                                            double* __restrict__ partial)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    Sum2 term;
    if (i < n_nodes) {
        const float4 r0 = bvh[4 * (size_t)i], r1 = bvh[4 * (size_t)i + 1], r2 = bvh[4 * (size_t)i + 2],
                     r3 = bvh[4 * (size_t)i + 3];
        const float lo[2][3] = { { r0.x, r0.z, r2.x }, { r1.x, r1.z, r2.z } };
        const float hi[2][3] = { { r0.y, r0.w, r2.y }, { r1.y, r1.w, r2.w } };
        const DevBox own = own_box(bvh, i);
        sum2_add(term, area64(own.lo, own.hi));
        const int32_t c[2] = { __float_as_int(r3.x), __float_as_int(r3.y) };
        for (int ch = 0; ch < 2; ++ch) {
            if (c[ch] >= 0) continue;
            uint32_t first, count;
            leaf_range(c[ch], first, count);
            sum2_add(term, area64(lo[ch], hi[ch]) * (double)count);
        }
    }
    term = block_sum(term);
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = term.hi;
        partial[2 * (size_t)blockIdx.x + 1] = term.lo;
    }
}

__global__ __launch_bounds__(kBlock) void refit_cost_final_kernel(const float4* __restrict__ bvh,
                                                                  const double* __restrict__ partial,
                                                                  uint32_t n_partial, double* __restrict__ cost)
{
    Sum2 sum;
    for (uint32_t i = threadIdx.x; i < n_partial; i += kBlock) sum2_add(sum, partial[2 * (size_t)i], partial[2 * (size_t)i + 1]);
    sum = block_sum(sum);
    if (threadIdx.x != 0) return;
    const DevBox root = own_box(bvh, 0);
    const double a = area64(root.lo, root.hi);
    *cost = a > 0.0 && a < (double)__builtin_inff() ? sum.hi / a : (double)__builtin_inff();
}

} // namespace

int refit_levels(const vr4* bvh, uint32_t n_nodes, uint32_t depth, uint32_t* level, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(level, 0xff, (size_t)n_nodes * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    // launch d marks the nodes of level d + 1; the deepest level, depth - 1, has no inner children
    for (uint32_t d = 0; d == 0u || d + 1u < depth; ++d)
        refit_level_kernel<<<blocks_for(n_nodes), kBlock, 0, s>>>((const float4*)bvh, n_nodes, d, level);
    return (int)hipGetLastError();
}

int refit_validate(const float* positions, uint32_t n_verts, const MeshArrays& m, DevBuildStatus* st, void* stream)
{
    const size_t n_slots = 3 * (size_t)m.n_refs;
    refit_validate_kernel<<<blocks_for(n_slots), kBlock, 0, (hipStream_t)stream>>>(positions, n_verts, m.slot_vert,
                                                                                   n_slots, st);
    return (int)hipGetLastError();
}

int refit_apply(const float* positions, const float* normals, const float* tangents, const MeshArrays& m, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    refit_tris_kernel<<<blocks_for(m.n_refs), kBlock, 0, s>>>(positions, normals, tangents, m.slot_vert, m.n_refs,
                                                              m.verts, m.tri_e, m.normals, m.tangents);
    for (uint32_t d = m.depth; d-- > 0u;)
        refit_boxes_kernel<<<blocks_for(m.n_nodes), kBlock, 0, s>>>(m.n_nodes, m.n_refs, d, m.node_level, m.verts,
                                                                    (float4*)m.bvh, (uint4*)m.bvh16);
    return (int)hipGetLastError();
}

uint32_t refit_cost_blocks(uint32_t n_nodes) { return blocks_for(n_nodes); }

int refit_sah_cost(const vr4* bvh, uint32_t n_nodes, double* partial, double* cost, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nb = blocks_for(n_nodes);
    refit_cost_kernel<<<nb, kBlock, 0, s>>>((const float4*)bvh, n_nodes, partial);
    refit_cost_final_kernel<<<1, kBlock, 0, s>>>((const float4*)bvh, partial, nb, cost);
    return (int)hipGetLastError();
}

} // namespace vr
