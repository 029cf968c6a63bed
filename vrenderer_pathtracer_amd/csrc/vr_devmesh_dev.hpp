// vr_devmesh_dev.hpp -- the device side of vr_devmesh.hpp (hipcc only): the
// one writer of a node's rows, the one gather of a compact triangle, triangle
// validation, and the emission stage both builders end with (emit_mesh),
// in the layout the render kernels read (vr_kernel.hpp node_step, trav_iter,
// ref_first).  The kernels that need no builder's types are in vr_devmesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "vr_devmesh.hpp"
#include "vr_refit.hpp"

namespace vr {

constexpr int kBlock = 256;                       // four wave64
inline uint32_t blocks_for(size_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// carves 256-B aligned pieces out of one allocation
struct Arena {
    size_t used = 0;
    char* base = nullptr;
    template <typename T>
    T* take(size_t n)
    {
        const size_t off = used;
        used += (n * sizeof(T) + 255u) & ~(size_t)255u;
        return base ? (T*)(base + off) : nullptr;
    }
};
// two passes over the same carving: sizes first, then pointers into one allocation
template <typename Carve>
hipError_t carve_alloc(Arena& ar, Carve&& carve)
{
    ar = Arena{};
    carve(ar);
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, ar.used);
    if (e != hipSuccess) return e;
    ar = Arena{ 0, (char*)p };
    carve(ar);
    return hipSuccess;
}

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    const float big = 3.402823466e38f;
    return fabsf(x) <= big && fabsf(y) <= big && fabsf(z) <= big;      // false for inf and NaN
}

// ---- boxes: fminf / fmaxf growth, two float4 in memory (.w unused) --------------
__device__ __forceinline__ void grow_fminmax(DevBox& b, float x, float y, float z)
{
    b.lo[0] = fminf(b.lo[0], x); b.lo[1] = fminf(b.lo[1], y); b.lo[2] = fminf(b.lo[2], z);
    b.hi[0] = fmaxf(b.hi[0], x); b.hi[1] = fmaxf(b.hi[1], y); b.hi[2] = fmaxf(b.hi[2], z);
}
__device__ __forceinline__ void grow_fminmax(DevBox& b, const DevBox& o)
{
    for (int a = 0; a < 3; ++a) { b.lo[a] = fminf(b.lo[a], o.lo[a]); b.hi[a] = fmaxf(b.hi[a], o.hi[a]); }
}
__device__ __forceinline__ DevBox load_box(const float4* a, size_t i)
{
    const float4 lo = a[2 * i], hi = a[2 * i + 1];
    return { { lo.x, lo.y, lo.z }, { hi.x, hi.y, hi.z } };
}
__device__ __forceinline__ void store_box(float4* a, size_t i, const DevBox& b)
{
    a[2 * i] = make_float4(b.lo[0], b.lo[1], b.lo[2], 0.f);
    a[2 * i + 1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.f);
}

// ---- triangle validation -----------------------------------------------------------
// The box of triangle t and its DEVBVH_* flags; the box is empty when a flag is up.
__device__ __forceinline__ uint32_t triangle_box(const float* __restrict__ pos, uint32_t n_verts,
                                                 const uint32_t* __restrict__ tris, uint32_t t, DevBox& b)
{
    b = empty_box();
    const uint32_t idx[3] = { tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2] };
    if (idx[0] >= n_verts || idx[1] >= n_verts || idx[2] >= n_verts) return DEVBVH_BAD_INDEX;
    uint32_t flags = 0u;
    for (int k = 0; k < 3; ++k) {
        const float* p = pos + 3 * (size_t)idx[k];
        const float x = p[0], y = p[1], z = p[2];
        if (!finite3(x, y, z)) flags |= DEVBVH_NONFINITE;
        grow_fminmax(b, x, y, z);
    }
    if (flags) b = empty_box();
    return flags;
}

// ---- the node rows -------------------------------------------------------------------
// Node i of the emitted array from its two child boxes and index words: three
// fp32 rows [c0 x, y] [c1 x, y] [c0 z | c1 z] as lo, hi pairs, the index row,
// and the fp16 rows of build_nodes16 (vr_mesh_layout.cpp): [c0 x y z | c1 x]
// [c1 y z | idx0 idx1], lows rounded down, highs up.  A refit keeps the index
// row (kIndexRow false) and passes the words it read there.
template <bool kIndexRow>
__device__ __forceinline__ void write_node_rows(float4* bvh, uint4* bvh16, size_t i, const DevBox& b0, const DevBox& b1,
                                                int32_t i0, int32_t i1)
{
    bvh[4 * i + 0] = make_float4(b0.lo[0], b0.hi[0], b0.lo[1], b0.hi[1]);
    bvh[4 * i + 1] = make_float4(b1.lo[0], b1.hi[0], b1.lo[1], b1.hi[1]);
    bvh[4 * i + 2] = make_float4(b0.lo[2], b0.hi[2], b1.lo[2], b1.hi[2]);
    if (kIndexRow) bvh[4 * i + 3] = make_float4(__int_as_float(i0), __int_as_float(i1), 0.f, 0.f);
    auto pair = [](float lo, float hi) {
        return (uint32_t)half_directed(__float_as_uint(lo), false) |
               ((uint32_t)half_directed(__float_as_uint(hi), true) << 16);
    };
    bvh16[2 * i + 0] = make_uint4(pair(b0.lo[0], b0.hi[0]), pair(b0.lo[1], b0.hi[1]), pair(b0.lo[2], b0.hi[2]),
                                  pair(b1.lo[0], b1.hi[0]));
    bvh16[2 * i + 1] = make_uint4(pair(b1.lo[1], b1.hi[1]), pair(b1.lo[2], b1.hi[2]), (uint32_t)i0, (uint32_t)i1);
}

// ---- the compact triangles ---------------------------------------------------------------
struct TriSource { const float *pos, *nrm, *tan, *uv; };        // per caller vertex; all but pos may be null
struct TriArrays { vr3 *verts, *tri_e; vr4 *normals, *tangents; vr2* uvs; uint32_t* slot_vert; };

// Compact triangle k from the caller's vertices vi[0..2]: verts, the
// Moller-Trumbore edges (fp32 subtractions, no contraction possible) and the
// attributes.  A build (kBuild) also records slot_vert and uvs and zeroes an
// absent attribute; a refit leaves those as they are.
template <bool kBuild>
__device__ __forceinline__ void gather_triangle(const TriSource& in, const TriArrays& out, uint32_t k, const uint32_t vi[3])
{
    // every load before the first store: the arrays carry no restrict through the structs
    vr3 p[3];
    vr4 n[3] = {}, t[3] = {};
    vr2 uv[3] = {};
    for (int v = 0; v < 3; ++v) {
        const size_t i = vi[v];
        p[v] = vr3{ in.pos[3 * i], in.pos[3 * i + 1], in.pos[3 * i + 2] };
        if (in.nrm) n[v] = vr4{ in.nrm[3 * i], in.nrm[3 * i + 1], in.nrm[3 * i + 2], 0.f };
        if (in.tan) t[v] = vr4{ in.tan[3 * i], in.tan[3 * i + 1], in.tan[3 * i + 2], 0.f };
        if (kBuild && in.uv) uv[v] = vr2{ in.uv[2 * i], in.uv[2 * i + 1] };
    }
    for (int v = 0; v < 3; ++v) {
        const size_t o = 3 * (size_t)k + v;
        out.verts[o] = p[v];
        if (kBuild || in.nrm) out.normals[o] = n[v];
        if (kBuild || in.tan) out.tangents[o] = t[v];
        if (kBuild) {
            out.slot_vert[o] = vi[v];
            out.uvs[o] = uv[v];
        }
    }
    out.tri_e[3 * (size_t)k + 0] = p[0];
    out.tri_e[3 * (size_t)k + 1] = vr3{ p[1].x - p[0].x, p[1].y - p[0].y, p[1].z - p[0].z };
    out.tri_e[3 * (size_t)k + 2] = vr3{ p[2].x - p[0].x, p[2].y - p[0].y, p[2].z - p[0].z };
}

// ---- emission: what both builders end with ---------------------------------------------------
struct EmitScratch {                              // per node, out of the builder's arena
    unsigned long long *keys, *keys_sorted;
    uint32_t *vals, *order, *newpos;
    void carve(Arena& ar, size_t max_nodes)
    {
        keys = ar.take<unsigned long long>(max_nodes); keys_sorted = ar.take<unsigned long long>(max_nodes);
        vals = ar.take<uint32_t>(max_nodes); order = ar.take<uint32_t>(max_nodes); newpos = ar.take<uint32_t>(max_nodes);
    }
};
struct EmitArgs {
    uint32_t n_nodes, root;                       // builder nodes, and which of them is the root
    uint32_t n_leaves, depth;                     // depth: the tree's levels (root = 1)
    bool record_depth;                            // write depth to the status record (else the builder has)
    const float4* nodebox;                        // per builder node, its own box
    const uint32_t* refs;                         // the caller's triangle of each compact triangle
    uint32_t n_refs, n_tris;
    TriSource src;
    const uint32_t* tris;
    EmitScratch scratch;
    char* temp; size_t temp_bytes;                // for the sort (emit_sort_temp_bytes)
    MeshArrays out;                               // the pointers only: the shape is what this call reports
    DevBuildStatus* status;
};

// vr_devmesh.hip: the sort's temporary storage for up to max_nodes nodes; scratch.order
// (the root first, the others by descending area of their box, ties by builder
// node number) and its inverse scratch.newpos; the per-triangle arrays in the
// order of refs (nothing when a flag is up)
hipError_t emit_sort_temp_bytes(uint32_t max_nodes, hipStream_t s, size_t& bytes);
hipError_t emit_order(const EmitArgs& a, hipStream_t s);
hipError_t emit_tris(const EmitArgs& a, hipStream_t s);

// Children: a small by-value accessor of a builder's own tree,
//   __device__ bool operator()(uint32_t id, uint32_t n_nodes, DevBox b[2], int32_t c[2], DevBuildStatus* st) const
// gives the child boxes of builder node id and, per child, a builder node
// number (>= 0) or the leaf code (< 0); false (after flagging st) emits nothing.
template <typename Children>
__global__ __launch_bounds__(kBlock) void emit_nodes_kernel(EmitArgs a, Children children)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0u) {
        a.status->nodes = a.n_nodes;
        a.status->leaves = a.n_leaves;
        a.status->slots = 3u * a.n_refs + a.n_leaves;
        if (a.record_depth) a.status->depth = a.depth;
    }
    if (i >= a.n_nodes) return;
    DevBox b[2];
    int32_t c[2];
    if (!children(a.scratch.order[i], a.n_nodes, b, c, a.status)) return;
    for (int k = 0; k < 2; ++k)                   // float4 offsets for inner children
        if (c[k] >= 0) c[k] = (int32_t)(4u * a.scratch.newpos[c[k]]);
    write_node_rows<true>((float4*)a.out.bvh, (uint4*)a.out.bvh16, i, b[0], b[1], c[0], c[1]);
}

// node order, node rows, triangle arrays, node levels: enqueued on s
template <typename Children>
hipError_t emit_mesh(const EmitArgs& a, const Children& children, hipStream_t s)
{
    hipError_t e = emit_order(a, s);
    if (e != hipSuccess) return e;
    emit_nodes_kernel<<<blocks_for(a.n_nodes), kBlock, 0, s>>>(a, children);
    if ((e = emit_tris(a, s)) != hipSuccess) return e;
    return (hipError_t)refit_levels(a.out.bvh, a.n_nodes, a.depth, a.out.node_level, s);
}

} // namespace vr
