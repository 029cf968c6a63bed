// vr_devbvh.hip -- BVH build on the device (gfx950), declared in vr_devbvh.hpp.
//
// A Morton-ordered tree balanced by count, so its depth is ceil(log2 L) and
// its whole topology is closed-form:
//   1. per-triangle boxes, validation flags and the mesh bounds (per-block
//      partials, then one block);
//   2. a stable radix sort of the triangles by the 63-bit Morton code of their
//      box centre (rocPRIM): ties keep the input order, i.e. triangle index;
//   3. L = max(2, ceil(n / max_leaf)) leaves, leaf j = sorted triangles
//      [floor(j n / L), floor((j + 1) n / L));
//   4. the inner node over leaves [a, b) splits at a + ceil((b - a) / 2): the
//      L - 1 inner nodes are the L - 1 split positions, and a thread finds its
//      node (or a leaf's root path) by walking down from [0, L);
//   5. boxes bottom-up, one launch per node height (both children of a node
//      are strictly lower), so kernel boundaries order every read after the
//      write it needs and no workgroup ever waits for another;
//   6. the emission stage shared with the SAH builder (vr_devmesh_dev.hpp
//      emit_mesh): the root first and the other nodes by descending surface
//      area, then the node rows and the per-triangle arrays.
// Everything is deterministic: no result depends on the order in which
// threads or blocks run (the only atomics are an OR of flags and a MAX).
#include <cstring>                                // rocPRIM's iterators call memset without including it
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "vr_devbvh.hpp"
#include "vr_devmesh_dev.hpp"

namespace vr {
namespace {

// union of the block's boxes, valid in thread 0
__device__ __forceinline__ DevBox block_union(DevBox b)
{
    __shared__ DevBox part[kBlock / 64];
    for (int o = 32; o > 0; o >>= 1) {
        DevBox t;
        for (int a = 0; a < 3; ++a) { t.lo[a] = __shfl_xor(b.lo[a], o); t.hi[a] = __shfl_xor(b.hi[a], o); }
        grow_fminmax(b, t);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBlock / 64; ++w) grow_fminmax(b, part[w]);
    return b;
}

// ---- 1. triangle boxes, validation, bounds -------------------------------
__global__ __launch_bounds__(kBlock) void tri_bounds_kernel(const float* __restrict__ pos, uint32_t n_verts,
                                                            const uint32_t* __restrict__ tris, uint32_t n_tris,
                                                            float4* __restrict__ tribox, float4* __restrict__ partial,
                                                            DevBuildStatus* st)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    DevBox b = empty_box();
    uint32_t flags = 0u;
    if (t < n_tris) {
        flags = triangle_box(pos, n_verts, tris, t, b);
        store_box(tribox, t, b);
    }
    if (flags) atomicOr(&st->flags, flags);
    b = block_union(b);
    if (threadIdx.x == 0) store_box(partial, blockIdx.x, b);
}

__global__ __launch_bounds__(kBlock) void reduce_bounds_kernel(const float4* __restrict__ partial, uint32_t n_partial,
                                                               float4* __restrict__ bounds)
{
    DevBox b = empty_box();
    for (uint32_t i = threadIdx.x; i < n_partial; i += kBlock) grow_fminmax(b, load_box(partial, i));
    b = block_union(b);
    if (threadIdx.x == 0) store_box(bounds, 0, b);
}

// ---- 2. Morton keys --------------------------------------------------------
__device__ __forceinline__ unsigned long long spread21(uint32_t v)
{
    unsigned long long x = v & 0x1fffffu;
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
// centre on [lo, hi] in 21 bits; a zero (or overflowed) extent gives cell 0
__device__ __forceinline__ uint32_t quant21(float c, float lo, float hi)
{
    const float ext = hi - lo;
    float f = ext > 0.f ? (c - lo) / ext * 2097152.f : 0.f;
    if (!(f >= 0.f)) f = 0.f;                    // NaN too
    if (f > 2097151.f) f = 2097151.f;
    return (uint32_t)f;
}
__global__ __launch_bounds__(kBlock) void morton_kernel(const float4* __restrict__ tribox,
                                                        const float4* __restrict__ bounds, uint32_t n_tris,
                                                        uint32_t n_refs, unsigned long long* __restrict__ keys,
                                                        uint32_t* __restrict__ vals)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_refs) return;
    const uint32_t t = k < n_tris ? k : 0u;       // a single triangle is stored twice
    const DevBox b = load_box(tribox, t), m = load_box(bounds, 0);
    const uint32_t qx = quant21(0.5f * b.lo[0] + 0.5f * b.hi[0], m.lo[0], m.hi[0]);
    const uint32_t qy = quant21(0.5f * b.lo[1] + 0.5f * b.hi[1], m.lo[1], m.hi[1]);
    const uint32_t qz = quant21(0.5f * b.lo[2] + 0.5f * b.hi[2], m.lo[2], m.hi[2]);
    keys[k] = (spread21(qx) << 2) | (spread21(qy) << 1) | spread21(qz);
    vals[k] = t;
}

// ---- 3./4. leaves and topology -------------------------------------------
__device__ __forceinline__ uint32_t split_of(uint32_t a, uint32_t b) { return a + (b - a + 1u) / 2u; }
__device__ __forceinline__ uint32_t leaf_first(uint32_t j, uint32_t n_refs, uint32_t n_leaves)
{
    return (uint32_t)((unsigned long long)j * n_refs / n_leaves);
}

// one thread per leaf: its root path (bit i = the child taken at depth i,
// under a leading 1: the key of ref_first), its exact box, its triangles' paths
__global__ __launch_bounds__(kBlock) void leaves_kernel(const float4* __restrict__ tribox,
                                                        const uint32_t* __restrict__ sorted, uint32_t n_refs,
                                                        uint32_t n_leaves, float4* __restrict__ leafbox,
                                                        unsigned long long* __restrict__ tpath, DevBuildStatus* st)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    uint32_t d = 0u;
    if (j < n_leaves) {
        uint32_t a = 0u, b = n_leaves;
        unsigned long long bits = 0ull;
        while (b - a > 1u) {
            const uint32_t m = split_of(a, b);
            const bool right = j >= m;
            bits |= (unsigned long long)(right ? 1u : 0u) << d;
            ++d;
            if (right) a = m; else b = m;
        }
        const unsigned long long path = (1ull << d) | bits;
        const uint32_t first = leaf_first(j, n_refs, n_leaves), end = leaf_first(j + 1u, n_refs, n_leaves);
        DevBox box = empty_box();
        for (uint32_t k = first; k < end; ++k) {
            grow_fminmax(box, load_box(tribox, sorted[k]));
            tpath[k] = path;
        }
        store_box(leafbox, j, box);
    }
    // a leaf d steps down hangs off an inner node at depth d (root = 1): one MAX per wave
    for (int o = 32; o > 0; o >>= 1) d = max(d, (uint32_t)__shfl_xor((int)d, o));
    if ((threadIdx.x & 63) == 0) atomicMax(&st->depth, d);
}

// one thread per inner node (= split position id + 1): children and height.
// A child is an inner node id (>= 0) or ~leaf (< 0).
__global__ __launch_bounds__(kBlock) void topology_kernel(uint32_t n_leaves, int2* __restrict__ child,
                                                          uint32_t* __restrict__ height)
{
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id + 1u >= n_leaves) return;
    const uint32_t s = id + 1u;
    uint32_t a = 0u, b = n_leaves, m;
    for (;;) {                                    // a < s < b holds throughout, and b - a shrinks
        m = split_of(a, b);
        if (s == m) break;
        if (s < m) b = m; else a = m;
    }
    int2 c;
    c.x = m - a == 1u ? ~(int32_t)a : (int32_t)(split_of(a, m) - 1u);
    c.y = b - m == 1u ? ~(int32_t)m : (int32_t)(split_of(m, b) - 1u);
    child[id] = c;
    height[id] = 32u - (uint32_t)__clz((int)(b - a - 1u));        // ceil(log2(b - a)), b - a >= 2
}

__device__ __forceinline__ DevBox child_box(int32_t c, const float4* leafbox, const float4* nodebox)
{
    return c < 0 ? load_box(leafbox, (uint32_t)~c) : load_box(nodebox, (uint32_t)c);
}

// ---- 5. inner boxes, one launch per height ---------------------------------
__global__ __launch_bounds__(kBlock) void refit_kernel(uint32_t n_nodes, uint32_t h, const int2* __restrict__ child,
                                                       const uint32_t* __restrict__ height,
                                                       const float4* __restrict__ leafbox, float4* nodebox)
{
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= n_nodes || height[id] != h) return;
    const int2 c = child[id];
    DevBox b = child_box(c.x, leafbox, nodebox);
    grow_fminmax(b, child_box(c.y, leafbox, nodebox));
    store_box(nodebox, id, b);
}

// ---- 6. emission: this tree's children (vr_devmesh_dev.hpp emit_nodes_kernel) ------
struct MortonChildren {
    const int2* child;
    const float4 *leafbox, *nodebox;
    uint32_t n_refs, n_leaves;
    __device__ bool operator()(uint32_t id, uint32_t, DevBox b[2], int32_t c[2], DevBuildStatus*) const
    {
        const int2 ch = child[id];
        c[0] = ch.x;
        c[1] = ch.y;
        for (int k = 0; k < 2; ++k) {
            b[k] = child_box(c[k], leafbox, nodebox);
            if (c[k] >= 0) continue;
            const uint32_t j = (uint32_t)~c[k], first = leaf_first(j, n_refs, n_leaves);
            c[k] = leaf_code(first, leaf_first(j + 1u, n_refs, n_leaves) - first);
        }
        return true;
    }
};

} // namespace

int devbvh_build(const float* positions, const float* normals, const float* tangents, const float* uvs,
                 uint32_t n_verts, const uint32_t* tris, uint32_t n_tris, uint32_t max_leaf, const MeshArrays& out,
                 DevBuildStatus* d_status, void** scratch_out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    *scratch_out = nullptr;
    const DevBuildShape sh = devbvh_shape(n_tris, max_leaf);
    const uint32_t n = sh.n_refs, L = sh.leaves, N = sh.nodes;
    const uint32_t nb_tris = blocks_for(n_tris);

    size_t temp_tris = 0, temp_nodes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, temp_tris, (unsigned long long*)nullptr,
                                             (unsigned long long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (size_t)n, 0u, 63u, s);
    if (e != hipSuccess) return (int)e;
    if ((e = emit_sort_temp_bytes(N, s, temp_nodes)) != hipSuccess) return (int)e;
    const size_t temp_bytes = temp_tris > temp_nodes ? temp_tris : temp_nodes;

    Arena ar;
    float4 *tribox, *partial, *bounds, *leafbox, *nodebox;
    unsigned long long *keys, *keys_sorted;
    uint32_t *vals, *sorted, *height;
    int2* child;
    EmitScratch emit;
    char* temp;
    e = carve_alloc(ar, [&](Arena& a) {
        tribox = a.take<float4>(2 * (size_t)n_tris);
        partial = a.take<float4>(2 * (size_t)nb_tris);
        bounds = a.take<float4>(2);
        keys = a.take<unsigned long long>(n);
        keys_sorted = a.take<unsigned long long>(n);
        vals = a.take<uint32_t>(n);
        sorted = a.take<uint32_t>(n);
        leafbox = a.take<float4>(2 * (size_t)L);
        nodebox = a.take<float4>(2 * (size_t)N);
        child = a.take<int2>(N);
        height = a.take<uint32_t>(N);
        emit.carve(a, N);
        temp = a.take<char>(temp_bytes ? temp_bytes : 16);
    });
    if (e != hipSuccess) return (int)e;
    auto bail = [&](hipError_t err) { (void)hipStreamSynchronize(s); (void)hipFree(ar.base); return (int)err; };

    tri_bounds_kernel<<<nb_tris, kBlock, 0, s>>>(positions, n_verts, tris, n_tris, tribox, partial, d_status);
    reduce_bounds_kernel<<<1, kBlock, 0, s>>>(partial, nb_tris, bounds);
    morton_kernel<<<blocks_for(n), kBlock, 0, s>>>(tribox, bounds, n_tris, n, keys, vals);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e);
    size_t tb = temp_bytes;
    e = rocprim::radix_sort_pairs(temp, tb, keys, keys_sorted, vals, sorted, (size_t)n, 0u, 63u, s);
    if (e != hipSuccess) return bail(e);

    leaves_kernel<<<blocks_for(L), kBlock, 0, s>>>(tribox, sorted, n, L, leafbox, out.tpath, d_status);
    topology_kernel<<<blocks_for(N), kBlock, 0, s>>>(L, child, height);
    for (uint32_t h = 1; h <= sh.depth; ++h)
        refit_kernel<<<blocks_for(N), kBlock, 0, s>>>(N, h, child, height, leafbox, nodebox);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e);

    // the root is the split of [0, L); leaves_kernel has recorded the depth
    const EmitArgs ea{ N, (L + 1u) / 2u - 1u, L, sh.depth, false, nodebox, sorted, n, n_tris,
                       { positions, normals, tangents, uvs }, tris, emit, temp, temp_bytes, out, d_status };
    if ((e = emit_mesh(ea, MortonChildren{ child, leafbox, nodebox, n, L }, s)) != hipSuccess) return bail(e);
    *scratch_out = ar.base;
    return 0;
}

} // namespace vr
