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
//   6. the root first and the other nodes by descending surface area (a second
//      radix sort), then the fp32 and fp16 node rows and the per-triangle
//      arrays in the layout the render kernels read (vr_kernel.hpp node_step,
//      trav_iter, ref_first).
// Everything is deterministic: no result depends on the order in which
// threads or blocks run (the only atomics are an OR of flags and a MAX).
#include <cstring>                                // rocPRIM's iterators call memset without including it
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "vr_devbvh.hpp"
#include "vr_refit.hpp"

namespace vr {
namespace {

constexpr int kBlock = 256;                       // four wave64

struct Box { float4 lo, hi; };                    // .w unused: two 16-B accesses per box

__device__ __forceinline__ Box empty_box()
{
    const float inf = __builtin_inff();
    return { make_float4(inf, inf, inf, 0.f), make_float4(-inf, -inf, -inf, 0.f) };
}
__device__ __forceinline__ void grow(Box& b, const Box& o)
{
    b.lo.x = fminf(b.lo.x, o.lo.x); b.lo.y = fminf(b.lo.y, o.lo.y); b.lo.z = fminf(b.lo.z, o.lo.z);
    b.hi.x = fmaxf(b.hi.x, o.hi.x); b.hi.y = fmaxf(b.hi.y, o.hi.y); b.hi.z = fmaxf(b.hi.z, o.hi.z);
}
__device__ __forceinline__ void grow(Box& b, float x, float y, float z)
{
    b.lo.x = fminf(b.lo.x, x); b.lo.y = fminf(b.lo.y, y); b.lo.z = fminf(b.lo.z, z);
    b.hi.x = fmaxf(b.hi.x, x); b.hi.y = fmaxf(b.hi.y, y); b.hi.z = fmaxf(b.hi.z, z);
}
__device__ __forceinline__ Box load_box(const float4* a, size_t i) { return { a[2 * i], a[2 * i + 1] }; }
__device__ __forceinline__ void store_box(float4* a, size_t i, const Box& b) { a[2 * i] = b.lo; a[2 * i + 1] = b.hi; }

// union of the block's boxes, valid in thread 0
__device__ __forceinline__ Box block_union(Box b)
{
    __shared__ Box part[kBlock / 64];
    for (int o = 32; o > 0; o >>= 1) {
        Box t;
        t.lo = make_float4(__shfl_xor(b.lo.x, o), __shfl_xor(b.lo.y, o), __shfl_xor(b.lo.z, o), 0.f);
        t.hi = make_float4(__shfl_xor(b.hi.x, o), __shfl_xor(b.hi.y, o), __shfl_xor(b.hi.z, o), 0.f);
        grow(b, t);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBlock / 64; ++w) grow(b, part[w]);
    return b;
}

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    const float big = 3.402823466e38f;
    return fabsf(x) <= big && fabsf(y) <= big && fabsf(z) <= big;      // false for inf and NaN
}

// ---- 1. triangle boxes, validation, bounds -------------------------------
__global__ __launch_bounds__(kBlock) void tri_bounds_kernel(const float* __restrict__ pos, uint32_t n_verts,
                                                            const uint32_t* __restrict__ tris, uint32_t n_tris,
                                                            float4* __restrict__ tribox, float4* __restrict__ partial,
                                                            DevBuildStatus* st)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    Box b = empty_box();
    uint32_t flags = 0u;
    if (t < n_tris) {
        const uint32_t i0 = tris[3 * (size_t)t], i1 = tris[3 * (size_t)t + 1], i2 = tris[3 * (size_t)t + 2];
        if (i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) {
            flags = DEVBVH_BAD_INDEX;
        } else {
            const uint32_t idx[3] = { i0, i1, i2 };
            for (int k = 0; k < 3; ++k) {
                const float* p = pos + 3 * (size_t)idx[k];
                const float x = p[0], y = p[1], z = p[2];
                if (!finite3(x, y, z)) flags |= DEVBVH_NONFINITE;
                grow(b, x, y, z);
            }
            if (flags) b = empty_box();
        }
        store_box(tribox, t, b);
    }
    if (flags) atomicOr(&st->flags, flags);
    b = block_union(b);
    if (threadIdx.x == 0) store_box(partial, blockIdx.x, b);
}

__global__ __launch_bounds__(kBlock) void reduce_bounds_kernel(const float4* __restrict__ partial, uint32_t n_partial,
                                                               float4* __restrict__ bounds)
{
    Box b = empty_box();
    for (uint32_t i = threadIdx.x; i < n_partial; i += kBlock) grow(b, load_box(partial, i));
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
    const Box b = load_box(tribox, t), m = load_box(bounds, 0);
    const uint32_t qx = quant21(0.5f * b.lo.x + 0.5f * b.hi.x, m.lo.x, m.hi.x);
    const uint32_t qy = quant21(0.5f * b.lo.y + 0.5f * b.hi.y, m.lo.y, m.hi.y);
    const uint32_t qz = quant21(0.5f * b.lo.z + 0.5f * b.hi.z, m.lo.z, m.hi.z);
    keys[k] = (spread21(qx) << 2) | (spread21(qy) << 1) | spread21(qz);
    vals[k] = t;
}

// ---- 3./4. leaves and topology -------------------------------------------
__device__ __forceinline__ uint32_t split_of(uint32_t a, uint32_t b) { return a + (b - a + 1u) / 2u; }
__device__ __forceinline__ uint32_t leaf_first(uint32_t j, uint32_t n_refs, uint32_t n_leaves)
{
    return (uint32_t)((unsigned long long)j * n_refs / n_leaves);
}
__device__ __forceinline__ int32_t leaf_code(uint32_t j, uint32_t n_refs, uint32_t n_leaves)
{
    const uint32_t first = leaf_first(j, n_refs, n_leaves), count = leaf_first(j + 1u, n_refs, n_leaves) - first;
    return ~(int32_t)((first << kLeafCountBits) | count);
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
        Box box = empty_box();
        for (uint32_t k = first; k < end; ++k) {
            grow(box, load_box(tribox, sorted[k]));
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

__device__ __forceinline__ Box child_box(int32_t c, const float4* leafbox, const float4* nodebox)
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
    Box b = child_box(c.x, leafbox, nodebox);
    grow(b, child_box(c.y, leafbox, nodebox));
    store_box(nodebox, id, b);
}

// ---- 6. node order and emission -------------------------------------------
// key: the root first, then descending area (the complement of a non-negative
// float's bits ascends as the float descends), ties by split position
__global__ __launch_bounds__(kBlock) void area_keys_kernel(uint32_t n_nodes, uint32_t root,
                                                           const float4* __restrict__ nodebox,
                                                           unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ vals)
{
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= n_nodes) return;
    const Box b = load_box(nodebox, id);
    const float dx = b.hi.x - b.lo.x, dy = b.hi.y - b.lo.y, dz = b.hi.z - b.lo.z;
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
    if (i < n_nodes) newpos[order[i]] = i;
}

__global__ __launch_bounds__(kBlock) void emit_nodes_kernel(uint32_t n_nodes, uint32_t n_refs, uint32_t n_leaves,
                                                            const uint32_t* __restrict__ order,
                                                            const uint32_t* __restrict__ newpos,
                                                            const int2* __restrict__ child,
                                                            const float4* __restrict__ leafbox,
                                                            const float4* __restrict__ nodebox,
                                                            float4* __restrict__ bvh, uint4* __restrict__ bvh16,
                                                            DevBuildStatus* st)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0u) {
        st->nodes = n_nodes;
        st->leaves = n_leaves;
        st->slots = 3u * n_refs + n_leaves;
    }
    if (i >= n_nodes) return;
    const int2 c = child[order[i]];
    const Box b0 = child_box(c.x, leafbox, nodebox), b1 = child_box(c.y, leafbox, nodebox);
    // float4 offsets for inner children, ~((first << 7) | count) for leaves
    const int32_t i0 = c.x < 0 ? leaf_code((uint32_t)~c.x, n_refs, n_leaves) : (int32_t)(4u * newpos[c.x]);
    const int32_t i1 = c.y < 0 ? leaf_code((uint32_t)~c.y, n_refs, n_leaves) : (int32_t)(4u * newpos[c.y]);
    bvh[4 * (size_t)i + 0] = make_float4(b0.lo.x, b0.hi.x, b0.lo.y, b0.hi.y);
    bvh[4 * (size_t)i + 1] = make_float4(b1.lo.x, b1.hi.x, b1.lo.y, b1.hi.y);
    bvh[4 * (size_t)i + 2] = make_float4(b0.lo.z, b0.hi.z, b1.lo.z, b1.hi.z);
    bvh[4 * (size_t)i + 3] = make_float4(__int_as_float(i0), __int_as_float(i1), 0.f, 0.f);
    // the fp16 rows of build_nodes16: [c0 x y z | c1 x] [c1 y z | idx0 idx1], lows down, highs up
    auto pair = [](float lo, float hi) {
        return (uint32_t)half_directed(__float_as_uint(lo), false) |
               ((uint32_t)half_directed(__float_as_uint(hi), true) << 16);
    };
    bvh16[2 * (size_t)i + 0] = make_uint4(pair(b0.lo.x, b0.hi.x), pair(b0.lo.y, b0.hi.y), pair(b0.lo.z, b0.hi.z),
                                          pair(b1.lo.x, b1.hi.x));
    bvh16[2 * (size_t)i + 1] = make_uint4(pair(b1.lo.y, b1.hi.y), pair(b1.lo.z, b1.hi.z), (uint32_t)i0, (uint32_t)i1);
}

// one thread per compact triangle: vertices, edges and attributes in sorted
// order.  The only kernel that follows the caller's indices after validation,
// so it does nothing when a flag is up.
__global__ __launch_bounds__(kBlock) void emit_tris_kernel(const float* __restrict__ pos, const float* __restrict__ nrm,
                                                           const float* __restrict__ tan, const float* __restrict__ uv,
                                                           const uint32_t* __restrict__ tris,
                                                           const uint32_t* __restrict__ sorted, uint32_t n_refs,
                                                           vr3* __restrict__ verts, vr3* __restrict__ tri_e,
                                                           vr4* __restrict__ normals, vr4* __restrict__ tangents,
                                                           vr2* __restrict__ uvs, uint32_t* __restrict__ slot_vert,
                                                           const DevBuildStatus* st)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_refs || st->flags != 0u) return;
    const uint32_t t = sorted[k];
    vr3 p[3];
    for (int v = 0; v < 3; ++v) {
        const size_t i = tris[3 * (size_t)t + v];
        const size_t o = 3 * (size_t)k + v;
        p[v] = vr3{ pos[3 * i], pos[3 * i + 1], pos[3 * i + 2] };
        verts[o] = p[v];
        slot_vert[o] = (uint32_t)i;
        normals[o] = nrm ? vr4{ nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], 0.f } : vr4{ 0.f, 0.f, 0.f, 0.f };
        tangents[o] = tan ? vr4{ tan[3 * i], tan[3 * i + 1], tan[3 * i + 2], 0.f } : vr4{ 0.f, 0.f, 0.f, 0.f };
        uvs[o] = uv ? vr2{ uv[2 * i], uv[2 * i + 1] } : vr2{ 0.f, 0.f };
    }
    // the Moller-Trumbore edges, the kernel's own fp32 subtractions (no contraction possible)
    tri_e[3 * (size_t)k + 0] = p[0];
    tri_e[3 * (size_t)k + 1] = vr3{ p[1].x - p[0].x, p[1].y - p[0].y, p[1].z - p[0].z };
    tri_e[3 * (size_t)k + 2] = vr3{ p[2].x - p[0].x, p[2].y - p[0].y, p[2].z - p[0].z };
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

} // namespace

int devbvh_build(const float* positions, const float* normals, const float* tangents, const float* uvs,
                 uint32_t n_verts, const uint32_t* tris, uint32_t n_tris, uint32_t max_leaf, const DevBuildOut& out,
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
    e = rocprim::radix_sort_pairs(nullptr, temp_nodes, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                  (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)N, 0u, 64u, s);
    if (e != hipSuccess) return (int)e;
    const size_t temp_bytes = temp_tris > temp_nodes ? temp_tris : temp_nodes;

    // two passes over the same carving: sizes first, then pointers
    Arena ar;
    float4 *tribox = nullptr, *partial = nullptr, *bounds = nullptr, *leafbox = nullptr, *nodebox = nullptr;
    unsigned long long *keys = nullptr, *keys_sorted = nullptr, *akeys = nullptr, *akeys_sorted = nullptr;
    uint32_t *vals = nullptr, *sorted = nullptr, *avals = nullptr, *order = nullptr, *newpos = nullptr, *height = nullptr;
    int2* child = nullptr;
    char* temp = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        ar.used = 0;
        tribox = ar.take<float4>(2 * (size_t)n_tris);
        partial = ar.take<float4>(2 * (size_t)nb_tris);
        bounds = ar.take<float4>(2);
        keys = ar.take<unsigned long long>(n);
        keys_sorted = ar.take<unsigned long long>(n);
        vals = ar.take<uint32_t>(n);
        sorted = ar.take<uint32_t>(n);
        leafbox = ar.take<float4>(2 * (size_t)L);
        nodebox = ar.take<float4>(2 * (size_t)N);
        child = ar.take<int2>(N);
        height = ar.take<uint32_t>(N);
        akeys = ar.take<unsigned long long>(N);
        akeys_sorted = ar.take<unsigned long long>(N);
        avals = ar.take<uint32_t>(N);
        order = ar.take<uint32_t>(N);
        newpos = ar.take<uint32_t>(N);
        temp = ar.take<char>(temp_bytes ? temp_bytes : 16);
        if (pass == 0) {
            void* p = nullptr;
            e = hipMalloc(&p, ar.used);
            if (e != hipSuccess) return (int)e;
            ar.base = (char*)p;
        }
    }
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
    area_keys_kernel<<<blocks_for(N), kBlock, 0, s>>>(N, (L + 1u) / 2u - 1u, nodebox, akeys, avals);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e);
    tb = temp_bytes;
    e = rocprim::radix_sort_pairs(temp, tb, akeys, akeys_sorted, avals, order, (size_t)N, 0u, 64u, s);
    if (e != hipSuccess) return bail(e);

    newpos_kernel<<<blocks_for(N), kBlock, 0, s>>>(N, order, newpos);
    emit_nodes_kernel<<<blocks_for(N), kBlock, 0, s>>>(N, n, L, order, newpos, child, leafbox, nodebox,
                                                       (float4*)out.bvh, (uint4*)out.bvh16, d_status);
    emit_tris_kernel<<<blocks_for(n), kBlock, 0, s>>>(positions, normals, tangents, uvs, tris, sorted, n, out.verts,
                                                      out.tri_e, out.normals, out.tangents, out.uvs, out.slot_vert,
                                                      d_status);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e);
    if ((e = (hipError_t)refit_levels(out.bvh, N, sh.depth, out.node_level, s)) != hipSuccess) return bail(e);
    *scratch_out = ar.base;
    return 0;
}

int launch_half_box(const float* in, size_t n, uint16_t* down, uint16_t* up, void* stream)
{
    if (n == 0) return 0;
    half_box_kernel<<<blocks_for(n), kBlock, 0, (hipStream_t)stream>>>(in, n, down, up);
    return (int)hipGetLastError();
}

} // namespace vr
