// vr_atlas.hip -- the kernels of vr_atlas.hpp.
//   prim_inverse   the inverse of prim_id by an integer atomicMin;
//   atlas_cover    one compact triangle per lane: the texel box in floating
//                  point, clipped to the atlas before any conversion to int; a
//                  box of at most 256 texels is walked by the lane, a larger
//                  triangle goes into a queue (ballot / mbcnt compaction);
//   atlas_cover_big  one block per queued triangle, its four waves taking the
//                  box's 8 x 8 texel tiles in turn, a texel per lane;
//   atlas_resolve  one texel per lane: the winner's barycentrics, a 16-byte cell;
//   atlas_gutter   one dilation pass from one cell plane into the other;
//   surface_fill   one record per lane: fill_hit's mesh arm, seven 16-byte stores.
// Coverage is a 64-bit atomicMin of (prim << 32 | compact triangle) per
// covered texel centre: an integer minimum does not depend on the order of its
// operands, so the winner is the smallest prim whatever the tree.  The box
// only bounds the walk; the exact test of vrhip.h decides.  fp64 throughout the
// raster, no contraction (the library builds with -ffp-contract=off), no
// float atomics.
#include <hip/hip_runtime.h>

#include "vr_atlas.hpp"
#include "vr_surface_dev.hpp"

namespace vr {

namespace {

constexpr unsigned long long kNoWinner = ~0ull;
constexpr uint32_t kIndexMask = (1u << kAtlasIndexBits) - 1u;
// texels a lane walks by itself.  256, not the 64 of a wave's tile: at 64 the 1M-triangle knot's 7 x 11 texel
// boxes at 4096^2 all went through the queue, two mostly empty tiles each (2.61 ms a call against 1.52;
// profiles/atlas/README.md)
constexpr uint32_t kSmallBox = 256u;

struct TriUV { double ax, ay, bx, by, cx, cy, A2; };

// The edge function of (p, q) at (x, y), evaluated on the endpoints ordered by
// (x, then y) and negated if that swapped them: the two triangles on a shared
// edge get the same magnitude with opposite signs.
__device__ __forceinline__ double edge_canon(double px, double py, double qx, double qy, double x, double y)
{
    const bool sw = qx < px || (qx == px && qy < py);
    const double lx = sw ? qx : px, ly = sw ? qy : py, hx = sw ? px : qx, hy = sw ? py : qy;
    const double e = (hx - lx) * (y - ly) - (hy - ly) * (x - lx);
    return sw ? -e : e;
}

// false: the triangle covers nothing (a non-finite uv, no area)
__device__ __forceinline__ bool tri_load(const vr2* uvs, uint32_t k, TriUV& t)
{
    const vr2 a = uvs[3u * k], b = uvs[3u * k + 1u], c = uvs[3u * k + 2u];
    const float big = 3.402823466e38f;
    const bool finite = fabsf(a.x) <= big && fabsf(a.y) <= big && fabsf(b.x) <= big && fabsf(b.y) <= big &&
                        fabsf(c.x) <= big && fabsf(c.y) <= big;
    t.ax = (double)a.x; t.ay = (double)a.y; t.bx = (double)b.x; t.by = (double)b.y; t.cx = (double)c.x; t.cy = (double)c.y;
    t.A2 = edge_canon(t.ax, t.ay, t.bx, t.by, t.cx, t.cy);
    return finite && t.A2 != 0.0 && fabs(t.A2) <= 1.7976931348623157e308;
}

__device__ __forceinline__ bool tri_covers(const TriUV& t, double x, double y)
{
    const double e0 = edge_canon(t.ax, t.ay, t.bx, t.by, x, y);
    const double e1 = edge_canon(t.bx, t.by, t.cx, t.cy, x, y);
    const double e2 = edge_canon(t.cx, t.cy, t.ax, t.ay, x, y);
    return t.A2 > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
}

// Texels [lo, hi] of one axis whose centres can lie in [mn, mx]: the texels
// that contain the two ends, widened by one, clipped to [0, n - 1] while still
// a double (uvs of 3e38 are legal).  false: none.
__device__ __forceinline__ bool axis_box(double mn, double mx, uint32_t n, uint32_t& lo, uint32_t& hi)
{
    const double l = floor(mn * (double)n) - 1.0, h = floor(mx * (double)n) + 1.0;
    const double last = (double)(n - 1u);
    if (!(h >= 0.0) || !(l <= last)) return false;
    lo = (uint32_t)fmax(l, 0.0);
    hi = (uint32_t)fmin(h, last);
    return true;
}

struct Box { uint32_t x0, x1, y0, y1; };
__device__ __forceinline__ bool tri_box(const TriUV& t, uint32_t w, uint32_t h, Box& b)
{
    return axis_box(fmin(fmin(t.ax, t.bx), t.cx), fmax(fmax(t.ax, t.bx), t.cx), w, b.x0, b.x1) &&
           axis_box(fmin(fmin(t.ay, t.by), t.cy), fmax(fmax(t.ay, t.by), t.cy), h, b.y0, b.y1);
}

__device__ __forceinline__ void cover_texel(const TriUV& t, unsigned long long key, unsigned long long* win, uint32_t w,
                                            uint32_t h, uint32_t x, uint32_t y)
{
    const double cx = ((double)x + 0.5) / (double)w, cy = ((double)y + 0.5) / (double)h;
    if (tri_covers(t, cx, cy)) atomicMin(win + ((size_t)y * w + x), key);
}

} // namespace

__global__ void __launch_bounds__(kBlockThreads) prim_inverse_kernel(const uint32_t* prim_id, uint32_t n_refs, uint32_t* inv,
                                                                     uint32_t n_prims)
{
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    if (k >= n_refs) return;
    const uint32_t prim = prim_id[k];
    if (prim < n_prims) atomicMin(inv + prim, k);
}

// queue[0]: the number of queued triangles; queue[1 ..]: their compact indices
__global__ void __launch_bounds__(kBlockThreads) atlas_cover_kernel(const vr2* uvs, const uint32_t* prim_id, uint32_t n_refs,
                                                                    uint32_t w, uint32_t h, unsigned long long* win,
                                                                    uint32_t* queue)
{
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    bool big = false;
    if (k < n_refs) {
        TriUV t;
        Box b;
        if (tri_load(uvs, k, t) && tri_box(t, w, h, b)) {
            const uint64_t texels = (uint64_t)(b.x1 - b.x0 + 1u) * (b.y1 - b.y0 + 1u);
            if (texels <= kSmallBox) {
                const unsigned long long key = (unsigned long long)prim_id[k] << 32 | k;
                for (uint32_t y = b.y0; y <= b.y1; ++y)
                    for (uint32_t x = b.x0; x <= b.x1; ++x) cover_texel(t, key, win, w, h, x, y);
            } else {
                big = true;
            }
        }
    }
    // every lane of the wave is here: one atomicAdd per wave reserves its slots
    const unsigned long long m = __ballot(big);
    if (m == 0ull) return;
    uint32_t base = 0u;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(queue, (uint32_t)__popcll(m));
    base = __shfl(base, 0, 64);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (big) queue[1u + base + rank] = k;
}

__global__ void __launch_bounds__(kBlockThreads) atlas_cover_big_kernel(const vr2* uvs, const uint32_t* prim_id, uint32_t w,
                                                                        uint32_t h, unsigned long long* win,
                                                                        const uint32_t* queue)
{
    const uint32_t n = queue[0];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    constexpr uint32_t kWaves = kBlockThreads / 64;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t k = queue[1u + i];
        TriUV t;
        Box b;
        if (!tri_load(uvs, k, t) || !tri_box(t, w, h, b)) continue;      // (queued triangles passed both)
        const unsigned long long key = (unsigned long long)prim_id[k] << 32 | k;
        const uint32_t tx = (b.x1 - b.x0) / 8u + 1u, ty = (b.y1 - b.y0) / 8u + 1u;
        const uint64_t tiles = (uint64_t)tx * ty;
        for (uint64_t tile = wave; tile < tiles; tile += kWaves) {
            const uint32_t x = b.x0 + (uint32_t)(tile % tx) * 8u + (lane & 7u);
            const uint32_t y = b.y0 + (uint32_t)(tile / tx) * 8u + (lane >> 3);
            if (x <= b.x1 && y <= b.y1) cover_texel(t, key, win, w, h, x, y);
        }
    }
}

__global__ void __launch_bounds__(kBlockThreads) atlas_resolve_kernel(const vr2* uvs, uint32_t w, uint32_t h,
                                                                      const unsigned long long* win, vr_u32x4* cells)
{
    const uint64_t n = (uint64_t)w * h;
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = win[i];
    vr_u32x4 cell = vr_u32x4{ kAtlasNone, kAtlasNone, 0u, 0u };
    if (key != kNoWinner) {
        const uint32_t k = (uint32_t)key;
        TriUV t;
        (void)tri_load(uvs, k, t);
        const double cx = ((double)(uint32_t)(i % w) + 0.5) / (double)w, cy = ((double)(uint32_t)(i / w) + 0.5) / (double)h;
        const double eu = (cx - t.ax) * (t.cy - t.ay) - (cy - t.ay) * (t.cx - t.ax);
        const double ev = (t.bx - t.ax) * (cy - t.ay) - (t.by - t.ay) * (cx - t.ax);
        const double ud = eu / t.A2, vd = ev / t.A2;
        const float u = (float)(ud < 0.0 ? 0.0 : ud > 1.0 ? 1.0 : ud);
        float v = (float)(vd < 0.0 ? 0.0 : vd > 1.0 ? 1.0 : vd);
        if (u + v > 1.f) v = 1.f - u;
        cell = vr_u32x4{ k, (uint32_t)(key >> 32), __float_as_uint(u), __float_as_uint(v) };
    }
    cells[i] = cell;
}

__global__ void __launch_bounds__(kBlockThreads) atlas_gutter_kernel(uint32_t w, uint32_t h, uint32_t pass, const vr_u32x4* src,
                                                                     vr_u32x4* dst)
{
    const uint64_t n = (uint64_t)w * h;
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    vr_u32x4 cell = src[i];
    if (cell.x == kAtlasNone) {
        const int x = (int)(i % w), y = (int)(i / w);
        const int dx[8] = { -1, 1, 0, 0, -1, 1, -1, 1 }, dy[8] = { 0, 0, -1, 1, -1, -1, 1, 1 };
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int nx = x + dx[j], ny = y + dy[j];
            if (cell.x != kAtlasNone || nx < 0 || ny < 0 || nx >= (int)w || ny >= (int)h) continue;
            const vr_u32x4 nb = src[(size_t)ny * w + (uint32_t)nx];
            if (nb.x != kAtlasNone) { cell = nb; cell.x = (nb.x & kIndexMask) | pass << kAtlasIndexBits; }
        }
    }
    dst[i] = cell;
}

// ATLAS: the records of the cells; otherwise those of the caller's (prim, u, v).
// An entry that names no triangle is classified before any attribute load.
template <bool ATLAS>
__global__ void __launch_bounds__(kBlockThreads) surface_fill_kernel(const RenderParams p, const SurfaceAt q, const vr_u32x4* cells)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= (uint64_t)q.n) return;
    uint32_t k = kAtlasNone, prim = kRayMiss;
    float u = 0.f, v = 0.f, t = 0.f;
    if constexpr (ATLAS) {
        const vr_u32x4 cell = cells[i];
        if (cell.x != kAtlasNone) {
            k = cell.x & kIndexMask;
            t = (float)(cell.x >> kAtlasIndexBits);
            prim = cell.y; u = __uint_as_float(cell.z); v = __uint_as_float(cell.w);
        }
    } else {
        const float big = 3.402823466e38f;
        prim = q.prims[i]; u = q.bary[2u * i]; v = q.bary[2u * i + 1u];
        if (prim < q.n_prims && fabsf(u) <= big && fabsf(v) <= big) k = q.inv[prim];
    }
    const vr_u32x4 zero = vr_u32x4{ 0u, 0u, 0u, 0u };
    vr_u32x4 w0 = zero, w1 = zero, w2 = zero, w3 = zero, w4 = zero, w5 = zero, w6 = zero;
    if (k != kAtlasNone) {
        const int a = (int)(3u * k);
        Ray r;
        r.o = mk4(0.f, 0.f, 0.f, 0.f); r.d = mk4(0.f, 0.f, 0.f, 0.f);
        HitRec hr;
        hr.t = 0.f; hr.kind = HK_MESH; hr.idx = a; hr.bu = u; hr.bv = v; hr.su = 0.f; hr.sv = 0.f;
        Hit h;
        fill_hit<kFeatAll>(p, r, hr, h);                 // the record of a hit there; its hit point has no meaning without a ray
        const float b0 = 1.f - u - v;
        const vr3 p0 = p.verts[a], p1 = p.verts[a + 1], p2 = p.verts[a + 2];
        h.hp = mk4((b0 * p0.x + u * p1.x) + v * p2.x, (b0 * p0.y + u * p1.y) + v * p2.y, (b0 * p0.z + u * p1.z) + v * p2.z, 0.f);
        float tu, tv;
        surface_mesh_uv(p, a, u, v, tu, tv);             // the surface query's own uv and record layout (vr_surface_dev.hpp)
        surface_hit_rows(t, (uint32_t)HK_MESH, prim, h, u, v, tu, tv, w0, w1, w2, w3, w4, w5, w6);
    } else if constexpr (ATLAS) {
        w0 = surface_miss_row();
    }
    vr_u32x4* rec = reinterpret_cast<vr_u32x4*>(q.hits + i);         // seven 16-B stores per record
    rec[0] = w0; rec[1] = w1; rec[2] = w2; rec[3] = w3; rec[4] = w4; rec[5] = w5; rec[6] = w6;
}

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlockThreads - 1u) / kBlockThreads); }

int launch_prim_inverse(const uint32_t* prim_id, uint32_t n_refs, uint32_t* inv, uint32_t n_prims, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(inv, 0xff, (size_t)n_prims * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    if (n_refs == 0u) return 0;
    prim_inverse_kernel<<<blocks_for(n_refs), kBlockThreads, 0, s>>>(prim_id, n_refs, inv, n_prims);
    return (int)hipGetLastError();
}

int launch_surface_at(const RenderParams& p, const SurfaceAt& q, void* stream)
{
    surface_fill_kernel<false><<<blocks_for(q.n), kBlockThreads, 0, (hipStream_t)stream>>>(p, q, nullptr);
    return (int)hipGetLastError();
}

int launch_atlas_surface(const RenderParams& p, const Atlas& q, uint32_t cu_count, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n = (uint64_t)q.w * q.h;
    vr_u32x4* cells_a = (vr_u32x4*)q.scratch;
    vr_u32x4* cells_b = cells_a + n;
    unsigned long long* win = (unsigned long long*)cells_b;          // dead once resolved, before the first gutter pass writes cells_b
    uint32_t* queue = (uint32_t*)(cells_b + n);
    hipError_t e = hipMemsetAsync(win, 0xff, n * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(queue, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    if (p.n_tris > 0u) {
        atlas_cover_kernel<<<blocks_for(p.n_tris), kBlockThreads, 0, s>>>(p.uvs, q.prim_id, p.n_tris, q.w, q.h, win, queue);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        // one resident set of blocks at most; the queue's length stays on the device
        const uint64_t resident = (uint64_t)(cu_count ? cu_count : 1u) * 8u;
        atlas_cover_big_kernel<<<(uint32_t)(p.n_tris < resident ? p.n_tris : resident), kBlockThreads, 0, s>>>(
            p.uvs, q.prim_id, q.w, q.h, win, queue);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;   // each step reports its own failed launch
    }
    atlas_resolve_kernel<<<blocks_for(n), kBlockThreads, 0, s>>>(p.uvs, q.w, q.h, win, cells_a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    for (uint32_t pass = 1u; pass <= q.gutter; ++pass) {
        atlas_gutter_kernel<<<blocks_for(n), kBlockThreads, 0, s>>>(q.w, q.h, pass, cells_a, cells_b);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        vr_u32x4* tmp = cells_a; cells_a = cells_b; cells_b = tmp;
    }
    SurfaceAt f{};
    f.n = (uint32_t)n; f.hits = q.hits;
    surface_fill_kernel<true><<<blocks_for(n), kBlockThreads, 0, s>>>(p, f, cells_a);
    return (int)hipGetLastError();
}

} // namespace vr
