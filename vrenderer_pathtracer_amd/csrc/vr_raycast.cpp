// vr_raycast.cpp -- the host walk of vr_rayquery.hpp: one lane of the
// reference's traversal (cuda/src/PathTracer.cu:276-463) over the flattened
// arrays, with its triangle test (cuda/include/RayIntersection.cuh:54-111) and
// closest-hit update (:379-386).  The warp vote (:353-363) only decides when a
// warp's lanes turn to their postponed leaves; no lane's sequence of box and
// triangle tests depends on it, so one lane alone needs none.  Host C++ only,
// compiled with -ffp-contract=off like the rest of the library: every
// operation below is one fp32 rounding, in the reference's order.
#include "vr_rayquery.hpp"

#include <cmath>
#include <cstring>
#include <vector>

#include "vr_bvh.hpp"

namespace vr {
namespace {

constexpr float kEps = 0.0000000003f;             // MathHelpers.cuh:17
constexpr int kWalkSentinel = 0x76543210;         // EntrypointSentinel (:276)

inline int32_t bits_of(float f) { int32_t i; std::memcpy(&i, &f, 4); return i; }
inline float float_of(int32_t i) { float f; std::memcpy(&f, &i, 4); return f; }
inline int32_t imin(int32_t a, int32_t b) { return a < b ? a : b; }
inline int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

// fminf / fmaxf as the GPUs evaluate them: a NaN operand is ignored and
// -0 < +0 (the C library leaves the zeros' order open, and the integer
// comparisons below see the sign)
inline float fmin_dev(float a, float b)
{
    if (a != a) return b;
    if (b != b) return a;
    if (a < b) return a;
    if (b < a) return b;
    return std::signbit(a) ? a : b;
}
inline float fmax_dev(float a, float b)
{
    if (a != a) return b;
    if (b != b) return a;
    if (a > b) return a;
    if (b > a) return b;
    return std::signbit(a) ? b : a;
}

// A slab distance as the device holds it.  Finite rays make NaN slabs (inf - inf
// once n * inv and o * inv overflow alike), and the integer comparisons below
// read a NaN's sign.  The device's invalid operations give 0xffc00000, the
// sign set, as x86's do; other hosts' give 0x7fc00000.  With the sign set, a
// box that straddles 0 on z (planes -inf and NaN) is missed; with it clear, z
// would drop out of the span and the box be entered.  Pinned against the
// device by tests/test_gpu_extreme.py
// (test_nan_slab_rays_agree_on_device_and_host) and against numpy, whatever
// the host, by tests/test_extreme_cpu.py.
inline float slab_dev(float x) { return x != x ? float_of((int32_t)0xffc00000u) : x; }

// spanBeginKepler / spanEndKepler (MathHelpers.cuh:454-552): float min / max
// per axis, then integer max / min of the bit patterns
inline float span_begin(float a0, float a1, float b0, float b1, float c0, float c1, float d)
{
    const int32_t zc = imax(imin(bits_of(slab_dev(c0)), bits_of(slab_dev(c1))), bits_of(d));
    return float_of(imax(imax(bits_of(fmin_dev(slab_dev(a0), slab_dev(a1))), bits_of(fmin_dev(slab_dev(b0), slab_dev(b1)))), zc));
}
inline float span_end(float a0, float a1, float b0, float b1, float c0, float c1, float d)
{
    const int32_t zc = imin(imax(bits_of(slab_dev(c0)), bits_of(slab_dev(c1))), bits_of(d));
    return float_of(imin(imin(bits_of(fmax_dev(slab_dev(a0), slab_dev(a1))), bits_of(fmax_dev(slab_dev(b0), slab_dev(b1)))), zc));
}

struct V3 { float x, y, z; };
inline V3 sub(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }

// intersectTriangle: true and (dist, u, v) where the reference returns them
inline bool intersect_triangle(V3 v1, V3 v2, V3 v3, V3 o, V3 d, float& dist, float& u, float& v)
{
    const V3 e1 = sub(v2, v1), e2 = sub(v3, v1);
    const V3 p = cross(d, e2);
    const float det = dot(e1, p);
    if (det > -kEps && det < kEps) return false;
    const float inv_det = 1.f / det;
    const V3 t = sub(o, v1);
    u = dot(t, p) * inv_det;
    if (u < 0.f || u > 1.f) return false;
    const V3 q = cross(t, e1);
    v = dot(d, q) * inv_det;
    if (v < 0.f || u + v > 1.f) return false;
    dist = dot(e2, q) * inv_det;
    return dist > kEps;
}

// One ray through a tree validate_flat accepted (`stack` holds its depth + 2 entries).
void walk(const float* bvh, const float* verts, V3 o, V3 d, float t0, bool any_hit, std::vector<int32_t>& stack,
          RayHit& out)
{
    float t = t0;
    out = RayHit{ t0, kRayMiss, 0.f, 0.f };
    size_t sp = 0;
    stack[0] = kWalkSentinel;
    int32_t leaf = 0;                             // first postponed leaf, non-negative if none
    int32_t node = 0;                             // the root
    const V3 inv = { 1.f / (std::fabs(d.x) > kEps ? d.x : kEps), 1.f / (std::fabs(d.y) > kEps ? d.y : kEps),
                     1.f / (std::fabs(d.z) > kEps ? d.z : kEps) };
    const V3 od = { o.x * inv.x, o.y * inv.y, o.z * inv.z };
    while (node != kWalkSentinel) {
        while ((uint32_t)node < (uint32_t)kWalkSentinel) {
            const float* n = bvh + 4 * (size_t)node;       // n0xy, n1xy, nz, child indices
            const float c0lox = n[0] * inv.x - od.x, c0hix = n[1] * inv.x - od.x;
            const float c0loy = n[2] * inv.y - od.y, c0hiy = n[3] * inv.y - od.y;
            const float c0loz = n[8] * inv.z - od.z, c0hiz = n[9] * inv.z - od.z;
            const float c1loz = n[10] * inv.z - od.z, c1hiz = n[11] * inv.z - od.z;
            const float c0min = span_begin(c0lox, c0hix, c0loy, c0hiy, c0loz, c0hiz, 0.f);
            const float c0max = span_end(c0lox, c0hix, c0loy, c0hiy, c0loz, c0hiz, 1e20f);
            const float c1lox = n[4] * inv.x - od.x, c1hix = n[5] * inv.x - od.x;
            const float c1loy = n[6] * inv.y - od.y, c1hiy = n[7] * inv.y - od.y;
            const float c1min = span_begin(c1lox, c1hix, c1loy, c1hiy, c1loz, c1hiz, 0.f);
            const float c1max = span_end(c1lox, c1hix, c1loy, c1hiy, c1loz, c1hiz, 1e20f);
            int32_t i0 = bits_of(n[12]), i1 = bits_of(n[13]);
            const bool swp = c1min < c0min;
            const bool tc0 = c0max >= c0min, tc1 = c1max >= c1min;
            if (!tc0 && !tc1) {
                node = stack[sp--];
            } else {
                node = tc0 ? i0 : i1;
                if (tc0 && tc1) {
                    if (swp) { const int32_t tmp = node; node = i1; i1 = tmp; }
                    stack[++sp] = i1;
                }
            }
            if (node < 0 && leaf >= 0) {          // postpone max 1
                leaf = node;
                node = stack[sp--];
            }
            if (leaf < 0) break;                  // the vote of a warp of one
        }
        while (leaf < 0) {
            for (size_t s = (size_t)~leaf;; s += 3) {
                const float* a = verts + 4 * s;
                if ((uint32_t)bits_of(a[0]) == 0x80000000u) break;
                float dist = 0.f, u = 0.f, v = 0.f;
                if (intersect_triangle({ a[0], a[1], a[2] }, { a[4], a[5], a[6] }, { a[8], a[9], a[10] }, o, d, dist, u, v) &&
                    dist < t) {
                    t = dist;
                    out = RayHit{ dist, (uint32_t)s, u, v };
                    if (any_hit) { out = RayHit{ 0.f, 0u, 0.f, 0.f }; return; }
                }
            }
            leaf = node;
            if (node < 0) node = stack[sp--];
        }
    }
}

inline bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

} // namespace

int flat_trace_rays(const float* bvh, size_t n_bvh_f4, const float* verts, size_t n_slots, const float* origins,
                    const float* dirs, const float* tmax, uint32_t n_rays, uint32_t mode, RayHit* hits)
{
    if (mode != RAYS_CLOSEST && mode != RAYS_ANY) return -1;
    if (n_rays != 0u && (!origins || !dirs || !hits)) return -1;
    if (!bvh || !verts) return -1;
    uint32_t depth = 0;
    if (validate_flat(bvh, n_bvh_f4, verts, n_slots, &depth, nullptr) != 0) return -4;
    std::vector<int32_t> stack((size_t)depth + 2u);
    for (uint32_t i = 0; i < n_rays; ++i) {
        const float* o = origins + 3 * (size_t)i;
        const float* d = dirs + 3 * (size_t)i;
        const float t0 = tmax ? tmax[i] : kRayNoHit;
        if (!finite3(o) || !finite3(d) || t0 != t0) {
            hits[i] = RayHit{ kRayNoHit, kRayMiss, 0.f, 0.f };
            continue;
        }
        walk(bvh, verts, { o[0], o[1], o[2] }, { d[0], d[1], d[2] }, t0, mode == RAYS_ANY, stack, hits[i]);
    }
    return 0;
}

} // namespace vr
