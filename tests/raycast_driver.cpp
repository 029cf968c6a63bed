// Stand-alone driver of the host ray query (vr_raycast.cpp) for a sanitizer
// build (tests/test_ray_query_sanitize.py): rays through a built tree, through
// a chain tree 40 levels deep, through trees over meshes at the extremes of
// float with rays of every magnitude, and at malformed trees, which must be refused
// with VRHIP_ERR_BVH (-4).  Prints "raycast ok=<accepted> rejected=<refused>"
// and exits non-zero when a tree lands on the wrong side.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vr_bvh.hpp"
#include "vr_rayquery.hpp"

namespace {

uint32_t g_seed = 12345u;
float rnd(float lo, float hi)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return lo + (hi - lo) * (float)(g_seed >> 8) / 16777216.f;
}

float bits_to_float(int32_t i) { float f; std::memcpy(&f, &i, 4); return f; }

struct Flat { std::vector<float> bvh, verts; };       // float4 rows

// scale > 0: every coordinate times scale, clipped to +-3.4e38 (1e37: the
// extent and the centroids overflow).  scale == 0: each triangle by its own
// 10^U(-30, 30), a tree next to the builder's depth cap.
Flat built_tree(uint32_t n_tris, uint32_t max_leaf, double scale = 1.0)
{
    std::vector<float> pos;
    std::vector<uint32_t> tris;
    for (uint32_t t = 0; t < n_tris; ++t) {
        const float c[3] = { rnd(-30, 30), rnd(-30, 30), rnd(-30, 30) };
        const double s = scale > 0.0 ? scale : std::pow(10.0, (double)rnd(-30, 30));
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) pos.push_back((float)std::fmax(-3.4e38, std::fmin(3.4e38, s * (double)(c[a] + rnd(-4, 4)))));
        for (uint32_t v = 0; v < 3; ++v) tris.push_back(3 * t + v);
    }
    vr::FlatMesh m;
    if (vr::build_flat(pos.data(), nullptr, nullptr, nullptr, 3 * n_tris, tris.data(), n_tris, max_leaf, m) != 0) return {};
    Flat f;
    f.bvh.assign((const float*)m.bvh.data(), (const float*)m.bvh.data() + 4 * m.bvh.size());
    f.verts.assign((const float*)m.verts.data(), (const float*)m.verts.data() + 4 * m.verts.size());
    return f;
}

// node i: triangle i in a leaf (child 0) and node i + 1 (child 1); the last node two leaves
Flat chain_tree(int levels)
{
    const int T = levels + 1;
    Flat f;
    f.verts.assign((size_t)16 * T, 0.f);
    std::vector<float> lo((size_t)3 * T), hi((size_t)3 * T);
    for (int t = 0; t < T; ++t) {
        for (int a = 0; a < 3; ++a) { lo[3 * t + a] = INFINITY; hi[3 * t + a] = -INFINITY; }
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) {
                const float x = rnd(-1, 1) + (a == 0 ? 3.f * (float)t : 0.f);
                f.verts[16 * t + 4 * v + a] = x;
                lo[3 * t + a] = std::fmin(lo[3 * t + a], x);
                hi[3 * t + a] = std::fmax(hi[3 * t + a], x);
            }
        f.verts[16 * t + 12] = bits_to_float((int32_t)0x80000000);
    }
    f.bvh.assign((size_t)16 * levels, 0.f);
    for (int i = 0; i < levels; ++i) {
        float rlo[3] = { INFINITY, INFINITY, INFINITY }, rhi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (int t = i + 1; t < T; ++t)
            for (int a = 0; a < 3; ++a) { rlo[a] = std::fmin(rlo[a], lo[3 * t + a]); rhi[a] = std::fmax(rhi[a], hi[3 * t + a]); }
        float* n = &f.bvh[16 * i];
        n[0] = lo[3 * i]; n[1] = hi[3 * i]; n[2] = lo[3 * i + 1]; n[3] = hi[3 * i + 1];
        n[4] = rlo[0]; n[5] = rhi[0]; n[6] = rlo[1]; n[7] = rhi[1];
        n[8] = lo[3 * i + 2]; n[9] = hi[3 * i + 2]; n[10] = rlo[2]; n[11] = rhi[2];
        n[12] = bits_to_float(~(int32_t)(4 * i));
        n[13] = bits_to_float(i + 1 < levels ? (int32_t)(4 * (i + 1)) : ~(int32_t)(4 * (i + 1)));
    }
    return f;
}

// rays aimed at triangles, random rays, axis-aligned and non-finite ones; both modes, with and without tmax.
// extreme: origin and direction magnitudes drawn from the whole range of float (1e-45 .. 3e38), zero and
// -0 directions among them, and tmax from {1e20, inf, 0, -1, 1e-30, 3e38, 1, -inf}
int trace(const Flat& f, uint32_t n_rays, uint32_t* hits_out, bool extreme = false)
{
    const size_t n_slots = f.verts.size() / 4;
    std::vector<float> o(3 * (size_t)n_rays), d(3 * (size_t)n_rays), tmax(n_rays);
    const float ladder[9] = { 1e-45f, 1e-38f, 1e-30f, 1e-10f, 1.f, 1e10f, 1e19f, 1e30f, 3e38f };
    const float bounds[8] = { 1e20f, INFINITY, 0.f, -1.f, 1e-30f, 3e38f, 1.f, -INFINITY };
    for (uint32_t i = 0; i < n_rays; ++i) {
        const float* v = &f.verts[4 * (size_t)(g_seed % (n_slots ? n_slots : 1))];
        const float om = extreme ? ladder[(g_seed >> 9) % 9u] : 80.f, dm = extreme ? ladder[(g_seed >> 17) % 9u] : 1.f;
        for (int a = 0; a < 3; ++a) {
            o[3 * i + a] = rnd(-om, om);
            d[3 * i + a] = i % 3 == 0 ? (extreme ? dm * rnd(0.5f, 1.f) * (v[a] < o[3 * i + a] ? -1.f : 1.f) : v[a] - o[3 * i + a])
                           : i % 3 == 1 ? rnd(-dm, dm) : (i % 2 ? -0.f : 0.f);
        }
        if (i % 3 == 2 && i % 5 != 0) d[3 * i + i % 3] = dm;    // every fifth of these keeps its all-zero direction
        if (!extreme) {
            if (i % 17 == 0) o[3 * i] = NAN;
            if (i % 19 == 0) d[3 * i + 1] = INFINITY;
        }
        tmax[i] = extreme ? bounds[i % 8u] : i % 23 == 0 ? NAN : rnd(0.1f, 3.f);
    }
    std::vector<vr::RayHit> hits(n_rays);
    uint32_t n_hit = 0;
    for (uint32_t mode = 0; mode < 2; ++mode)
        for (int with_tmax = 0; with_tmax < 2; ++with_tmax) {
            const int rc = vr::flat_trace_rays(f.bvh.data(), f.bvh.size() / 4, f.verts.data(), n_slots, o.data(), d.data(),
                                               with_tmax ? tmax.data() : nullptr, n_rays, mode, hits.data());
            if (rc != 0) return rc;
            for (const vr::RayHit& h : hits) n_hit += h.prim != vr::kRayMiss;
        }
    if (hits_out) *hits_out = n_hit;
    return 0;
}

} // namespace

int main()
{
    int ok = 0, rejected = 0, wrong = 0;
    auto expect = [&](const Flat& f, bool valid, const char* what, bool need_hits = true, bool extreme = false) {
        uint32_t n_hit = 0;
        const int rc = trace(f, 600, &n_hit, extreme);
        if (rc == 0) ++ok; else ++rejected;
        if (valid ? (rc != 0 || (need_hits && n_hit == 0)) : rc != -4) {
            std::fprintf(stderr, "%s: rc %d, %u hits\n", what, rc, n_hit);
            ++wrong;
        }
    };
    const Flat built = built_tree(300, 2), one = built_tree(1, 1), chain = chain_tree(40);
    expect(built, true, "built tree");
    expect(built_tree(65, 3), true, "built tree, leaves of 3");
    expect(one, true, "one triangle", false);       // rays aimed at its corners may graze it
    expect(chain, true, "chain tree");
    // the extremes of float: no hit is required, only that every operation is defined
    expect(built, true, "built tree, extreme rays", false, true);
    expect(built_tree(200, 2, 1e37), true, "huge mesh, extreme rays", false, true);
    expect(built_tree(200, 1, 0.0), true, "wide mesh, extreme rays", false, true);
    expect(built_tree(200, 3, 1e18), true, "big mesh, extreme rays", false, true);

    Flat bad = built;                                  // a child offset out of range
    bad.bvh[13] = bits_to_float((int32_t)(bad.bvh.size() / 4 + 4));
    expect(bad, false, "child offset out of range");
    bad = built;                                       // an offset that is no node boundary
    bad.bvh[12] = bits_to_float(6);
    expect(bad, false, "misaligned child offset");
    bad = built;                                       // a leaf run past the end of the vertices
    bad.bvh[12] = bits_to_float(~(int32_t)(bad.verts.size() / 4 + 7));
    expect(bad, false, "leaf slot out of range");
    bad = built;                                       // no terminator: every run reaches the end
    for (size_t s = 0; s < bad.verts.size() / 4; ++s) {
        uint32_t b;
        std::memcpy(&b, &bad.verts[4 * s], 4);
        if (b == 0x80000000u) bad.verts[4 * s] = 1.f;
    }
    expect(bad, false, "missing terminator");
    bad = chain;                                       // a cycle: the deepest node points back at the root
    bad.bvh[16 * 39 + 13] = bits_to_float(0);
    expect(bad, false, "cycle");
    bad = chain;                                       // a node with two parents
    bad.bvh[16 * 5 + 12] = bits_to_float(4 * 20);
    expect(bad, false, "node with two parents");
    bad = built;                                       // a truncated node array
    bad.bvh.resize(bad.bvh.size() - 16);
    expect(bad, false, "truncated node array");
    bad = Flat{};                                      // a root that is its own child, one slot of vertices
    bad.bvh.assign(16, 0.f);
    bad.verts.assign(4, 1.f);
    expect(bad, false, "self-referencing root");

    // refused arguments
    vr::RayHit h{};
    const float z[3] = { 0.f, 0.f, 1.f };
    if (vr::flat_trace_rays(built.bvh.data(), built.bvh.size() / 4, built.verts.data(), built.verts.size() / 4, z, z, nullptr,
                            1, 2, &h) != -1 ||
        vr::flat_trace_rays(built.bvh.data(), built.bvh.size() / 4, built.verts.data(), built.verts.size() / 4, nullptr, z,
                            nullptr, 1, 0, &h) != -1 ||
        vr::flat_trace_rays(built.bvh.data(), built.bvh.size() / 4, built.verts.data(), built.verts.size() / 4, nullptr,
                            nullptr, nullptr, 0, 0, nullptr) != 0)
        ++wrong;
    std::printf("raycast ok=%d rejected=%d\n", ok, rejected);
    return wrong ? 1 : 0;
}
