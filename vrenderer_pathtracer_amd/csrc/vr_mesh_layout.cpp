// vr_mesh_layout.cpp -- see vr_mesh_layout.hpp.
#include "vr_mesh_layout.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <queue>
#include <unordered_map>
#include <utility>

namespace vr {
namespace {

// Per compact triangle, the path from the root to its leaf (bit i = the child
// taken at depth i) under a leading 1 bit: the key the kernel's equal-t
// tie-break (ref_first) uses to find the two leaves' lowest common ancestor.
// Paths depend only on the tree's shape, so the node renumbering below keeps them.
void tri_paths(DeviceMesh& dm)
{
    dm.tpath.assign(std::max<size_t>(dm.tris.size() / 3, 1), 0ull);
    if (dm.nodes.empty()) return;
    struct Item { size_t off; unsigned long long bits; int depth; };
    std::vector<Item> st{ { 0, 0ull, 0 } };
    while (!st.empty()) {
        const Item it = st.back();
        st.pop_back();
        for (int ch = 0; ch < 2; ++ch) {
            int32_t idx;
            std::memcpy(&idx, &dm.nodes[it.off + 3].x + ch, 4);
            const unsigned long long bits = it.bits | ((unsigned long long)ch << it.depth);
            if (idx >= 0) { st.push_back({ (size_t)idx, bits, it.depth + 1 }); continue; }
            const uint32_t code = (uint32_t)~idx;
            const uint32_t first = code >> kLeafCountBits, count = code & ((1u << kLeafCountBits) - 1u);
            for (uint32_t t = first; t < first + count; ++t) dm.tpath[t] = (1ull << (it.depth + 1)) | bits;
        }
    }
}

// Renumbers the inner nodes so that node i is the i-th largest box by surface
// area (a parent always precedes its children; the root stays at 0).  The
// kernel keeps a prefix of this array in LDS: the boxes a random ray is most
// likely to enter.  Only addresses change -- every node keeps its boxes and
// child order, so the traversal visits the same nodes in the same order.
#ifndef VR_TOP_NODES
#define VR_TOP_NODES 1024
#endif
constexpr size_t kTopNodes = VR_TOP_NODES;    // >= any kernel's LDS node cache

void order_nodes_by_area(DeviceMesh& dm)
{
    const size_t n = dm.nodes.size() / 4;
    if (n == 0) return;
    auto child_area = [&](size_t node, int ch) {
        const vr4& a = dm.nodes[4 * node + ch];            // x and y extents of child ch
        const vr4& z = dm.nodes[4 * node + 2];
        const float dx = a.y - a.x, dy = a.w - a.z, dz = ch ? z.w - z.z : z.y - z.x;
        return dx * dy + dy * dz + dz * dx;
    };
    auto child = [&](size_t node, int ch) {
        int32_t idx;
        std::memcpy(&idx, &dm.nodes[4 * node + 3].x + ch, 4);
        return idx;
    };
    std::vector<int32_t> newoff(n, -1);
    std::vector<size_t> order;
    order.reserve(n);
    // the first kTop nodes: largest boxes first (the LDS-cached prefix)
    std::priority_queue<std::pair<float, int64_t>> pq;   // (area, -node): ties by address
    pq.push({ INFINITY, 0 });
    newoff[0] = 0;
    while (!pq.empty() && order.size() < kTopNodes) {
        const size_t node = (size_t)(-pq.top().second);
        pq.pop();
        newoff[node] = (int32_t)(4 * order.size());
        order.push_back(node);
        for (int ch = 0; ch < 2; ++ch) {
            const int32_t idx = child(node, ch);
            if (idx < 0 || newoff[idx / 4] != -1) continue;
            newoff[idx / 4] = -2;                          // queued
            pq.push({ child_area(node, ch), -(int64_t)(idx / 4) });
        }
    }
    // the rest: depth-first from the frontier, the two children of a node
    // placed side by side (a ray that enters one often enters the other, and
    // they share a cache line)
    std::vector<size_t> frontier;
    while (!pq.empty()) { frontier.push_back((size_t)(-pq.top().second)); pq.pop(); }
    std::sort(frontier.begin(), frontier.end(), [&](size_t a, size_t b) { return a < b; });
    std::vector<size_t> st;
    auto place = [&](size_t node) { newoff[node] = (int32_t)(4 * order.size()); order.push_back(node); };
    for (size_t f : frontier) {
        place(f);
        st.push_back(f);
        while (!st.empty()) {
            const size_t node = st.back();
            st.pop_back();
            size_t kids[2];
            int nk = 0;
            for (int ch = 0; ch < 2; ++ch) {
                const int32_t idx = child(node, ch);
                if (idx >= 0 && newoff[idx / 4] == -1) kids[nk++] = (size_t)(idx / 4);
            }
            for (int k = 0; k < nk; ++k) place(kids[k]);
            for (int k = nk - 1; k >= 0; --k) st.push_back(kids[k]);   // first child's subtree next
        }
    }
    std::vector<vr4> out(4 * order.size());
    for (size_t i = 0; i < order.size(); ++i) {
        for (int r = 0; r < 4; ++r) out[4 * i + r] = dm.nodes[4 * order[i] + r];
        for (int ch = 0; ch < 2; ++ch) {
            float* slot = &out[4 * i + 3].x + ch;
            int32_t idx;
            std::memcpy(&idx, slot, 4);
            if (idx >= 0) std::memcpy(slot, &newoff[idx / 4], 4);
        }
    }
    dm.nodes.swap(out);
}

// IEEE binary16 bits of x rounded toward -inf (down) or +inf (up), so the
// half box always contains the float box.  Out-of-range values become
// -inf / +inf on the outward side.
uint16_t half_bits_directed(float x, bool up)
{
    uint32_t u;
    std::memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const float ax = std::fabs(x);
    auto half_to_float = [](uint16_t h) {
        const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
        float f;
        if (e == 0) f = std::ldexp((float)m, -24);
        else if (e == 31) f = m ? NAN : INFINITY;
        else f = std::ldexp((float)(m | 0x400u), (int)e - 25);
        return s ? -f : f;
    };
    // truncation toward zero of |x| to half precision
    uint16_t mag;
    if (ax >= 65504.f) {
        mag = 0x7bffu;                                   // max finite
    } else if (ax < std::ldexp(1.f, -14)) {
        mag = (uint16_t)(ax / std::ldexp(1.f, -24));     // subnormal, truncated
    } else {
        int e;
        const float m = std::frexp(ax, &e);              // ax = m * 2^e, m in [0.5, 1)
        const uint32_t mant = (uint32_t)std::ldexp(m, 11) & 0x3ffu;   // 10 fraction bits, truncated
        mag = (uint16_t)(((uint32_t)(e - 1 + 15) << 10) | mant);
    }
    uint16_t h = (uint16_t)(sign | mag);
    // truncation moved |x| toward zero; step one ulp outward where needed
    const float hv = half_to_float(h);
    const bool below = hv < x, above = hv > x;
    if (up && below) h = sign ? (uint16_t)(h - 1) : (uint16_t)(h + 1);
    if (!up && above) h = sign ? (uint16_t)(h + 1) : (uint16_t)(h - 1);
    if ((h & 0x7fffu) == 0x7c00u || ((h & 0x7fffu) > 0x7c00u)) h = (uint16_t)((h & 0x8000u) | 0x7c00u);
    if (up && ax >= 65504.f && x > 0.f && half_to_float(h) < x) h = 0x7c00u;          // +inf
    if (!up && ax >= 65504.f && x < 0.f && half_to_float(h) > x) h = 0xfc00u;         // -inf
    return h;
}

// fp16 copy of the node array for the t-culled traversal: per node
// [c0.lo.x c0.hi.x c0.lo.y c0.hi.y c0.lo.z c0.hi.z c1.lo.x c1.hi.x]
// [c1.lo.y c1.hi.y c1.lo.z c1.hi.z idx0 idx1], lows rounded down and highs up.
void build_nodes16(DeviceMesh& dm)
{
    const size_t n = dm.nodes.size() / 4;
    dm.nodes16.assign(2 * n, vr4{ 0, 0, 0, 0 });
    for (size_t i = 0; i < n; ++i) {
        const vr4 n0 = dm.nodes[4 * i], n1 = dm.nodes[4 * i + 1], nz = dm.nodes[4 * i + 2], ni = dm.nodes[4 * i + 3];
        const float v[12] = { n0.x, n0.y, n0.z, n0.w, nz.x, nz.y, n1.x, n1.y, n1.z, n1.w, nz.z, nz.w };
        uint16_t h[16];
        for (int k = 0; k < 12; ++k) h[k] = half_bits_directed(v[k], (k & 1) != 0);
        std::memcpy(&h[12], &ni.x, 4);
        std::memcpy(&h[14], &ni.y, 4);
        std::memcpy(&dm.nodes16[2 * i], h, 32);
    }
}

} // namespace

bool to_device_layout(const float* bvh, size_t n_bvh_f4, const vr4* verts, const vr4* normals,
                      const vr4* tangents, const vr2* uvs, DeviceMesh& dm, std::string& why)
{
    // The input must be a tree (vr::validate_flat, which every upload runs
    // first, rejects a node or leaf run with two parents): each triangle then
    // has ONE root path, the key of the equal-t tie-break (tri_paths).  A
    // shared node or leaf is refused here too rather than merged, since a
    // merged copy would give its triangles the path of one parent only.
    dm.nodes.assign((const vr4*)bvh, (const vr4*)bvh + n_bvh_f4);
    std::vector<size_t> st{ 0 };
    std::vector<uint8_t> seen(n_bvh_f4 / 4, 0);
    std::unordered_map<int32_t, int> leaf_seen;
    while (!st.empty()) {
        const size_t off = st.back();
        st.pop_back();
        if (seen[off / 4]) { why = "flattened BVH is not a tree (a node has two parents)"; return false; }
        seen[off / 4] = 1;
        float* idxf = &dm.nodes[off + 3].x;
        for (int ch = 0; ch < 2; ++ch) {
            int32_t idx;
            std::memcpy(&idx, &idxf[ch], 4);
            if (idx >= 0) { st.push_back((size_t)idx); continue; }
            if (!leaf_seen.emplace(idx, 1).second) { why = "flattened BVH is not a tree (a leaf has two parents)"; return false; }
            const size_t first = dm.tris.size() / 3;
            size_t s = (size_t)(~idx), count = 0;
            for (;;) {
                uint32_t b;
                std::memcpy(&b, &verts[s].x, 4);
                if (b == 0x80000000u) break;
                dm.prim_id.push_back((uint32_t)s);
                for (int k = 0; k < 3; ++k) {
                    dm.tris.push_back(vr3{ verts[s + k].x, verts[s + k].y, verts[s + k].z });
                    dm.normals.push_back(normals[s + k]);
                    dm.tangents.push_back(tangents[s + k]);
                    dm.uvs.push_back(uvs[s + k]);
                }
                s += 3;
                ++count;
            }
            if (count >= (1u << kLeafCountBits)) { why = "leaf with >= 128 triangles"; return false; }
            if (first >= (1u << (31 - kLeafCountBits))) { why = "more than 16M triangle references"; return false; }
            const int32_t code = ~(int32_t)((first << kLeafCountBits) | count);
            std::memcpy(&idxf[ch], &code, 4);
        }
    }
    tri_paths(dm);
    order_nodes_by_area(dm);
    build_nodes16(dm);
    if (dm.tris.empty()) {
        dm.tris.push_back(vr3{ 0, 0, 0 });
        dm.normals.push_back(vr4{ 0, 0, 0, 0 });
        dm.tangents = dm.normals;
        dm.uvs.push_back(vr2{ 0, 0 });
        dm.prim_id.push_back(0u);
    }
    // The Moller-Trumbore edges are the same fp32 subtractions whichever side
    // performs them; precomputed, the triangle test reads v0 and both edges
    // and skips 6 VALU ops per test.  The face normal at shading keeps using
    // the vertices (v0 - v1 is not -(v1 - v0) for signed zeros).
    dm.tri_e.resize(dm.tris.size());
    for (size_t t = 0; t + 2 < dm.tris.size(); t += 3) {
        const vr3 a = dm.tris[t], b = dm.tris[t + 1], d = dm.tris[t + 2];
        dm.tri_e[t] = a;
        dm.tri_e[t + 1] = vr3{ b.x - a.x, b.y - a.y, b.z - a.z };
        dm.tri_e[t + 2] = vr3{ d.x - a.x, d.y - a.y, d.z - a.z };
    }
    return true;
}

bool device_to_flat(const std::vector<vr4>& dn, const std::vector<vr3>& dv, const std::vector<vr4>& dnrm,
                    const std::vector<vr4>& dtan, const std::vector<vr2>& duv, FlatMesh& out)
{
    const size_t dev_nodes = dn.size() / 4, dev_tris = dv.size() / 3, nv = dv.size();
    if (dev_nodes == 0 || dnrm.size() < nv || dtan.size() < nv || duv.size() < nv) return false;
    std::vector<vr4>&ob = out.bvh, &ov = out.verts, &on = out.normals, &ot = out.tangents;
    std::vector<vr2>& ou = out.uvs;
    ob.assign(4, vr4{ 0.f, 0.f, 0.f, 0.f });
    ov.clear(); on.clear(); ot.clear(); ou.clear();
    ov.reserve(nv + nv / 3); on.reserve(nv + nv / 3); ot.reserve(nv + nv / 3); ou.reserve(nv + nv / 3);
    uint32_t tb;
    const int32_t tbits = (int32_t)0x80000000;
    std::memcpy(&tb, &tbits, 4);
    float term;
    std::memcpy(&term, &tb, 4);
    std::vector<std::pair<size_t, size_t>> stack{ { 0, 0 } };   // (device node, output float4 offset)
    while (!stack.empty()) {
        const size_t node = stack.back().first, idx = stack.back().second;
        stack.pop_back();
        int32_t indices[2];
        for (int i = 0; i < 2; ++i) {
            int32_t ci;
            std::memcpy(&ci, &dn[4 * node + 3].x + i, 4);
            if (ci >= 0) {
                if ((size_t)ci / 4 >= dev_nodes || ob.size() > dn.size()) return false;
                indices[i] = (int32_t)ob.size();
                stack.push_back({ (size_t)ci / 4, ob.size() });
                ob.resize(ob.size() + 4, vr4{ 0.f, 0.f, 0.f, 0.f });
                continue;
            }
            const uint32_t code = (uint32_t)~ci;
            const size_t first = code >> kLeafCountBits, count = code & ((1u << kLeafCountBits) - 1u);
            if (first + count > dev_tris) return false;
            indices[i] = ~(int32_t)ov.size();
            for (size_t s = 3 * first; s < 3 * (first + count); ++s) {
                ov.push_back(vr4{ dv[s].x, dv[s].y, dv[s].z, 0.f });
                on.push_back(dnrm[s]);
                ot.push_back(dtan[s]);
                ou.push_back(duv[s]);
            }
            ov.push_back(vr4{ term, 0.f, 0.f, 0.f });
            ot.push_back(vr4{ term, 0.f, 0.f, 0.f });
            on.push_back(vr4{ term, 0.f, 0.f, 0.f });
            ou.push_back(vr2{ term, 0.f });
        }
        ob[idx + 0] = dn[4 * node + 0];
        ob[idx + 1] = dn[4 * node + 1];
        ob[idx + 2] = dn[4 * node + 2];
        float f0, f1;
        std::memcpy(&f0, &indices[0], 4);
        std::memcpy(&f1, &indices[1], 4);
        ob[idx + 3] = vr4{ f0, f1, 0.f, 0.f };
    }
    return true;
}

} // namespace vr
