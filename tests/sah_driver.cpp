// The device SAH builder's decisions (csrc/vr_devsah.hpp) run on the host: the
// level loop of vr_devsah.hip, serially, with a stable partition, then the
// LIFO flatten of vr::build_flat.  Prints, per mesh file given, the number of
// float4 of the flattened bvh array, the tree's depth and an FNV-1a digest of
// the array's 32-bit words.
// Mesh file: u32 n_verts, n_tris, max_leaf; f32 positions[3 n_verts]; u32 tris[3 n_tris].
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vr_devsah.hpp"

using namespace vr;

struct Item { uint32_t first, count, parent, which; };
struct Node { SahBox box[2]; int32_t child[2]; };          // child >= 0: node, < 0: ~leaf
struct Leaf { uint32_t first, count; };

static int run(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return 1;
    uint32_t hdr[3];
    if (std::fread(hdr, 4, 3, f) != 3) return 1;
    const uint32_t n_verts = hdr[0], n_tris = hdr[1], max_leaf = hdr[2];
    std::vector<float> pos(3 * (size_t)n_verts);
    std::vector<uint32_t> tris(3 * (size_t)n_tris);
    if (std::fread(pos.data(), 4, pos.size(), f) != pos.size()) return 1;
    if (std::fread(tris.data(), 4, tris.size(), f) != tris.size()) return 1;
    std::fclose(f);

    std::vector<SahBox> tribox(n_tris);
    for (uint32_t t = 0; t < n_tris; ++t) {
        SahBox b = sah_empty();
        for (int k = 0; k < 3; ++k) {
            const float* p = &pos[3 * (size_t)tris[3 * (size_t)t + k]];
            sah_grow(b, SahBox{ { p[0], p[1], p[2] }, { p[0], p[1], p[2] } });
        }
        tribox[t] = b;
    }
    const uint32_t n = n_tris < 2u ? 2u : n_tris;          // a single triangle is stored twice
    std::vector<uint32_t> refs(n);
    for (uint32_t k = 0; k < n; ++k) refs[k] = k < n_tris ? k : 0u;

    std::vector<Node> nodes;
    std::vector<Leaf> leaves;
    std::vector<Item> items{ { 0u, n, 0u, 0u } }, next;
    uint32_t depth = 0;
    for (uint32_t level = 0; !items.empty(); ++level) {
        next.clear();
        for (const Item& im : items) {
            const bool root = level == 0u;
            SahBox b = sah_empty(), cb = sah_empty();
            for (uint32_t i = im.first; i < im.first + im.count; ++i) {
                const SahBox& t = tribox[refs[i]];
                sah_grow(b, t);
                SahBox c;
                for (int a = 0; a < 3; ++a) c.lo[a] = c.hi[a] = sah_centroid(t.lo[a], t.hi[a]);
                sah_grow(cb, c);
            }
            double best = __builtin_inf();
            uint32_t best_key = kSahNoKey, best_nl = 0;
            const bool early = sah_early_leaf(im.count, level, root);
            if (!early) {
                for (int a = 2; a >= 0; --a) {                 // any order: ties go to the lower key
                    const float ext = cb.hi[a] - cb.lo[a];
                    if (!(ext > 0.f)) continue;
                    std::vector<SahBox> bb(kSahBins, sah_empty());
                    std::vector<uint32_t> bc(kSahBins, 0u);
                    for (uint32_t i = im.first; i < im.first + im.count; ++i) {
                        const SahBox& t = tribox[refs[i]];
                        const int k = sah_bin(sah_centroid(t.lo[a], t.hi[a]), cb.lo[a], ext);
                        sah_grow(bb[k], t);
                        ++bc[k];
                    }
                    std::vector<SahBox> lb(kSahBins, sah_empty());      // bins 0..k
                    std::vector<uint32_t> lc(kSahBins, 0u);
                    for (int k = 0; k < kSahBins; ++k) {
                        if (k) { lb[k] = lb[k - 1]; lc[k] = lc[k - 1]; }
                        sah_grow(lb[k], bb[k]);
                        lc[k] += bc[k];
                    }
                    SahBox R = sah_empty();                             // bins k+1..127
                    uint32_t nr = 0;
                    for (int k = kSahBins - 2; k >= 0; --k) {
                        sah_grow(R, bb[k + 1]);
                        nr += bc[k + 1];
                        const SahBox& L = lb[k];
                        const uint32_t nl = lc[k];
                        if (nl == 0u || nr == 0u) continue;
                        const double cost = sah_cost(sah_area(L), nl, sah_area(R), nr);
                        if (sah_better(cost, sah_key(a, k), best, best_key)) { best = cost; best_key = sah_key(a, k); best_nl = nl; }
                    }
                }
            }
            const bool has_axis = best_key != kSahNoKey;
            const bool split = !early && (root || !sah_want_leaf(im.count, max_leaf, has_axis, best, sah_area(b)));
            int32_t code;
            if (split) {
                const uint32_t id = (uint32_t)nodes.size();
                nodes.push_back(Node{});
                uint32_t nl = sah_median(im.count);
                if (has_axis) {
                    const int a = (int)(best_key / kSahBins), ks = (int)(best_key % kSahBins);
                    const float ext = cb.hi[a] - cb.lo[a];
                    auto mid = std::stable_partition(refs.begin() + im.first, refs.begin() + im.first + im.count, [&](uint32_t t) {
                        return sah_bin(sah_centroid(tribox[t].lo[a], tribox[t].hi[a]), cb.lo[a], ext) <= ks;
                    });
                    nl = (uint32_t)(mid - (refs.begin() + im.first));
                    if (nl != best_nl) return 2;
                }
                next.push_back({ im.first, nl, id, 0u });
                next.push_back({ im.first + nl, im.count - nl, id, 1u });
                code = (int32_t)id;
                depth = level + 1u;
            } else {
                code = ~(int32_t)leaves.size();
                leaves.push_back({ im.first, im.count });
            }
            if (!root) {
                nodes[im.parent].box[im.which] = b;
                nodes[im.parent].child[im.which] = code;
            }
        }
        items.swap(next);
    }

    // the LIFO flatten of vr::build_flat (vr_bvh.cpp:490-535)
    std::vector<float> bvh(16, 0.f);
    size_t n_slots = 0;
    std::vector<std::pair<uint32_t, size_t>> stack{ { 0u, 0 } };
    while (!stack.empty()) {
        const uint32_t ni = stack.back().first;
        const size_t idx = stack.back().second;
        stack.pop_back();
        int32_t indices[2];
        for (int i = 0; i < 2; ++i) {
            const int32_t c = nodes[ni].child[i];
            if (c >= 0) {
                indices[i] = (int32_t)(bvh.size() / 4);
                stack.push_back({ (uint32_t)c, bvh.size() / 4 });
                bvh.resize(bvh.size() + 16, 0.f);
            } else {
                indices[i] = ~(int32_t)n_slots;
                n_slots += 3 * (size_t)leaves[~c].count + 1;
            }
        }
        const SahBox &b0 = nodes[ni].box[0], &b1 = nodes[ni].box[1];
        const float row[12] = { b0.lo[0], b0.hi[0], b0.lo[1], b0.hi[1], b1.lo[0], b1.hi[0], b1.lo[1], b1.hi[1],
                                b0.lo[2], b0.hi[2], b1.lo[2], b1.hi[2] };
        std::memcpy(&bvh[4 * idx], row, sizeof(row));
        std::memcpy(&bvh[4 * idx + 12], indices, 8);
    }
    unsigned long long h = 0xcbf29ce484222325ull;
    for (float v : bvh) {
        uint32_t w;
        std::memcpy(&w, &v, 4);
        h = (h ^ w) * 0x100000001b3ull;
    }
    std::printf("%zu %u %016llx\n", bvh.size() / 4, depth, h);
    return 0;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; ++i)
        if (int rc = run(argv[i])) { std::fprintf(stderr, "%s: error %d\n", argv[i], rc); return rc; }
    return 0;
}
