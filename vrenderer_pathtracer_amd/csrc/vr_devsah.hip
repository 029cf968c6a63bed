// vr_devsah.hip -- the host's binned-SAH tree built on the device (gfx950),
// declared in vr_devsah.hpp.
//
// Level-synchronous and top-down.  At each level the active nodes ("items")
// own disjoint contiguous ranges of the reference array, each range in
// ascending triangle index.  Per level:
//   1. bounds   the box and centroid box of every large item (> kSahSmall
//               references): per-thread runs, a wave reduction where the wave
//               is in one item, then integer min/max atomics;
//   2. bin      the 3 x 128 bins of every large item: in LDS where a block's
//               chunk lies in one item, then integer atomics to the item's
//               global bins;
//   3. node     one wave64 per item.  A small item is held a reference per
//               lane: bounds by wave reduction, and each lane evaluates the
//               split after its own bin (an empty bin repeats its predecessor's
//               cost, and a repeated cost never wins under strict <).  A large
//               item is swept from its global bins, two bins per lane, and the
//               bins are left empty for the next level.  Either way the wave
//               takes the argmin with ties to the lower (axis, bin) and applies
//               the host's leaf rule;
//   4. flag     per reference of a splitting item: does it go left;
//   5. two exclusive scans (rocPRIM): of the flags over the references (the
//               stable partition's ranks) and of the split decisions over the
//               items (the children's item and node numbers);
//   6. children per item: a leaf writes its code, box and root paths, a split
//               takes its node number and makes two items for the next level;
//   7. scatter  per reference: its place in the next level's order.
// One counter is read back per level (the number of splits).  Kernel
// boundaries give all ordering; no workgroup waits for another.  No result
// depends on scheduling: the only atomics are integer min, max, add and or.
// Emission is the stage shared with the Morton builder (vr_devmesh_dev.hpp
// emit_mesh): the root first, the other nodes by descending area.
#include <cstring>                                // rocPRIM's iterators call memset without including it
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "vr_devmesh_dev.hpp"
#include "vr_devsah.hpp"

namespace vr {
namespace {

constexpr int kChunk = 8;                         // references per thread in the bounds and bin kernels
constexpr uint32_t kInactive = 0xffffffffu;       // a reference whose leaf is made
constexpr uint32_t kNoAxis = 3u;
constexpr int kBinFields = 7;                     // lo xyz, hi xyz (ordered images), count

struct Item {                                     // an active node of the current level
    uint32_t first, count;                        // its range of the reference array
    uint32_t parent;                              // node number of its parent
    uint32_t pad;
    unsigned long long path;                      // root path under a leading 1
};
struct ItemState {
    int32_t b[6], cb[6];                          // box and centroid box, ordered images, lo xyz then hi xyz
    uint32_t split, axis, k, nl;                  // decision: axis kNoAxis = the median of the current order
};
struct Control { uint32_t splits; uint32_t pad[3]; };

__device__ __forceinline__ int32_t enc(float f) { return sah_ordered(__float_as_int(f)); }
__device__ __forceinline__ float dec(int32_t i) { return __int_as_float(sah_ordered(i)); }

__device__ __forceinline__ SahBox centroid_box(const SahBox& t)
{
    SahBox c;
    for (int a = 0; a < 3; ++a) c.lo[a] = c.hi[a] = sah_centroid(t.lo[a], t.hi[a]);
    return c;
}
__device__ __forceinline__ SahBox dec_box(const int32_t* p)
{
    return { { dec(p[0]), dec(p[1]), dec(p[2]) }, { dec(p[3]), dec(p[4]), dec(p[5]) } };
}
__device__ __forceinline__ SahBox shfl_box(const SahBox& b, int src)
{
    SahBox r;
    for (int a = 0; a < 3; ++a) { r.lo[a] = __shfl(b.lo[a], src); r.hi[a] = __shfl(b.hi[a], src); }
    return r;
}
// union over the wave, in every lane
__device__ __forceinline__ SahBox wave_union(SahBox b)
{
    for (int o = 32; o > 0; o >>= 1) {
        SahBox t;
        for (int a = 0; a < 3; ++a) { t.lo[a] = __shfl_xor(b.lo[a], o); t.hi[a] = __shfl_xor(b.hi[a], o); }
        sah_grow(b, t);
    }
    return b;
}
__device__ __forceinline__ void fail(DevBuildStatus* st) { atomicOr(&st->flags, DEVBVH_INTERNAL); }

// ---- triangle boxes, validation, the first order ------------------------------
__global__ __launch_bounds__(kBlock) void sah_tris_kernel(const float* __restrict__ pos, uint32_t n_verts,
                                                          const uint32_t* __restrict__ tris, uint32_t n_tris,
                                                          uint32_t n_refs, float4* __restrict__ tribox,
                                                          uint32_t* __restrict__ refs, uint32_t* __restrict__ node_of,
                                                          DevBuildStatus* st)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_refs) return;
    const uint32_t t = k < n_tris ? k : 0u;       // a single triangle is stored twice
    refs[k] = t;
    node_of[k] = 0u;
    if (k >= n_tris) return;
    DevBox b;
    const uint32_t flags = triangle_box(pos, n_verts, tris, t, b);
    store_box(tribox, t, b);
    if (flags) atomicOr(&st->flags, flags);
}

__global__ __launch_bounds__(kBlock) void sah_fill_bins_kernel(int32_t* __restrict__ bins, size_t n_slots)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_slots * 3u * kBinFields * kSahBins) return;
    const uint32_t f = (uint32_t)(i / kSahBins) % kBinFields;
    bins[i] = f < 3u ? enc(__builtin_inff()) : f < 6u ? enc(-__builtin_inff()) : 0;
}

__global__ __launch_bounds__(kBlock) void sah_root_kernel(Item* items, uint32_t n_refs)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) items[0] = Item{ 0u, n_refs, 0u, 0u, 1ull };
}

__global__ __launch_bounds__(kBlock) void sah_init_items_kernel(uint32_t n_items, ItemState* __restrict__ state,
                                                                const DevBuildStatus* st)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_items || st->flags != 0u) return;
    ItemState s;
    for (int a = 0; a < 3; ++a) {
        s.b[a] = s.cb[a] = enc(__builtin_inff());
        s.b[3 + a] = s.cb[3 + a] = enc(-__builtin_inff());
    }
    s.split = 0u; s.axis = kNoAxis; s.k = 0u; s.nl = 0u;
    state[i] = s;
}

// ---- 1. bounds of the large items ----------------------------------------------
__device__ __forceinline__ void flush_bounds(ItemState* state, uint32_t item, const SahBox& b, const SahBox& cb)
{
    for (int a = 0; a < 3; ++a) {
        atomicMin(&state[item].b[a], enc(b.lo[a]));
        atomicMax(&state[item].b[3 + a], enc(b.hi[a]));
        atomicMin(&state[item].cb[a], enc(cb.lo[a]));
        atomicMax(&state[item].cb[3 + a], enc(cb.hi[a]));
    }
}

__global__ __launch_bounds__(kBlock) void sah_bounds_kernel(uint32_t n_refs, uint32_t n_items,
                                                            const uint32_t* __restrict__ refs,
                                                            const uint32_t* __restrict__ node_of,
                                                            const Item* __restrict__ items,
                                                            const float4* __restrict__ tribox, ItemState* state,
                                                            DevBuildStatus* st)
{
    if (st->flags != 0u) return;
    const size_t base = (size_t)blockIdx.x * kBlock * kChunk;
    uint32_t cur = kInactive;
    SahBox b = sah_empty(), cb = sah_empty();
    for (int it = 0; it < kChunk; ++it) {
        const size_t i = base + (size_t)it * kBlock + threadIdx.x;
        uint32_t item = i < n_refs ? node_of[i] : kInactive;
        if (item != kInactive && (item >= n_items || items[item].count <= kSahSmall)) item = kInactive;
        if (item == kInactive) continue;
        if (item != cur) {
            if (cur != kInactive) flush_bounds(state, cur, b, cb);
            cur = item; b = sah_empty(); cb = sah_empty();
        }
        const SahBox t = load_box(tribox, refs[i]);
        sah_grow(b, t);
        sah_grow(cb, centroid_box(t));
    }
    // the whole wave in one item: one set of atomics for the wave
    const uint32_t lead = __shfl(cur, 0);
    if (__all(cur == lead)) {
        if (lead == kInactive) return;
        b = wave_union(b); cb = wave_union(cb);
        if ((threadIdx.x & 63) == 0) flush_bounds(state, lead, b, cb);
    } else if (cur != kInactive) {
        flush_bounds(state, cur, b, cb);
    }
}

// ---- 2. bins of the large items -------------------------------------------------
__device__ __forceinline__ size_t bin_at(uint32_t slot, int axis, int field, int k)
{
    return (((size_t)slot * 3u + axis) * kBinFields + field) * kSahBins + k;
}

__global__ __launch_bounds__(kBlock) void sah_bin_kernel(uint32_t n_refs, uint32_t n_items, uint32_t n_slots,
                                                         const uint32_t* __restrict__ refs,
                                                         const uint32_t* __restrict__ node_of,
                                                         const Item* __restrict__ items,
                                                         const ItemState* __restrict__ state,
                                                         const float4* __restrict__ tribox, int32_t* bins,
                                                         DevBuildStatus* st)
{
    __shared__ int32_t lbin[3 * kBinFields * kSahBins];            // 10.5 KB
    if (st->flags != 0u) return;
    const size_t base = (size_t)blockIdx.x * kBlock * kChunk;
    size_t last = base + (size_t)kBlock * kChunk - 1;
    if (last >= n_refs) last = n_refs - 1u;
    // item ranges are contiguous, so a chunk that starts and ends in one item lies in it
    const uint32_t i0 = node_of[base], i1 = node_of[last];
    const bool one = i0 != kInactive && i0 == i1 && i0 < n_items && items[i0].count > kSahSmall;
    if (one) {
        for (int j = threadIdx.x; j < 3 * kBinFields * kSahBins; j += kBlock) {
            const int f = (j / kSahBins) % kBinFields;
            lbin[j] = f < 3 ? enc(__builtin_inff()) : f < 6 ? enc(-__builtin_inff()) : 0;
        }
        __syncthreads();
    }
    for (int it = 0; it < kChunk; ++it) {
        const size_t i = base + (size_t)it * kBlock + threadIdx.x;
        if (i >= n_refs) break;
        const uint32_t item = one ? i0 : node_of[i];
        if (item == kInactive || item >= n_items) continue;
        const Item im = items[item];
        if (im.count <= kSahSmall) continue;
        const uint32_t slot = im.first / (kSahSmall + 1u);
        if (slot >= n_slots) { fail(st); continue; }
        const SahBox cb = dec_box(state[item].cb);
        const SahBox t = load_box(tribox, refs[i]);
        for (int a = 0; a < 3; ++a) {
            const float ext = cb.hi[a] - cb.lo[a];
            if (!(ext > 0.f)) continue;
            const int k = sah_bin(sah_centroid(t.lo[a], t.hi[a]), cb.lo[a], ext);
            if (one) {
                int32_t* p = &lbin[(a * kBinFields) * kSahBins + k];
                for (int c = 0; c < 3; ++c) {
                    atomicMin(p + c * kSahBins, enc(t.lo[c]));
                    atomicMax(p + (3 + c) * kSahBins, enc(t.hi[c]));
                }
                atomicAdd(p + 6 * kSahBins, 1);
            } else {
                for (int c = 0; c < 3; ++c) {
                    atomicMin(&bins[bin_at(slot, a, c, k)], enc(t.lo[c]));
                    atomicMax(&bins[bin_at(slot, a, 3 + c, k)], enc(t.hi[c]));
                }
                atomicAdd(&bins[bin_at(slot, a, 6, k)], 1);
            }
        }
    }
    if (one) {
        __syncthreads();
        const uint32_t slot = items[i0].first / (kSahSmall + 1u);
        if (slot >= n_slots) return;
        for (int j = threadIdx.x; j < 3 * kSahBins; j += kBlock) {
            const int a = j / kSahBins, k = j % kSahBins;
            const int32_t* p = &lbin[(a * kBinFields) * kSahBins + k];
            const int32_t cnt = p[6 * kSahBins];
            if (cnt == 0) continue;
            for (int c = 0; c < 3; ++c) {
                atomicMin(&bins[bin_at(slot, a, c, k)], p[c * kSahBins]);
                atomicMax(&bins[bin_at(slot, a, 3 + c, k)], p[(3 + c) * kSahBins]);
            }
            atomicAdd(&bins[bin_at(slot, a, 6, k)], cnt);
        }
    }
}

// ---- 3. the decision, one wave per item ------------------------------------------
struct Best { double cost; uint32_t key, nl; };

__device__ __forceinline__ void consider(Best& best, const SahBox& L, uint32_t nl, const SahBox& R, uint32_t nr,
                                         int axis, int k)
{
    if (nl == 0u || nr == 0u) return;
    const double cost = sah_cost(sah_area(L), nl, sah_area(R), nr);
    const uint32_t key = sah_key(axis, k);
    if (sah_better(cost, key, best.cost, best.key)) { best.cost = cost; best.key = key; best.nl = nl; }
}
__device__ __forceinline__ Best wave_best(Best b)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double c = __shfl_xor(b.cost, o);
        const uint32_t key = __shfl_xor(b.key, o), nl = __shfl_xor(b.nl, o);
        if (sah_better(c, key, b.cost, b.key)) { b.cost = c; b.key = key; b.nl = nl; }
    }
    return b;
}

__global__ __launch_bounds__(kBlock) void sah_node_kernel(uint32_t n_items, uint32_t n_refs, uint32_t n_slots,
                                                          uint32_t level, uint32_t max_leaf,
                                                          const uint32_t* __restrict__ refs,
                                                          const Item* __restrict__ items,
                                                          const float4* __restrict__ tribox, ItemState* state,
                                                          int32_t* bins, uint32_t* __restrict__ isplit,
                                                          DevBuildStatus* st)
{
    if (st->flags != 0u) return;
    const uint32_t item = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= n_items) return;                  // wave-uniform
    const Item im = items[item];
    const bool root = level == 0u;
    if ((size_t)im.first + im.count > n_refs || im.count == 0u) {
        if (lane == 0) { fail(st); isplit[item] = 0u; }
        return;
    }
    SahBox b, cb;
    Best best{ __builtin_inf(), kSahNoKey, 0u };
    bool early;
    if (im.count <= kSahSmall) {
        // a reference per lane
        const bool act = (uint32_t)lane < im.count;
        const SahBox tb = act ? load_box(tribox, refs[im.first + lane]) : sah_empty();
        const SahBox tc = act ? centroid_box(tb) : sah_empty();
        b = wave_union(tb);
        cb = wave_union(tc);
        early = sah_early_leaf(im.count, level, root);
        if (!early) {
            int k[3];
            bool ax[3];
            for (int a = 0; a < 3; ++a) {
                const float ext = cb.hi[a] - cb.lo[a];
                ax[a] = ext > 0.f;
                k[a] = ax[a] && act ? sah_bin(tc.lo[a], cb.lo[a], ext) : 0;
            }
            // the split after this lane's own bin, on each axis
            SahBox L[3] = { sah_empty(), sah_empty(), sah_empty() }, R[3] = { sah_empty(), sah_empty(), sah_empty() };
            uint32_t nl[3] = { 0u, 0u, 0u }, nr[3] = { 0u, 0u, 0u };
            for (uint32_t j = 0; j < im.count; ++j) {
                const SahBox bj = shfl_box(tb, (int)j);
                for (int a = 0; a < 3; ++a) {
                    const int kj = __shfl(k[a], (int)j);
                    if (kj <= k[a]) { sah_grow(L[a], bj); ++nl[a]; }
                    else { sah_grow(R[a], bj); ++nr[a]; }
                }
            }
            for (int a = 0; a < 3; ++a)
                if (act && ax[a]) consider(best, L[a], nl[a], R[a], nr[a], a, k[a]);
        }
    } else {
        b = dec_box(state[item].b);
        cb = dec_box(state[item].cb);
        early = sah_early_leaf(im.count, level, root);
        const uint32_t slot = im.first / (kSahSmall + 1u);
        if (slot >= n_slots) {
            if (lane == 0) { fail(st); isplit[item] = 0u; }
            return;
        }
        if (!early) {
            for (int a = 0; a < 3; ++a) {
                const float ext = cb.hi[a] - cb.lo[a];
                if (!(ext > 0.f)) continue;       // never binned: its bins are empty
                // bins `lane` and `lane + 64` of this axis; the bins are left empty
                SahBox e0, e1;
                for (int c = 0; c < 3; ++c) {
                    e0.lo[c] = dec(bins[bin_at(slot, a, c, lane)]);
                    e0.hi[c] = dec(bins[bin_at(slot, a, 3 + c, lane)]);
                    e1.lo[c] = dec(bins[bin_at(slot, a, c, lane + 64)]);
                    e1.hi[c] = dec(bins[bin_at(slot, a, 3 + c, lane + 64)]);
                }
                const uint32_t c0 = (uint32_t)bins[bin_at(slot, a, 6, lane)];
                const uint32_t c1 = (uint32_t)bins[bin_at(slot, a, 6, lane + 64)];
                for (int c = 0; c < 3; ++c) {
                    bins[bin_at(slot, a, c, lane)] = bins[bin_at(slot, a, c, lane + 64)] = enc(__builtin_inff());
                    bins[bin_at(slot, a, 3 + c, lane)] = bins[bin_at(slot, a, 3 + c, lane + 64)] = enc(-__builtin_inff());
                }
                bins[bin_at(slot, a, 6, lane)] = bins[bin_at(slot, a, 6, lane + 64)] = 0;
                // candidates: the split after bin `lane` and after bin `lane + 64`
                SahBox L0 = sah_empty(), R0 = sah_empty(), L1 = sah_empty(), R1 = sah_empty();
                uint32_t nl0 = 0u, nr0 = 0u, nl1 = 0u, nr1 = 0u;
                for (int j = 0; j < 64; ++j) {
                    const SahBox b0 = shfl_box(e0, j), b1 = shfl_box(e1, j);        // bins j and j + 64
                    const uint32_t n0 = __shfl(c0, j), n1 = __shfl(c1, j);
                    if (j <= lane) { sah_grow(L0, b0); nl0 += n0; } else { sah_grow(R0, b0); nr0 += n0; }
                    sah_grow(R0, b1); nr0 += n1;
                    sah_grow(L1, b0); nl1 += n0;
                    if (j <= lane) { sah_grow(L1, b1); nl1 += n1; } else { sah_grow(R1, b1); nr1 += n1; }
                }
                consider(best, L0, nl0, R0, nr0, a, lane);
                consider(best, L1, nl1, R1, nr1, a, lane + 64);
            }
        }
    }
    best = wave_best(best);
    if (lane != 0) return;
    const bool has_axis = best.key != kSahNoKey;
    const bool split = !early && (root || !sah_want_leaf(im.count, max_leaf, has_axis, best.cost, sah_area(b)));
    ItemState s;
    for (int a = 0; a < 3; ++a) {
        s.b[a] = enc(b.lo[a]); s.b[3 + a] = enc(b.hi[a]);
        s.cb[a] = enc(cb.lo[a]); s.cb[3 + a] = enc(cb.hi[a]);
    }
    s.split = split ? 1u : 0u;
    s.axis = has_axis ? best.key / kSahBins : kNoAxis;
    s.k = has_axis ? best.key % kSahBins : 0u;
    s.nl = has_axis ? best.nl : sah_median(im.count);
    if (split && (s.nl == 0u || s.nl >= im.count)) { fail(st); s.split = 0u; }
    state[item] = s;
    isplit[item] = s.split;
}

// ---- 4. which references go left -------------------------------------------------
__global__ __launch_bounds__(kBlock) void sah_flag_kernel(uint32_t n_refs, uint32_t n_items,
                                                          const uint32_t* __restrict__ refs,
                                                          const uint32_t* __restrict__ node_of,
                                                          const Item* __restrict__ items,
                                                          const ItemState* __restrict__ state,
                                                          const float4* __restrict__ tribox,
                                                          uint32_t* __restrict__ flags, const DevBuildStatus* st)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_refs || st->flags != 0u) return;
    const uint32_t item = node_of[i];
    uint32_t left = 0u;
    if (item != kInactive && item < n_items && state[item].split) {
        const uint32_t a = state[item].axis;
        if (a < 3u) {
            const float lo = dec(state[item].cb[a]), hi = dec(state[item].cb[3 + a]);
            const SahBox t = load_box(tribox, refs[i]);
            left = sah_bin(sah_centroid(t.lo[a], t.hi[a]), lo, hi - lo) <= (int)state[item].k ? 1u : 0u;
        } else {
            left = i - items[item].first < state[item].nl ? 1u : 0u;
        }
    }
    flags[i] = left;
}

// ---- 6. leaves and the next level's items ----------------------------------------
__global__ __launch_bounds__(kBlock) void sah_children_kernel(uint32_t n_items, uint32_t level, uint32_t node_base,
                                                              uint32_t max_nodes, uint32_t n_refs,
                                                              const Item* __restrict__ items,
                                                              const ItemState* __restrict__ state,
                                                              const uint32_t* __restrict__ isplit,
                                                              const uint32_t* __restrict__ sidx,
                                                              Item* __restrict__ next, float4* __restrict__ nodebox,
                                                              float4* __restrict__ cbox, int32_t* __restrict__ child,
                                                              unsigned long long* __restrict__ tpath, Control* ctl,
                                                              DevBuildStatus* st)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_items || st->flags != 0u) return;
    const Item im = items[i];
    const ItemState s = state[i];
    const uint32_t which = i & 1u;
    if ((size_t)im.first + im.count > n_refs) { fail(st); return; }
    const SahBox b = dec_box(s.b);
    if (i == n_items - 1u) ctl->splits = sidx[i] + isplit[i];
    if (level > 0u) {
        if (im.parent >= max_nodes) { fail(st); return; }
        store_box(cbox, 2 * (size_t)im.parent + which, b);
    }
    if (s.split) {
        const uint32_t id = node_base + sidx[i];
        if (id >= max_nodes || 2u * sidx[i] + 1u >= n_refs) { fail(st); return; }
        store_box(nodebox, id, b);
        if (level > 0u) child[2 * (size_t)im.parent + which] = (int32_t)id;
        next[2u * sidx[i]] = Item{ im.first, s.nl, id, 0u, sah_child_path(im.path, level, 0u) };
        next[2u * sidx[i] + 1u] = Item{ im.first + s.nl, im.count - s.nl, id, 0u, sah_child_path(im.path, level, 1u) };
    } else {
        if (level == 0u) { fail(st); return; }   // the root is always split
        if (!leaf_count_fits(im.count)) { atomicOr(&st->flags, DEVBVH_BIG_LEAF); return; }
        child[2 * (size_t)im.parent + which] = leaf_code(im.first, im.count);
        for (uint32_t k = 0; k < im.count; ++k) tpath[im.first + k] = im.path;
    }
}

// ---- 7. the next level's order ----------------------------------------------------
__global__ __launch_bounds__(kBlock) void sah_scatter_kernel(uint32_t n_refs, uint32_t n_items,
                                                             const uint32_t* __restrict__ refs,
                                                             const uint32_t* __restrict__ node_of,
                                                             const Item* __restrict__ items,
                                                             const ItemState* __restrict__ state,
                                                             const uint32_t* __restrict__ sidx,
                                                             const uint32_t* __restrict__ flags,
                                                             const uint32_t* __restrict__ rank,
                                                             uint32_t* __restrict__ refs_out,
                                                             uint32_t* __restrict__ node_out, DevBuildStatus* st)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_refs || st->flags != 0u) return;
    const uint32_t item = node_of[i], r = refs[i];
    if (item == kInactive || item >= n_items || !state[item].split) {
        refs_out[i] = r;
        node_out[i] = kInactive;
        return;
    }
    const Item im = items[item];
    const uint32_t left = flags[i], before = rank[i] - rank[im.first];          // lefts of this item before i
    const uint32_t dest = left ? im.first + before : im.first + state[item].nl + (i - im.first - before);
    if (dest >= n_refs || dest < im.first || dest >= im.first + im.count) { fail(st); return; }
    refs_out[dest] = r;
    node_out[dest] = 2u * sidx[item] + (left ? 0u : 1u);
}

// ---- emission: this tree's children (vr_devmesh_dev.hpp emit_nodes_kernel) ---------
struct SahChildren {
    const int32_t* child;                         // per node, two: a node number or a leaf code
    const float4* cbox;                           // per node, its two child boxes
    __device__ bool operator()(uint32_t id, uint32_t n_nodes, DevBox b[2], int32_t c[2], DevBuildStatus* st) const
    {
        if (id >= n_nodes) { fail(st); return false; }
        for (int k = 0; k < 2; ++k) {
            c[k] = child[2 * (size_t)id + k];
            if (c[k] >= 0 && (uint32_t)c[k] >= n_nodes) { fail(st); return false; }
            b[k] = load_box(cbox, 2 * (size_t)id + k);
        }
        return true;
    }
};

struct Scratch {
    float4 *tribox, *nodebox, *cbox;
    uint32_t *refs[2], *node_of[2], *flags, *rank, *isplit, *sidx;
    Item* items[2];
    ItemState* state;
    int32_t *bins, *child;
    EmitScratch emit;
    Control* ctl;
    char* temp;
    size_t n_slots;
};

void carve(Arena& ar, Scratch& s, uint32_t n, size_t temp_bytes)
{
    const size_t N = n - 1u;                      // nodes at most
    s.n_slots = n / (kSahSmall + 1u) + 1u;        // large items have distinct first / (kSahSmall + 1)
    s.tribox = ar.take<float4>(2 * (size_t)n);
    for (int i = 0; i < 2; ++i) {
        s.refs[i] = ar.take<uint32_t>(n);
        s.node_of[i] = ar.take<uint32_t>(n);
        s.items[i] = ar.take<Item>(n);
    }
    s.flags = ar.take<uint32_t>(n);
    s.rank = ar.take<uint32_t>(n);
    s.isplit = ar.take<uint32_t>(n);
    s.sidx = ar.take<uint32_t>(n);
    s.state = ar.take<ItemState>(n);
    s.bins = ar.take<int32_t>(s.n_slots * 3u * kBinFields * kSahBins);
    s.nodebox = ar.take<float4>(2 * N);
    s.cbox = ar.take<float4>(4 * N);
    s.child = ar.take<int32_t>(2 * N);
    s.emit.carve(ar, N);
    s.ctl = ar.take<Control>(1);
    s.temp = ar.take<char>(temp_bytes ? temp_bytes : 16);
}

hipError_t temp_sizes(uint32_t n, hipStream_t s, size_t& bytes)
{
    size_t scan = 0, sort = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, scan, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n,
                                           rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    e = emit_sort_temp_bytes(n - 1u, s, sort);
    bytes = scan > sort ? scan : sort;
    return e;
}

} // namespace

size_t devsah_arena_bytes(uint32_t n_tris)
{
    const uint32_t n = n_tris < 2u ? 2u : n_tris;
    size_t temp = 0;
    if (temp_sizes(n, nullptr, temp) != hipSuccess) return 0;
    Arena ar;
    Scratch sc;
    carve(ar, sc, n, temp);
    return ar.used;
}

int devsah_build(const float* positions, const float* normals, const float* tangents, const float* uvs,
                 uint32_t n_verts, const uint32_t* tris, uint32_t n_tris, uint32_t max_leaf, const MeshArrays& out,
                 DevBuildStatus* d_status, void** scratch_out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    *scratch_out = nullptr;
    const uint32_t n = n_tris < 2u ? 2u : n_tris;
    const uint32_t max_nodes = n - 1u;

    size_t temp_bytes = 0;
    hipError_t e = temp_sizes(n, s, temp_bytes);
    if (e != hipSuccess) return (int)e;
    Arena ar;
    Scratch sc;
    if ((e = carve_alloc(ar, [&](Arena& a) { carve(a, sc, n, temp_bytes); })) != hipSuccess) return (int)e;
    auto bail = [&](hipError_t err) { (void)hipStreamSynchronize(s); (void)hipFree(ar.base); return (int)err; };

    const uint32_t nb = blocks_for(n), nb_chunk = (uint32_t)((n + (size_t)kBlock * kChunk - 1) / ((size_t)kBlock * kChunk));
    sah_tris_kernel<<<nb, kBlock, 0, s>>>(positions, n_verts, tris, n_tris, n, sc.tribox, sc.refs[0], sc.node_of[0],
                                          d_status);
    sah_fill_bins_kernel<<<blocks_for(sc.n_slots * 3u * kBinFields * kSahBins), kBlock, 0, s>>>(sc.bins, sc.n_slots);
    sah_root_kernel<<<1, kBlock, 0, s>>>(sc.items[0], n);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e);

    uint32_t n_items = 1u, node_base = 0u, depth = 0u;
    int cur = 0;
    Control hctl{};
    DevBuildStatus hst{};
    for (uint32_t level = 0; n_items > 0u && level < kMaxBuildDepth; ++level) {
        const uint32_t* refs = sc.refs[cur];
        const uint32_t* node_of = sc.node_of[cur];
        const Item* items = sc.items[cur];
        sah_init_items_kernel<<<blocks_for(n_items), kBlock, 0, s>>>(n_items, sc.state, d_status);
        sah_bounds_kernel<<<nb_chunk, kBlock, 0, s>>>(n, n_items, refs, node_of, items, sc.tribox, sc.state, d_status);
        if (level + 1u < kMaxBuildDepth)          // below the depth cap every item is a leaf unbinned
            sah_bin_kernel<<<nb_chunk, kBlock, 0, s>>>(n, n_items, (uint32_t)sc.n_slots, refs, node_of, items,
                                                       sc.state, sc.tribox, sc.bins, d_status);
        sah_node_kernel<<<(n_items + kBlock / 64 - 1) / (kBlock / 64), kBlock, 0, s>>>(
            n_items, n, (uint32_t)sc.n_slots, level, max_leaf, refs, items, sc.tribox, sc.state, sc.bins, sc.isplit,
            d_status);
        sah_flag_kernel<<<nb, kBlock, 0, s>>>(n, n_items, refs, node_of, items, sc.state, sc.tribox, sc.flags,
                                              d_status);
        if ((e = hipGetLastError()) != hipSuccess) return bail(e);
        size_t tb = temp_bytes;
        e = rocprim::exclusive_scan(sc.temp, tb, sc.flags, sc.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), s);
        if (e != hipSuccess) return bail(e);
        tb = temp_bytes;
        e = rocprim::exclusive_scan(sc.temp, tb, sc.isplit, sc.sidx, 0u, (size_t)n_items, rocprim::plus<uint32_t>(), s);
        if (e != hipSuccess) return bail(e);
        sah_children_kernel<<<blocks_for(n_items), kBlock, 0, s>>>(n_items, level, node_base, max_nodes, n, items,
                                                                   sc.state, sc.isplit, sc.sidx, sc.items[cur ^ 1],
                                                                   sc.nodebox, sc.cbox, sc.child, out.tpath, sc.ctl,
                                                                   d_status);
        sah_scatter_kernel<<<nb, kBlock, 0, s>>>(n, n_items, refs, node_of, items, sc.state, sc.sidx, sc.flags,
                                                 sc.rank, sc.refs[cur ^ 1], sc.node_of[cur ^ 1], d_status);
        if ((e = hipGetLastError()) != hipSuccess) return bail(e);
        // the level's one read-back: the number of splits (and the error flags)
        if ((e = hipMemcpyAsync(&hctl, sc.ctl, sizeof(Control), hipMemcpyDeviceToHost, s)) != hipSuccess) return bail(e);
        if ((e = hipMemcpyAsync(&hst, d_status, sizeof(hst), hipMemcpyDeviceToHost, s)) != hipSuccess) return bail(e);
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail(e);
        if (hst.flags != 0u) { *scratch_out = ar.base; return 0; }     // the caller reads the flags
        const uint32_t splits = hctl.splits;
        if (splits > 0u) depth = level + 1u;
        if ((size_t)node_base + splits > max_nodes || 2u * (size_t)splits > n) return bail(hipErrorUnknown);
        node_base += splits;
        n_items = 2u * splits;
        cur ^= 1;
    }
    const uint32_t N = node_base;
    if (N == 0u || n_items != 0u) return bail(hipErrorUnknown);

    const EmitArgs ea{ N, 0u, N + 1u, depth, true, sc.nodebox, sc.refs[cur], n, n_tris,
                       { positions, normals, tangents, uvs }, tris, sc.emit, sc.temp, temp_bytes, out, d_status };
    if ((e = emit_mesh(ea, SahChildren{ sc.child, sc.cbox }, s)) != hipSuccess) return bail(e);
    *scratch_out = ar.base;
    return 0;
}

} // namespace vr
