// vr_shade_dev.hpp -- device half of vr_shade.hpp: the kernel that traces
// paths from the caller's surface records and its per-feature-set launchers,
// included by the translation units that instantiate it (vr_shade*.hip).
#pragma once
#include "vr_kernel.hpp"
#include "vr_shade.hpp"

namespace vr {

// bounce_step's material part (PathTracer.cu:664-764) for a hit that is given
// as a Hit rather than found as a HitRec: bounce_step calls fill_hit itself and
// cannot take one.  The same operations in the same order as its plain
// branches, so a record fill_hit wrote shades to the same bits: the emission
// term, the three material types, the Fresnel test, lookup_brdf, draw_root,
// sincos_p and normalize4 as there.  Not here: the depth term (no camera
// origin), the diffuse pre-sample of the service and one-frame kernels, the
// counters and the SHADE_ONLY exits.  The path is at bounce 0 and never ends here.
template <uint32_t FEAT>
__device__ __forceinline__ void shade_given_hit(const RenderParams& p, Ray& ray, const Hit& h, PathState& ps)
{
    ps.accum = add4(ps.accum, mul4(ps.mask, h.em));
    ray.o = h.hp;
    const vr4 normal = h.n;
    if (h.type == 0) {                                                   // :671-676
        ray.d = sub4(ray.d, mul4s(mul4s(normal, 2.f), dot4(normal, ray.d)));
        ray.o = add4(ray.o, mul4s(normal, 0.05f));
    } else if (h.type == 1) {                                            // :678-722
        const float aoi = dot4(h.n, muls4(-1.f, ray.d));
        // (bounce_step: powf only matters when spec.x != 0)
        float fe = 0.f;
        if (h.spec.x != 0.f)
            fe = ((1.f - p.fresnel_coef) * pow_p(1.f - aoi, p.fresnel_pow) + p.fresnel_coef * 1.f) * h.spec.x;
        const bool reflect = (ps.rng.uniform() < fe);
        vr4 newdir;
        const vr4 w = normal;
        const vr4 axis = __builtin_fabsf(w.x) > 0.1f ? mk4(0.f, 1.f, 0.f, 0.f) : mk4(1.f, 0.f, 0.f, 0.f);
        if (reflect) {
            muleq4(ps.mask, h.spec);
            newdir = normalize4(sub4(ray.d, mul4s(mul4s(normal, 2.f), dot4(normal, ray.d))));
        } else {
            const float rand1 = 2.f * VR_PI * ps.rng.uniform();
            const float rand2 = ps.rng.uniform();
            const float rand2s = draw_root<FEAT>(rand2);
            const vr4 u = normalize4(cross4(axis, w));
            const vr4 v = cross4(w, u);
            float sn, cs;
            sincos_p(rand1, &sn, &cs);
            newdir = normalize4(add4(add4(mul4s(mul4s(u, cs), rand2s), mul4s(mul4s(v, sn), rand2s)),
                                     mul4s(w, draw_root<FEAT>(1 - rand2))));
            muleq4(ps.mask, h.col);
            muleq4s(ps.mask, dot4(newdir, normal));
            muleq4s(ps.mask, 2.f);
        }
        ray.o = add4(ray.o, mul4s(normal, 0.05f));
        ray.d = newdir;
    } else if (h.type == 2) {                                            // :724-764
        const vr4 w = normal;
        const vr4 axis = __builtin_fabsf(w.x) > 0.1f ? mk4(0.f, 1.f, 0.f, 0.f) : mk4(1.f, 0.f, 0.f, 0.f);
        const float rand1 = 2.f * VR_PI * ps.rng.uniform();
        const float rand2 = ps.rng.uniform();
        const float rand2s = draw_root<FEAT>(rand2);
        const vr4 u = normalize4(cross4(axis, w));
        const vr4 v = cross4(w, u);
        float sn, cs;
        sincos_p(rand1, &sn, &cs);
        const vr4 newdir = normalize4(add4(add4(mul4s(mul4s(u, cs), rand2s), mul4s(mul4s(v, sn), rand2s)),
                                           mul4s(w, draw_root<FEAT>(1 - rand2))));
        if HAS(F_BRDF) {
            const float dw = 24 * pow_p(newdir.x * newdir.x + newdir.y * newdir.y + newdir.z * newdir.z, -1.5f);
            const vr4 b = lookup_brdf(p.brdf, newdir, ray.d, h.n, h.tan);
            const vr4 bm = mk4(__builtin_fmaxf(b.x, 0.f), __builtin_fmaxf(b.y, 0.f), __builtin_fmaxf(b.z, 0.f),
                               __builtin_fmaxf(b.w, 0.f));
            muleq4(ps.mask, muls4(dw, bm));
        } else {
            muleq4(ps.mask, h.col);
            muleq4s(ps.mask, dot4(newdir, normal));
            muleq4s(ps.mask, 2.f);
        }
        ray.o = add4(ray.o, mul4s(normal, 0.05f));
        ray.d = newdir;
    }
    ++ps.bounce;
}

__device__ __forceinline__ vr4 shade_row(const vr_u32x4& r)
{
    return mk4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), 0.f);
}

enum : uint32_t { kLaneDone = 0u, kLaneStart = 1u, kLaneRay = 2u };

// One record per lane, in ray_radiance_kernel's shape: a block fills its node
// cache once, then each of its waves takes chunks of kShadeSlice = 64
// consecutive records in a grid-stride loop over at most one resident set of
// blocks.  A lane classifies its record before any scene work: an invalid one
// stores its four zero words and, like a lane past the last record, takes no
// part.  Then the wave loops, and one trip is:
//   1. the lanes at a path's start reload their record and direction, run
//      path_begin and bounce 0: shade_given_hit for a hit, bounce_step's own
//      miss branch for a miss;
//   2. the lanes holding a ray do one intersect and one bounce_step, exactly
//      as trace strings them together;
//   3. the lanes whose path ended add r * c to their sum, then start the next
//      sample or store their float4 and are done.
// The wave takes its next chunk when no lane is live.  A record's sum stays in
// its lane's registers and grows in path order; there is no scratch and no
// finish pass.  No atomics, no spinning on memory, no waiting for another
// wave: every trip advances every live lane by one bounce or retires it (a
// path has at most four bounces, a record n_samples paths), so the loop is
// bounded by construction.  Live across the traversal are the record index,
// the sample counter, the seed pair, the sum and the path's own state; the
// 112-byte record is reloaded at each path's start, not held.
// Not here: a lane taking another record as soon as its own is done (slices
// longer than a wave, ballot + mbcnt refill).  It was built and measured and
// lost to this form on the deciding workload (profiles/shade/).
template <int STACK, uint32_t FEAT>
__global__ void __launch_bounds__(kBlockThreads, render_waves<FEAT>(STACK))
surface_shade_kernel(const RenderParams p, const SurfaceShade q)
{
    constexpr bool MK = (FEAT & F_MESH) != 0u;           // a kernel that may traverse the mesh
    constexpr int CN = MK ? cache_nodes(STACK) : 1;
    __shared__ int lds_stack[MK ? STACK * kBlockThreads : 1];
    __shared__ vr4 lds_nodes[3 * CN];
    __shared__ int2 lds_idx[CN];
    const int tid = threadIdx.x;
    const Lds L = lds_setup<FEAT>(p, lds_stack, lds_nodes, lds_idx, CN, tid);
    constexpr uint64_t kWaves = kBlockThreads / 64;
    const uint64_t n_chunks = ((uint64_t)q.n_hits + kShadeSlice - 1u) / kShadeSlice;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    const uint64_t lane = (uint64_t)(tid & 63);
    const float big = 3.402823466e38f;
    const float coef = 1.f / (float)q.n_samples;
    Cnt cnt;
    for (uint64_t chunk = (uint64_t)blockIdx.x * kWaves + (uint64_t)(tid >> 6); chunk < n_chunks; chunk += n_waves) {
        const uint64_t i = chunk * kShadeSlice + lane;
        uint32_t state = kLaneDone, k = 0u, s1 = 0u, s2 = 0u;
        float sum_x = 0.f, sum_y = 0.f, sum_z = 0.f;
        PathState ps;
        Ray ray;
        path_begin(ps, s1, s2);                          // defined values; every path begins its own
        ray.o = ray.d = mk4(0.f, 0.f, 0.f, 0.f);
        if (i < (uint64_t)q.n_hits) {
            const float* d = q.dirs + 3u * i;
            const vr4 dv = mk4(d[0], d[1], d[2], 0.f);
            const vr_u32x4 w0 = *reinterpret_cast<const vr_u32x4*>(q.hits + i);
            const float dd = dot4(dv, dv);
            // the radiance query's rule for a direction; then what the record says it is
            const bool valid = fabsf(dv.x) <= big && fabsf(dv.y) <= big && fabsf(dv.z) <= big && dd > 0.f && dd <= big &&
                               w0.y <= (uint32_t)HK_MESH && (w0.y == (uint32_t)HK_NONE || w0.w <= 2u);
            if (valid) {
                s1 = q.seeds[2u * i];
                s2 = q.seeds[2u * i + 1u];
                state = kLaneStart;
            } else {
                q.radiance[i] = mk4(0.f, 0.f, 0.f, 0.f);
            }
        }
        while (__ballot(state != kLaneDone) != 0ull) {
            bool done = false;
            vr4 out = mk4(0.f, 0.f, 0.f, 0.f);
            // 1. bounce 0 from the record
            if (state == kLaneStart) {
                const vr_u32x4* rec = reinterpret_cast<const vr_u32x4*>(q.hits + i);
                const float* d = q.dirs + 3u * i;
                const vr_u32x4 w0 = rec[0];
                ray.d = normalize4(mk4(d[0], d[1], d[2], 0.f));
                path_begin(ps, s1, s2);                  // a path leaves its seeds one hash on, where the next one starts
                if (w0.y == (uint32_t)HK_NONE) {
                    HitRec miss;
                    miss.t = 1e20f; miss.kind = HK_NONE; miss.idx = 0; miss.bu = miss.bv = 0.f; miss.su = miss.sv = 0.f;
                    ray.o = mk4(0.f, 0.f, 0.f, 0.f);
                    done = bounce_step<false, FEAT, false>(p, ray, miss, ps, out, cnt);      // :631-652, always ends
                } else {
                    Hit h;
                    h.hp = shade_row(rec[1]);
                    h.n = shade_row(rec[2]);
                    h.tan = shade_row(rec[3]);
                    h.col = shade_row(rec[4]);
                    h.spec = shade_row(rec[5]);
                    h.em = shade_row(rec[6]);
                    h.type = w0.w;
                    shade_given_hit<FEAT>(p, ray, h, ps);
                }
                state = kLaneRay;
            }
            // 2. one bounce of the render's own
            if (state == kLaneRay && !done) {
                HitRec hr;
                if (intersect_spheres<false, FEAT>(p, ray, hr, cnt) && mesh_needed<false, FEAT>(p, hr, ps.bounce))
                    traverse_mesh<STACK, false, FEAT>(p, ray, hr, L, cnt, any_hit_enough<false, FEAT>(p, ps.bounce));
                done = bounce_step<false, FEAT, false>(p, ray, hr, ps, out, cnt);
            }
            // 3. retire
            if (done) {
                sum_x = sum_x + out.x * coef;
                sum_y = sum_y + out.y * coef;
                sum_z = sum_z + out.z * coef;
                ++k;
                if (k < q.n_samples) {
                    state = kLaneStart;
                } else {
                    q.radiance[i] = mk4(sum_x, sum_y, sum_z, 0.f);           // one 16-B store per record
                    state = kLaneDone;
                }
            }
        }
    }
}

// One resident set of blocks at the kernel's launch bounds (render_waves
// waves on each of the four SIMDs), or the blocks the records need if fewer.
template <int STACK, uint32_t FEAT>
void launch_shade_one(const RenderParams& p, const SurfaceShade& q, uint32_t cu_count, hipStream_t s)
{
    constexpr uint32_t per_cu = (uint32_t)(4 * render_waves<FEAT>(STACK) * 64 / kBlockThreads);
    constexpr uint64_t per_block = (uint64_t)kShadeSlice * (kBlockThreads / 64);
    const uint64_t need = ((uint64_t)q.n_hits + per_block - 1u) / per_block;
    const uint64_t resident = (uint64_t)(cu_count ? cu_count : 1u) * per_cu;
    const uint32_t blocks = (uint32_t)(need < resident ? need : resident);
    surface_shade_kernel<STACK, FEAT><<<blocks, kBlockThreads, 0, s>>>(p, q);
}

// A mesh feature set at every stack size mesh_stack_entries returns.
template <uint32_t FEAT>
void launch_shade_stack(const RenderParams& p, const SurfaceShade& q, int stack, uint32_t cu_count, hipStream_t s)
{
    static_assert((FEAT & F_MESH) != 0u, "sphere sets run at 16 entries and no mesh LDS");
    if (stack <= 16) launch_shade_one<16, FEAT>(p, q, cu_count, s);
    else if (stack <= 24) launch_shade_one<24, FEAT>(p, q, cu_count, s);
    else if (stack <= 32) launch_shade_one<32, FEAT>(p, q, cu_count, s);
    else launch_shade_one<64, FEAT>(p, q, cu_count, s);
}

// per feature class, one translation unit each
void launch_shade_cornell_mesh(const RenderParams& p, const SurfaceShade& q, int stack, uint32_t cu_count, hipStream_t s);
void launch_shade_hdri_mesh(const RenderParams& p, const SurfaceShade& q, int stack, uint32_t cu_count, hipStream_t s);
void launch_shade_sphere(const RenderParams& p, const SurfaceShade& q, uint32_t cu_count, hipStream_t s);

} // namespace vr
