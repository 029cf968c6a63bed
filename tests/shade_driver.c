/* TEST INFRASTRUCTURE ONLY -- the yardstick of vrhip_shade_surface.
 *
 * The oracle's trace (oracle/vro.c, static) restated with one change: at
 * bounce 0 the hit and the hit flag are the caller's instead of
 * intersect_scene's.  This file includes vro.c, so every function the
 * restatement calls from bounce 1 on (intersect_scene, lookup_brdf, the
 * generator, the libm switch) is the one the reference-rendered fixtures pin
 * through the renders, and tests/test_shade_cpu.py pins the restatement itself
 * to that trace: fed intersect_scene's own records it must return trace's
 * radiance bit for bit.  Compiled by tests/shade_cases.py into a shared object
 * of its own with oracle/Makefile's CFLAGS, plus vro_math.c; nothing in the
 * product links it.
 *
 * The one other difference: there is no camera origin, so the depth term of
 * :656-661 is not computed and a path's w is 0.
 */
#include "vro.c"

/* trace (vro.c) from `ray`, whose bounce-0 result is (hit0, *h0) */
static vf4 trace_given(tctx *tc, const ray_t *first, const hit_t *h0, int hit0, uint32_t *s0, uint32_t *s1)
{
    const vro_scene *sc = tc->sc;
    const mctx *m = &tc->m;
    ray_t ray = *first;
    vf4 accum = f4(0.f, 0.f, 0.f, 0.f);
    vf4 mask = f4(1.f, 1.f, 1.f, 0.f);
    uint32_t seed = vro_hash(s0, s1);
    rng_t rng; rng_seed(&rng, seed);

    for (unsigned bounces = 0; bounces < 4; bounces++) {
        hit_t h;
        int hit;
        if (bounces == 0) {
            h = *h0;                                                /* the one change */
            hit = hit0;
        } else {
            memset(&h, 0, sizeof(h));
            hit = intersect_scene(tc, &ray, &h);
        }
        if (!hit) {
            if (!sc->use_cornell) {                                 /* :631-648 */
                float lx = m_atan2f(m, ray.d.x, ray.d.z);
                float ly = m_acosf(m, ray.d.y);
                lx = lx < 0 ? (float)((double)lx + 2.0 * (double)VR_PI) : lx;
                lx = (float)((double)lx / (2.0 * (double)VR_PI));
                ly = ly / VR_PI;
                int x = f2i(lx * (float)sc->hdr_w);
                int y = f2i(ly * (float)sc->hdr_h);
                int val = (int)((uint32_t)x + (uint32_t)y * sc->hdr_w);
                int addr = (int)clampi(val, 0, (int)(sc->hdr_w * sc->hdr_h - 1u));
                addeq4(&accum, mul4(mul4s(mask, 2.f), ld4(sc->hdr, addr)));
                accum.w = 0.f;
                return accum;
            }
            return f4(0.f, 0.f, 0.f, 0.f);                          /* :649-652 */
        }
        addeq4(&accum, mul4(mask, h.emission));                     /* :664 */
        ray.o = h.hitPoint;
        vf4 normal = h.normal;

        if (h.hitType == 0) {                                       /* :671-676 */
            ray.d = sub4(ray.d, mul4s(mul4s(normal, 2.f), dot4(normal, ray.d)));
            addeq4(&ray.o, mul4s(normal, 0.05f));
        } else if (h.hitType == 1) {                                /* :678-722 */
            float aoi = dot4(h.normal, muls4(-1.f, ray.d));
            float fe = lerpf_(m_powf(m, 1.f - aoi, sc->fresnel_pow), 1.f, sc->fresnel_coef) * h.spec.x;
            int reflect = (rng_uniform(&rng) < fe);
            vf4 newdir;
            vf4 w = normal;
            vf4 axis = fabsf(w.x) > 0.1f ? f4(0.f, 1.f, 0.f, 0.f) : f4(1.f, 0.f, 0.f, 0.f);
            if (reflect) {
                muleq4(&mask, h.spec);
                newdir = normalize4(sub4(ray.d, mul4s(mul4s(normal, 2.f), dot4(normal, ray.d))));
            } else {
                float rand1 = 2.f * VR_PI * rng_uniform(&rng);
                float rand2 = rng_uniform(&rng);
                float rand2s = sqrtf(rand2);
                vf4 u = normalize4(cross4(axis, w));
                vf4 v = cross4(w, u);
                float sn, cs;
                m_sincos(m, rand1, &sn, &cs);
                newdir = normalize4(add4(add4(mul4s(mul4s(u, cs), rand2s), mul4s(mul4s(v, sn), rand2s)),
                                         mul4s(w, sqrtf(1 - rand2))));
                muleq4(&mask, h.color);
                muleq4s(&mask, dot4(newdir, normal));
                muleq4s(&mask, 2.f);
            }
            addeq4(&ray.o, mul4s(normal, 0.05f));
            ray.d = newdir;
        } else if (h.hitType == 2) {                                /* :724-764 */
            vf4 w = normal;
            vf4 axis = fabsf(w.x) > 0.1f ? f4(0.f, 1.f, 0.f, 0.f) : f4(1.f, 0.f, 0.f, 0.f);
            float rand1 = 2.f * VR_PI * rng_uniform(&rng);
            float rand2 = rng_uniform(&rng);
            float rand2s = sqrtf(rand2);
            vf4 u = normalize4(cross4(axis, w));
            vf4 v = cross4(w, u);
            float sn, cs;
            m_sincos(m, rand1, &sn, &cs);
            vf4 newdir = normalize4(add4(add4(mul4s(mul4s(u, cs), rand2s), mul4s(mul4s(v, sn), rand2s)),
                                         mul4s(w, sqrtf(1 - rand2))));
            if (sc->brdf) {
                float dw = 24 * m_powf(m, newdir.x * newdir.x + newdir.y * newdir.y + newdir.z * newdir.z, -1.5f);
                muleq4(&mask, muls4(dw, max4(lookup_brdf(tc, newdir, ray.d, h.normal, h.tangent), f4(0, 0, 0, 0))));
            } else {
                muleq4(&mask, h.color);
                muleq4s(&mask, dot4(newdir, normal));
                muleq4s(&mask, 2.f);
            }
            addeq4(&ray.o, mul4s(normal, 0.05f));
            ray.d = newdir;
        }
    }
    accum.w = 0.f;
    return accum;
}

/* records: uint32[28 n], the words of vrhip_surface_hit; read are kind (0 a
 * miss, anything else a hit), type and the xyz of position, normal, tangent,
 * color, specular and emission (their w taken as 0).  dirs: float[3 n],
 * normalised by normalize4.  seeds: uint32[2 n].  out: float[4 k_max n], path
 * k of record i at out[4 (k_max i + k)], the k + 1'th on the record's seed
 * stream.  Returns tctx.err. */
int shade_driver(const vro_scene *sc, const uint32_t *records, const float *dirs, const uint32_t *seeds, uint32_t n,
                 uint32_t k_max, float *out)
{
    tctx tc;
    memset(&tc, 0, sizeof(tc));
    tc.sc = sc;
    tc.m.libm = sc->libm;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t *w = records + 28 * (size_t)i;
        hit_t h;
        memset(&h, 0, sizeof(h));
        h.hitPoint = f4(bitsf(w[4]), bitsf(w[5]), bitsf(w[6]), 0.f);
        h.normal = f4(bitsf(w[8]), bitsf(w[9]), bitsf(w[10]), 0.f);
        h.tangent = f4(bitsf(w[12]), bitsf(w[13]), bitsf(w[14]), 0.f);
        h.color = f4(bitsf(w[16]), bitsf(w[17]), bitsf(w[18]), 0.f);
        h.spec = f4(bitsf(w[20]), bitsf(w[21]), bitsf(w[22]), 0.f);
        h.emission = f4(bitsf(w[24]), bitsf(w[25]), bitsf(w[26]), 0.f);
        h.hitType = w[3];
        ray_t r;
        r.o = f4(0.f, 0.f, 0.f, 0.f);
        r.d = normalize4(f4(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2], 0.f));
        uint32_t s0 = seeds[2 * (size_t)i], s1 = seeds[2 * (size_t)i + 1];
        for (uint32_t k = 0; k < k_max; ++k) {
            vf4 res = trace_given(&tc, &r, &h, w[1] != 0u, &s0, &s1);
            memcpy(out + 4 * ((size_t)k_max * i + k), &res, 16);
        }
    }
    return tc.err;
}
