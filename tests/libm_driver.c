/* libm_driver.c -- the yardstick of tests/test_libm_cpu.py and
 * tests/test_gpu_libm.py: batch loops over the oracle's own functions (the
 * portable libm of oracle/vro_math.c; f2i, d2i, f2u8, lookup_brdf and trace of
 * oracle/vro.c, included below), so that a set of 2^22 elements costs one call.
 * Built with the oracle's CFLAGS (-ffp-contract=off).
 *
 * -DMUTANT=k wraps those functions in what a GPU or a toolchain gets wrong
 * (tests/test_libm_cpu.py shows that the input sets notice each):
 *   1  denormal operands read as signed zero
 *   2  denormal results returned as signed zero
 *   3  atan2 reads -0 in x as +0
 *   4  pow returns FLT_MAX where the result overflows
 *   5  acos of |x| > 1 returns 0 or pi instead of NaN
 *   6  the last bit of the result flipped when the first operand's bit
 *      pattern is a multiple of 4099
 *   7  theta_half_index rounds s * 90 to the nearest integer before it truncates
 *   8  phi_diff_index without its + pi wrap for negative angles
 */
#include "vro.c"
#include <float.h>

#ifndef MUTANT
#define MUTANT 0
#endif

/* the function codes of vrhip_selftest_math (include/vrhip.h) */
enum { FN_SIN = 0, FN_COS = 1, FN_ACOS = 2, FN_ATAN2 = 3, FN_POW = 4, FN_F2I = 7, FN_D2I = 8, FN_F2U8 = 9 };

static float flushed(float x)
{
    const uint32_t u = fbits(x);
    return (u & 0x7f800000u) == 0u ? bitsf(u & 0x80000000u) : x;
}

static float libm_one(int fn, float a, float b)
{
    float r = 0.f, s, c;
#if MUTANT == 1
    a = flushed(a); b = flushed(b);
#endif
    switch (fn) {
    case FN_SIN: vro_p_sincosf(a, &s, &c); r = s; break;
    case FN_COS: vro_p_sincosf(a, &s, &c); r = c; break;
    case FN_ACOS:
        r = vro_p_acosf(a);
#if MUTANT == 5
        if (a > 1.f) r = 0.f;
        if (a < -1.f) r = 3.14159274f;
#endif
        break;
    case FN_ATAN2:
#if MUTANT == 3
        if (fbits(b) == 0x80000000u) b = 0.f;
#endif
        r = vro_p_atan2f(a, b);
        break;
    case FN_POW:
        r = vro_p_powf(a, b);
#if MUTANT == 4
        if (fabsf(r) == INFINITY && a != 0.f && fabsf(a) != INFINITY && fabsf(b) != INFINITY)
            r = r > 0.f ? FLT_MAX : -FLT_MAX;
#endif
        break;
    default: return 0.f;
    }
#if MUTANT == 2
    r = flushed(r);
#endif
#if MUTANT == 6
    if (fbits(a) % 4099u == 0u) r = bitsf(fbits(r) ^ 1u);
#endif
    return r;
}

/* out[i] = fn(a[i], b[i]) as vrhip_selftest_math defines it (7 and 8: the int's bits; 9: the byte as a float) */
int libm_batch(int fn, const float *a, const float *b, float *out, size_t n)
{
    switch (fn) {
    case FN_SIN: case FN_COS: case FN_ACOS: case FN_ATAN2: case FN_POW:
#pragma omp parallel for schedule(static)
        for (size_t i = 0; i < n; ++i) out[i] = libm_one(fn, a[i], b[i]);
        return 0;
    case FN_F2I:
        for (size_t i = 0; i < n; ++i) out[i] = ibitsf(f2i(a[i]));
        return 0;
    case FN_D2I:
        for (size_t i = 0; i < n; ++i) out[i] = ibitsf(d2i((double)a[i] * (double)b[i]));
        return 0;
    case FN_F2U8:
        for (size_t i = 0; i < n; ++i) out[i] = (float)f2u8(a[i]);
        return 0;
    }
    return -1;
}

/* brdf_index of vro.c with the arm it took (0: theta_diff < 1e-3, 1: the
 * general one, 2: theta_H <= 1e-3) and, in mutant builds, a wrong index map */
static int theta_half_index_m(float theta_half)
{
#if MUTANT == 7
    if (theta_half <= 0.0) return 0;
    float s = sqrtf((float)((double)theta_half * (2.0 / (double)VR_PI)));
    return (int)clampi(f2i(rintf(s * 90)), 0, 90 - 1);
#else
    return theta_half_index(theta_half);
#endif
}
static int phi_diff_index_m(float phi_diff)
{
#if MUTANT == 8
    return (int)clampi(d2i((double)phi_diff * (1.0 / (double)VR_PI * (360 / 2))), 0, 360 / 2 - 1);
#else
    return phi_diff_index(phi_diff);
#endif
}
static int brdf_index_arm(const mctx *m, vf4 refl, vf4 cur, vf4 normal, vf4 tangent, int *arm)
{
    vf4 bitangent = cross4(normal, tangent);
    vf4 H = normalize4(sub4(refl, cur));
    float theta_H = m_acosf(m, clampf(dot4(normal, H), 0.f, 1.f));
    float theta_diff = m_acosf(m, clampf(dot4(H, refl), 0.f, 1.f));
    float phi_diff = 0.f;
    if ((double)theta_diff < 1e-3) {
        *arm = 0;
        phi_diff = m_atan2f(m, clampf(-dot4(refl, bitangent), -1.f, 1.f), clampf(dot4(refl, tangent), -1.f, 1.f));
    } else if ((double)theta_H > 1e-3) {
        *arm = 1;
        vf4 u = muls4(-1.f, normalize4(sub4(normal, muls4(dot4(normal, H), H))));
        vf4 v = cross4(H, u);
        phi_diff = m_atan2f(m, clampf(dot4(refl, v), -1.f, 1.f), clampf(dot4(refl, u), -1.f, 1.f));
    } else {
        *arm = 2;
        theta_H = 0.f;
    }
    return phi_diff_index_m(phi_diff) + theta_diff_index(theta_diff) * 360 / 2
           + theta_half_index_m(theta_H) * 360 / 2 * 90;
}

/* The oracle's lookup_brdf on n frames (refl, cur, normal, tangent: 16 floats
 * each) against a planar table: out 4 n floats, index and arm n each.  Returns
 * the number of frames on which the restated index above differs from the
 * oracle's brdf_index (0 in the plain build: the mutants live in the
 * restatement, whose index then also picks the table entry). */
long libm_brdf(const float *table, const float *frames, size_t n, float *out, int32_t *index, uint8_t *arm)
{
    vro_scene sc;
    memset(&sc, 0, sizeof(sc));
    sc.brdf = table;
    sc.libm = VRO_LIBM_PORTABLE;
    tctx tc = { &sc, { VRO_LIBM_PORTABLE }, NULL, 0 };
    long differ = 0;
    for (size_t i = 0; i < n; ++i) {
        vf4 f[4];
        memcpy(f, frames + 16 * i, 64);
        int a = 0;
        const int ind = brdf_index_arm(&tc.m, f[0], f[1], f[2], f[3], &a);
        differ += ind != brdf_index(&tc.m, f[0], f[1], f[2], f[3]);
        vf4 r;
#if MUTANT == 7 || MUTANT == 8
        r = f4((float)((double)table[ind] * (1.0 / 1500.0)), (float)((double)table[ind + 1458000] * (1.15 / 1500.0)),
               (float)((double)table[ind + 2916000] * (1.66 / 1500.0)), 0.f);
#else
        r = lookup_brdf(&tc, f[0], f[1], f[2], f[3]);
#endif
        memcpy(out + 4 * i, &r, 16);
        if (index) index[i] = ind;
        if (arm) arm[i] = (uint8_t)a;
    }
    return differ;
}

/* The oracle's trace of one path per ray, as vrhip_trace_radiance(samples = 1)
 * defines its record: the ray (o, normalize(d)), the path seeded by the ray's
 * seed pair, rgb = 0 + result * 1 and w the path's.  escaped[i] = 1 when the
 * ray meets nothing at bounce 0.  The caller keeps every float finite and the
 * squared length of d inside (0, FLT_MAX]. */
int libm_trace_rays(const vro_scene *sc, const float *o, const float *d, const uint32_t *seeds, size_t n, float *out,
                    uint8_t *escaped)
{
    if (!sc->use_cornell && !sc->hdr) return -2;
    int err = 0;
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; ++i) {
        tctx tc = { sc, { sc->libm }, NULL, 0 };
        ray_t r;
        r.o = f4(o[3 * i], o[3 * i + 1], o[3 * i + 2], 0.f);
        r.d = normalize4(f4(d[3 * i], d[3 * i + 1], d[3 * i + 2], 0.f));
        if (escaped) {
            hit_t h;
            memset(&h, 0, sizeof(h));
            escaped[i] = (uint8_t)!intersect_scene(&tc, &r, &h);
        }
        uint32_t s0 = seeds[2 * i], s1 = seeds[2 * i + 1];
        const vf4 res = trace(&tc, &r, &s0, &s1);
        const vf4 io = add4(f4(0.f, 0.f, 0.f, 0.f), mul4s(res, 1.f / 1.f));
        out[4 * i] = io.x; out[4 * i + 1] = io.y; out[4 * i + 2] = io.z; out[4 * i + 3] = res.w;
        if (tc.err) {
#pragma omp critical
            err = tc.err;
        }
    }
    return err;
}
