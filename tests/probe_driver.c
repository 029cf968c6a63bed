/* probe_driver.c -- the yardstick of vrhip_probe_sh and vrhip_sh_irradiance:
 * the projection and the irradiance evaluation of include/vrhip.h restated in
 * plain C, one probe at a time, from per-ray radiance records.  Written from
 * the definition, not from the kernels.  The records may come from the oracle
 * or from vrhip_trace_radiance on the expanded rays: the driver adds nothing
 * to them but the basis, the weights and the order of the sum.  Built with the
 * oracle's CFLAGS (-ffp-contract=off): every operation below is one fp32
 * rounding.
 *
 * `mutant` selects a deliberately wrong build (tests/test_probe_cpu.py shows
 * that each changes the output of the case set):
 *   1  the 64 slots added one after the other instead of by the tree
 *   2  blocks of 32            3  Y6 contracted into an fma
 *   4  (Y * L) * w             5  seeds combined with + instead of ^
 *   6  an invalid ray contributes (w * Y) * 0
 *   7  the tail of the last block padded with the last term instead of +0
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { WORDS = 28, TERMS = 27, BLOCK = 64 };

/* the seed pairs of ray (i, k), [P][K][2] */
void probe_expand_seeds(const uint32_t* probe_seeds, const uint32_t* dir_seeds, uint32_t P, uint32_t K, uint32_t mutant,
                        uint32_t* out)
{
    for (uint32_t i = 0; i < P; ++i)
        for (uint32_t k = 0; k < K; ++k)
            for (int a = 0; a < 2; ++a) {
                const uint32_t x = probe_seeds[2 * i + a], y = dir_seeds[2 * k + a];
                out[2 * ((size_t)i * K + k) + a] = mutant == 5 ? x + y : x ^ y;
            }
}

static void basis(float x, float y, float z, uint32_t mutant, float* Y)
{
    Y[0] = 0.282094792f;
    Y[1] = 0.488602512f * y;
    Y[2] = 0.488602512f * z;
    Y[3] = 0.488602512f * x;
    Y[4] = 1.09254843f * (x * y);
    Y[5] = 1.09254843f * (y * z);
    Y[6] = 0.315391565f * (mutant == 3 ? fmaf(3.f, z * z, -1.f) : 3.f * (z * z) - 1.f);
    Y[7] = 1.09254843f * (x * z);
    Y[8] = 0.546274215f * (x * x - y * y);
}

/* the 27 terms of one ray; dir as given, normalised as the radiance query does (1 / sqrtf, then a product) */
static void terms(const float* rec, const float* dir, float w, int valid, uint32_t mutant, float* t)
{
    for (int j = 0; j < TERMS; ++j) t[j] = 0.f;
    if (!valid && mutant != 6) return;
    const float dd = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
    const float inv = 1.0f / sqrtf(dd);
    float Y[9];
    basis(dir[0] * inv, dir[1] * inv, dir[2] * inv, mutant, Y);
    for (int j = 0; j < 9; ++j)
        for (int c = 0; c < 3; ++c) {
            const float L = valid ? rec[c] : 0.f;
            t[3 * j + c] = mutant == 4 ? (Y[j] * L) * w : (w * Y[j]) * L;
        }
}

/* rec: [P][K][4] radiance records (rgb read); dirs: [K][3]; weights: [K] or NULL; valid: [P][K]; out: [P][28] words */
int probe_project(const float* rec, const float* dirs, const float* weights, const uint8_t* valid, uint32_t P, uint32_t K,
                  uint32_t mutant, uint32_t* out)
{
    const uint32_t B = mutant == 2 ? 32u : (uint32_t)BLOCK;
    if (K == 0u) return 1;
    const float w_default = 12.566370614f / (float)K;
    for (uint32_t i = 0; i < P; ++i) {
        float total[TERMS];
        uint32_t count = 0u;
        for (int j = 0; j < TERMS; ++j) total[j] = 0.f;
        for (uint32_t b0 = 0; b0 < K; b0 += B) {
            float v[BLOCK][TERMS];
            for (uint32_t l = 0; l < B; ++l) {
                uint32_t k = b0 + l;
                if (k >= K) {
                    if (mutant != 7) { for (int j = 0; j < TERMS; ++j) v[l][j] = 0.f; continue; }
                    k = K - 1u;
                } else {
                    count += valid[(size_t)i * K + k] ? 1u : 0u;
                }
                terms(rec + 4 * ((size_t)i * K + k), dirs + 3 * (size_t)k, weights ? weights[k] : w_default,
                      valid[(size_t)i * K + k] != 0, mutant, v[l]);
            }
            if (mutant == 1) {
                for (uint32_t l = 1; l < B; ++l)
                    for (int j = 0; j < TERMS; ++j) v[0][j] = v[0][j] + v[l][j];
            } else {
                for (uint32_t s = B / 2u; s > 0u; s >>= 1)
                    for (uint32_t l = 0; l < s; ++l)
                        for (int j = 0; j < TERMS; ++j) v[l][j] = v[l][j] + v[l + s][j];
            }
            for (int j = 0; j < TERMS; ++j) total[j] = total[j] + v[0][j];
        }
        memcpy(out + (size_t)WORDS * i, total, sizeof(total));
        out[(size_t)WORDS * i + TERMS] = count;
    }
    return 0;
}

/* sh: [m][28]; index: [n] or NULL (then record q); normals: [n][3] as given; out: [n][4] */
int probe_irradiance(const float* sh, uint32_t m, const uint32_t* index, const float* normals, uint32_t n, float* out)
{
    static const float A[9] = { 3.14159274f, 2.09439516f, 2.09439516f, 2.09439516f,
                                0.785398185f, 0.785398185f, 0.785398185f, 0.785398185f, 0.785398185f };
    for (uint32_t q = 0; q < n; ++q) {
        const uint32_t p = index ? index[q] : q;
        float* o = out + 4 * (size_t)q;
        o[0] = o[1] = o[2] = o[3] = 0.f;
        if (p >= m) continue;
        float Y[9];
        basis(normals[3 * (size_t)q], normals[3 * (size_t)q + 1], normals[3 * (size_t)q + 2], 0u, Y);
        const float* s = sh + (size_t)WORDS * p;
        for (int c = 0; c < 3; ++c) {
            float e = A[0] * (s[c] * Y[0]);
            for (int j = 1; j < 9; ++j) e = e + A[j] * (s[3 * j + c] * Y[j]);
            o[c] = e;
        }
    }
    return 0;
}
