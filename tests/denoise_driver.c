/* denoise_driver.c -- the yardstick of vrhip_denoise: the filter's pixelwise
 * definition (include/vrhip.h) restated in plain C, one cell at a time, with
 * no tiling, no scratch planes and no reciprocal shortcut.  Written from the
 * definition, not from the kernels.  Built with the oracle's CFLAGS
 * (-ffp-contract=off): every operation below is one fp32 rounding.
 *
 * -DMUTANT=k builds a deliberately wrong filter (tests/test_denoise_cpu.py
 * shows which parity case notices which):
 *   1  stride s + 1           2  taps clamped to the edge instead of skipped
 *   3  kc not scaled per pass 4  taps summed in reverse order
 *   5  demodulation threshold ignored (every channel of a valid cell divided)
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef MUTANT
#define MUTANT 0
#endif

enum { WORDS = 28, KIND = 1, POSITION = 4, NORMAL = 8, ALBEDO = 16 };

static float word(const uint32_t* rec, int k) { float f; memcpy(&f, rec + k, 4); return f; }

static int valid(const uint32_t* guides, size_t i) { const uint32_t k = guides[WORDS * i + KIND]; return k >= 1u && k <= 4u; }

static int demodulated(float a)
{
#if MUTANT == 5
    (void)a; return 1;
#else
    return a > 0x1p-8f;
#endif
}

/* stats (or NULL): [0] taps evaluated, [1..3] taps whose wn, wp, wc lies strictly inside (0.01, 0.99) */
int denoise_driver(const float* color, const uint32_t* guides, uint32_t W, uint32_t H, uint32_t n_passes, uint32_t flags,
                   uint32_t m, float sigma_color, float sigma_position, float* out, double* stats)
{
    static const float K[3] = { 0.375f, 0.25f, 0.0625f };
    const size_t n = (size_t)W * H;
    if (n_passes == 0) { memmove(out, color, n * 16); return 0; }
    float* C = malloc(n * 16), * D = malloc(n * 16);
    if (!C || !D) { free(C); free(D); return 1; }
    memcpy(C, color, n * 16);
    const int demod = (flags & 1u) != 0;
    if (demod)
        for (size_t i = 0; i < n; ++i)
            if (valid(guides, i))
                for (int ch = 0; ch < 3; ++ch) {
                    const float a = word(guides + WORDS * i, ALBEDO + ch);
                    if (demodulated(a)) C[4 * i + ch] = color[4 * i + ch] * (1.f / a);
                }
    const float kp = 1.f / (sigma_position * sigma_position);
    const float kc0 = 1.f / (sigma_color * sigma_color);
    for (uint32_t j = 0; j < n_passes; ++j) {
#if MUTANT == 1
        const long long s = (1ll << j) + 1;
#else
        const long long s = 1ll << j;
#endif
#if MUTANT == 3
        const float kc = kc0;
#else
        const float kc = kc0 * (float)(1u << (2u * j));
#endif
        for (long long y = 0; y < (long long)H; ++y)
            for (long long x = 0; x < (long long)W; ++x) {
                const size_t p = (size_t)y * W + (size_t)x;
                float* o = D + 4 * p;
                const float* Cp = C + 4 * p;
                o[0] = Cp[0]; o[1] = Cp[1]; o[2] = Cp[2]; o[3] = Cp[3];
                if (!valid(guides, p)) continue;
                const uint32_t* gp = guides + WORDS * p;
                const float npx = word(gp, NORMAL), npy = word(gp, NORMAL + 1), npz = word(gp, NORMAL + 2);
                const float ppx = word(gp, POSITION), ppy = word(gp, POSITION + 1), ppz = word(gp, POSITION + 2);
                float sum[3] = { 0.f, 0.f, 0.f }, ws = 0.f;
                for (int t = 0; t < 25; ++t) {
#if MUTANT == 4
                    const int dy = 2 - t / 5, dx = 2 - t % 5;
#else
                    const int dy = t / 5 - 2, dx = t % 5 - 2;
#endif
                    long long qx = x + dx * s, qy = y + dy * s;
#if MUTANT == 2
                    qx = qx < 0 ? 0 : qx >= (long long)W ? (long long)W - 1 : qx;
                    qy = qy < 0 ? 0 : qy >= (long long)H ? (long long)H - 1 : qy;
#else
                    if (qx < 0 || qx >= (long long)W || qy < 0 || qy >= (long long)H) continue;
#endif
                    const size_t q = (size_t)qy * W + (size_t)qx;
                    if (!valid(guides, q)) continue;
                    const uint32_t* gq = guides + WORDS * q;
                    const float* Cq = C + 4 * q;
                    const float h = K[abs(dy)] * K[abs(dx)];
                    const float dn = (npx * word(gq, NORMAL) + npy * word(gq, NORMAL + 1)) + npz * word(gq, NORMAL + 2);
                    float wn = dn > 0.f ? dn : 0.f;
                    for (uint32_t r = 0; r < m; ++r) wn = wn * wn;
                    const float ex = word(gq, POSITION) - ppx, ey = word(gq, POSITION + 1) - ppy, ez = word(gq, POSITION + 2) - ppz;
                    const float dp = (npx * ex + npy * ey) + npz * ez;
                    const float wp = 1.f / (1.f + (dp * dp) * kp);
                    const float cx = Cq[0] - Cp[0], cy = Cq[1] - Cp[1], cz = Cq[2] - Cp[2];
                    const float d2 = (cx * cx + cy * cy) + cz * cz;
                    const float wc = 1.f / (1.f + d2 * kc);
                    const float w = ((h * wn) * wp) * wc;
                    sum[0] = sum[0] + w * Cq[0];
                    sum[1] = sum[1] + w * Cq[1];
                    sum[2] = sum[2] + w * Cq[2];
                    ws = ws + w;
                    if (stats) {
                        stats[0] += 1.0;
                        stats[1] += wn > 0.01f && wn < 0.99f;
                        stats[2] += wp > 0.01f && wp < 0.99f;
                        stats[3] += wc > 0.01f && wc < 0.99f;
                    }
                }
                if (ws > 0.f) {
                    const float inv = 1.f / ws;
                    o[0] = sum[0] * inv; o[1] = sum[1] * inv; o[2] = sum[2] * inv;
                }
            }
        float* t = C; C = D; D = t;
    }
    for (size_t i = 0; i < n; ++i) {
        float* o = out + 4 * i;                /* out may be color: color is not read from here on */
        float c[4] = { C[4 * i], C[4 * i + 1], C[4 * i + 2], C[4 * i + 3] };
        if (demod && valid(guides, i))
            for (int ch = 0; ch < 3; ++ch) {
                const float a = word(guides + WORDS * i, ALBEDO + ch);
                if (demodulated(a)) c[ch] = c[ch] * a;
            }
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
    }
    free(C); free(D);
    return 0;
}
