// vrhip_selftest.cpp -- device self-tests and the vector-memory microbenchmark
// (vrhip_selftest_*, vrhip_microbench_vmem): no context, a device index only.
#include "vr_ctx.hpp"
#include "vr_devmesh.hpp"
#include "vr_merl.hpp"

int vrhip_microbench_vmem(int device, uint32_t width_bytes, uint32_t distinct, double* lane_loads_per_s)
{
    if (!lane_loads_per_s || distinct == 0 || distinct > 64 || (64 % distinct) != 0 ||
        (width_bytes != 4 && width_bytes != 8 && width_bytes != 12 && width_bytes != 16))
        return fail(VRHIP_ERR_INVALID, "width must be 4/8/12/16 bytes, distinct a divisor of 64");
    HIP_TRY(hipSetDevice(device));
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    const uint32_t n_lines = 1u << 14;                   // 1 MiB: L2-resident (4 MiB per XCD)
    const uint32_t blocks = (uint32_t)cus * 8u;          // 8 waves per SIMD
    const int iters = 256;
    uint32_t* tab = nullptr;
    HIP_TRY(hipMalloc((void**)&tab, (size_t)n_lines * 64 + 64));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto done = [&](int code) {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        (void)hipFree(tab);
        return code;
    };
    if (hipMemset(tab, 0, (size_t)n_lines * 64 + 64) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
        hipEventCreate(&e1) != hipSuccess)
        return done(fail(VRHIP_ERR_HIP, "microbench setup failed"));
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {                  // the first launch warms the caches
        if (hipEventRecord(e0, nullptr) != hipSuccess ||
            vr::launch_vmem_roof((int)width_bytes, tab, n_lines, distinct, iters, blocks, tab + n_lines * 16, nullptr) != 0 ||
            hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)
            return done(fail(VRHIP_ERR_HIP, "microbench launch failed"));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (rep > 0 && ms < best) best = ms;
    }
    *lane_loads_per_s = (double)blocks * 256.0 * iters * 4.0 / (best * 1e-3);
    return done(VRHIP_OK);
}

int vrhip_selftest_math(int device, int fn, const float* a, const float* b, float* out, size_t n)
{
    if (!a || !b || !out) return fail(VRHIP_ERR_INVALID, "null argument");
    if ((fn & vr::kSelftestHoisted) && (fn & ~vr::kSelftestHoisted) > 4)
        return fail(VRHIP_ERR_INVALID, "the hoisted constant form holds functions 0..4 only");
    if (n == 0) return VRHIP_OK;                          // nothing to launch
    HIP_TRY(hipSetDevice(device));
    float* d = nullptr;                                   // a, b, out: n floats each
    HIP_TRY(hipMalloc((void**)&d, 3 * n * 4));
    hipError_t e = hipMemcpy(d, a, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, b, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = (hipError_t)vr::launch_selftest_math(fn, d, d + n, d + 2 * n, n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);                                     // on every path
    if (e != hipSuccess) return fail(VRHIP_ERR_HIP, std::string("math selftest: ") + hipGetErrorString(e));
    return VRHIP_OK;
}

int vrhip_selftest_brdf(int device, const float* table, size_t n_floats, const float* frames, size_t n, float* out)
{
    if (!table || !frames || !out) return fail(VRHIP_ERR_INVALID, "null argument");
    if (n_floats != vr::kMerlFloats) return fail(VRHIP_ERR_INVALID, "BRDF table must hold 3*1458000 floats");
    if (n == 0) return VRHIP_OK;
    HIP_TRY(hipSetDevice(device));
    const std::vector<float> rgb = brdf_interleaved(table);
    float *dT = nullptr, *df = nullptr;                   // df: the frames (16 n floats), then the results (4 n)
    HIP_TRY(hipMalloc((void**)&dT, n_floats * 4));
    if (hipMalloc((void**)&df, n * 80) != hipSuccess) { (void)hipFree(dT); return fail(VRHIP_ERR_NOMEM, "selftest buffers"); }
    hipError_t e = hipMemcpy(dT, rgb.data(), n_floats * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(df, frames, n * 64, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = (hipError_t)vr::launch_selftest_brdf(dT, (const vr::vr4*)df, (vr::vr4*)(df + 16 * n), n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, df + 16 * n, n * 16, hipMemcpyDeviceToHost);
    (void)hipFree(dT); (void)hipFree(df);
    if (e != hipSuccess) return fail(VRHIP_ERR_HIP, std::string("BRDF selftest: ") + hipGetErrorString(e));
    return VRHIP_OK;
}

int vrhip_selftest_half_box(int device, const float* in, size_t n, uint16_t* down, uint16_t* up)
{
    if (!in || !down || !up) return fail(VRHIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(device));
    float* din = nullptr;
    uint16_t* dout = nullptr;                             // down, then up
    HIP_TRY(hipMalloc((void**)&din, n * 4 + 4));
    if (hipMalloc((void**)&dout, n * 4 + 4) != hipSuccess) { (void)hipFree(din); return fail(VRHIP_ERR_NOMEM, "selftest buffers"); }
    hipError_t e = hipMemcpy(din, in, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = (hipError_t)vr::launch_half_box(din, n, dout, dout + n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(down, dout, n * 2, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(up, dout + n, n * 2, hipMemcpyDeviceToHost);
    (void)hipFree(din); (void)hipFree(dout);
    if (e != hipSuccess) return fail(VRHIP_ERR_HIP, std::string("half box selftest: ") + hipGetErrorString(e));
    return VRHIP_OK;
}

static int selftest_exact(int fn, int device, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches,
                          uint32_t* first_bad)
{
    if (!mismatches || !first_bad) return fail(VRHIP_ERR_INVALID, "null argument");
    if (lo_bits > hi_bits || hi_bits > 0x80000000u) return fail(VRHIP_ERR_INVALID, "bit range outside [0, 2^31]");
    HIP_TRY(hipSetDevice(device));
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 16));
    uint32_t* df = (uint32_t*)(d + 1);
    const uint32_t init_first = 0xffffffffu;
    HIP_TRY(hipMemset(d, 0, 8));
    HIP_TRY(hipMemcpy(df, &init_first, 4, hipMemcpyHostToDevice));
    float* T = nullptr;
    if (fn == 2) {                                        // the tonemap table under test
        HIP_TRY(hipMalloc((void**)&T, 256 * sizeof(float)));
        if (vr::launch_tone_table(T, nullptr)) { (void)hipFree(d); (void)hipFree(T); return fail(VRHIP_ERR_HIP, "tone table launch failed"); }
    }
    int e = vr::launch_selftest_exact(fn, lo_bits, hi_bits, d, df, T, nullptr);
    if (e) { (void)hipFree(d); if (T) (void)hipFree(T); return fail(VRHIP_ERR_HIP, "selftest launch failed"); }
    unsigned long long n = 0;
    HIP_TRY(hipMemcpy(&n, d, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(first_bad, df, 4, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    if (T) (void)hipFree(T);
    *mismatches = n;
    return VRHIP_OK;
}

int vrhip_selftest_rcp(int device, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches, uint32_t* first_bad)
{
    return selftest_exact(0, device, lo_bits, hi_bits, mismatches, first_bad);
}

int vrhip_selftest_sqrt(int device, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches, uint32_t* first_bad)
{
    return selftest_exact(1, device, lo_bits, hi_bits, mismatches, first_bad);
}

int vrhip_selftest_tonemap(int device, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches, uint32_t* first_bad)
{
    return selftest_exact(2, device, lo_bits, hi_bits, mismatches, first_bad);
}
