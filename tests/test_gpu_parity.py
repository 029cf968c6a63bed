"""GPU parity: the HIP path (through the C ABI) against the CPU oracle.

Bar (DESIGN.md "Parity"):
  * vs the oracle in portable-libm mode: bit-exact accumulation, RGBA8 and
    depth images (same IEEE op sequence on both sides);
  * vs the oracle in glibc mode (the semantics the survey probe of the
    reference produced): per-pixel radiance within the north-star tolerance,
    image RMSE of accum/frames < TOL_RMSE and >= TOL_PIX_FRAC of pixels with
    max-channel |delta| <= 1e-3 (libm ulp differences are amplified by
    branch flips in a few paths; SURVEY.md 8c measured that noise floor).
"""
import os

import numpy as np
import pytest

import pyoracle as po
from vrenderer_pathtracer_amd import VRendererHIP, scenes, selftest_math, selftest_rcp, selftest_sqrt, selftest_tonemap
from vrenderer_pathtracer_amd._native import VRHIPError

pytestmark = pytest.mark.gpu

TOL_RMSE = 1e-3          # north_star: per-pixel RMSE < 1e-3 vs the reference at equal spp
TOL_PIX_FRAC = 0.995     # >= 99.5 % of pixels with max-channel |delta| <= 1e-3


def gpu_render(scene, frames=2, times=None, tiling=None, strict=False, split=None):
    r = VRendererHIP(0)
    scenes.load_into(r, scene)
    r.set_strict_traversal(strict)
    if split is not None:
        r.set_path_split(split)
    if tiling:
        r.set_tiling(*tiling)
    if times is None:
        times = [scene["time"]] * frames
    r.render(frames=frames, times=times)
    out = r.read_accum(), r.read_rgba8(), r.read_depth8(), r.getFrameCount()
    r.cleanUp()
    return out


def rendered(a, scene):
    h = (scene["height"] // 16) * 16
    w = (scene["width"] // 16) * 16
    return a[:h, :w]


def assert_bitexact(g, o, scene, what):
    g, o = rendered(g, scene), rendered(o, scene)
    if g.dtype == np.float32:
        diff = g.view(np.uint32) != o.view(np.uint32)
    else:
        diff = g != o
    n = int(diff.any(-1).sum())
    assert n == 0, f"{what}: {n} pixels differ (first at {np.argwhere(diff.any(-1))[:3].tolist()})"


@pytest.mark.parametrize("fn,name", [(0, "sin"), (1, "cos"), (2, "acos"), (3, "atan2"), (4, "pow")])
def test_device_libm_bitexact(native, oracle, fn, name):
    rng = np.random.default_rng(fn)
    n = 200000
    if fn in (0, 1):
        a = np.concatenate([rng.uniform(0, 2 * np.pi, n), rng.uniform(-40, 40, n)]).astype(np.float32)
        b = np.zeros_like(a)
    elif fn == 2:
        a = np.concatenate([rng.uniform(-1, 1, n), [-1, 1, 0, -0.0, 0.5, -0.5, 1.5]]).astype(np.float32)
        b = np.zeros_like(a)
    elif fn == 3:
        a = np.concatenate([rng.uniform(-2, 2, n), [0, -0.0, 0, 1, -1]]).astype(np.float32)
        b = np.concatenate([rng.uniform(-2, 2, n), [-1, -1, 0, 0, 0]]).astype(np.float32)
    else:
        a = np.concatenate([rng.uniform(0, 2, n), rng.uniform(0.5, 1.5, n), [0, -2, -0.5, 1, 2]]).astype(np.float32)
        b = np.concatenate([rng.uniform(0.1, 8, n), np.full(n, -1.5), [2, 3, 0.5, np.nan, np.inf]]).astype(np.float32)
    got = selftest_math(fn, a, b)
    L = oracle.lib()
    f = {0: L.vro_p_sinf, 1: L.vro_p_cosf, 2: L.vro_p_acosf, 3: L.vro_p_atan2f, 4: L.vro_p_powf}[fn]
    if fn in (3, 4):
        ref = np.array([f(float(x), float(y)) for x, y in zip(a, b)], np.float32)
    else:
        ref = np.array([f(float(x)) for x in a], np.float32)
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), f"{name}: {int((~same).sum())} mismatches, e.g. {a[~same][:3]} {got[~same][:3]} {ref[~same][:3]}"


def test_device_minmax_signed_zero(native):
    a = np.array([-0.0, 0.0, 1.0, -1.0], np.float32)
    b = np.array([0.0, -0.0, -1.0, 1.0], np.float32)
    mn = selftest_math(5, a, b)
    mx = selftest_math(6, a, b)
    # oracle/vro.c vmin/vmax: -0 < +0
    assert np.signbit(mn[0]) and np.signbit(mn[1])
    assert not np.signbit(mx[0]) and not np.signbit(mx[1])
    assert mn[2] == -1 and mx[3] == 1


def test_device_f2i_semantics(native):
    a = np.array([np.nan, 3e9, -3e9, 2.9, -2.9, 0.0], np.float32)
    got = selftest_math(7, a).view(np.int32)
    assert got.tolist() == [0, 2147483647, -2147483648, 2, -2, 0]


def test_rcp_exhaustive(native):
    # the triangle test's 1/det (rcp_rn, vr_math.hpp) equals IEEE 1.f/det for
    # every float of magnitude in [2^-32, 2^125], both signs (2.6e9 inputs);
    # only |det| >= VR_EPS (3e-10 > 2^-32) can accept a hit, larger |det|
    # takes the division
    lo = int(np.float32(2.0 ** -32).view(np.uint32))
    hi = int(np.float32(2.0 ** 125).view(np.uint32)) + 1
    n, first = selftest_rcp(lo, hi)
    assert n == 0, f"{n} mismatches, first {first:#010x}"


def test_tonemap_table_exhaustive(native):
    """The table tonemap (vr_kernel.hpp tone_byte: the hardware log2 / exp2
    estimate checked against the context's 256 thresholds) gives the byte of
    f2u8(pow(c, 1/2.2) * 255) with the f64 pow for every float c in [-0, 1]
    -- every value a clamped channel can take."""
    n, first = selftest_tonemap(0, 0x3F800001)
    assert n == 0, (n, hex(first))


def test_sqrt_exhaustive(native):
    # sqrt_rn (vr_math.hpp; sphere tests, normalisation, cosine sampling)
    # equals sqrtf for every float in [2^-96, FLT_MAX] (1.9e9 inputs); waves
    # with an input outside take sqrtf
    lo = int(np.float32(2.0 ** -96).view(np.uint32))
    hi = 0x7f800000
    n, first = selftest_sqrt(lo, hi)
    assert n == 0, f"{n} mismatches, first {first:#010x}"


@pytest.mark.parametrize("cfg,w,h,frames", [
    ("C1", 128, 128, 3),
    ("C2", 160, 96, 2),
    ("C3", 160, 96, 2),
    ("C4", 144, 96, 2),
])
def test_render_bitexact_vs_portable_oracle(native, oracle, cfg, w, h, frames):
    sc = scenes.make_scene(cfg, w, h)
    times = [12345 + 7 * i for i in range(frames)]
    ga, gr, gd, nf = gpu_render(sc, frames, times)
    oa, orgba, od, _ = po.render(sc, frames=frames, times=times, libm=po.LIBM_PORTABLE)
    assert nf == frames
    assert_bitexact(ga, oa, sc, "accum")
    assert_bitexact(gr, orgba, sc, "rgba8")
    assert_bitexact(gd, od, sc, "depth8")


@pytest.mark.parametrize("cfg,w,h,frames", [
    ("C1", 128, 128, 8),
    ("C2", 160, 96, 8),
    ("C3", 160, 96, 8),
    ("C4", 144, 96, 8),
    ("C5", 96, 64, 8),      # the 1M-triangle knot (depth-22 tree, 24-entry-stack kernels)
])
def test_render_tolerance_vs_glibc_oracle(native, oracle, cfg, w, h, frames):
    """Default (t-culled) GPU render vs the oracle with glibc's libm -- the
    semantics of the survey's probe of the reference -- at equal spp: image
    RMSE of accum/frames below the north-star 1e-3 and >= 99.5 % of pixels
    with max-channel |delta| <= 1e-3 (TOL_RMSE, TOL_PIX_FRAC)."""
    sc = scenes.make_scene(cfg, w, h)
    times = [sc["time"] + 11 * i for i in range(frames)]
    ga, _, _, _ = gpu_render(sc, frames, times)
    oa, _, _, _ = po.render(sc, frames=frames, times=times, libm=po.LIBM_GLIBC)
    g = rendered(ga, sc)[..., :3] / frames
    o = rendered(oa, sc)[..., :3] / frames
    d = np.abs(g - o).max(-1)
    rmse = float(np.sqrt(((g - o) ** 2).mean()))
    frac = float((d <= 1e-3).mean())
    print(f"{cfg} {w}x{h} {frames} frames vs glibc oracle: RMSE {rmse:.3e}, {frac:.5f} of pixels within 1e-3")
    assert rmse < TOL_RMSE, rmse
    assert frac >= TOL_PIX_FRAC, frac


@pytest.mark.parametrize("cfg,frames,rows", [
    ("C2", 8, None),             # 1280x720 x 8 frames: 14.7 M paths
    ("C3", 8, None),             # 1280x720 x 8 frames
    ("C4", 4, None),             # 1920x1080 (rendered 1920x1072) x 4 frames
    ("C5", 4, None),             # 3840x2160 x 4 frames: 66 M paths (oracle: ~10 s on 16 threads)
])
def test_render_tolerance_vs_glibc_oracle_baseline_size(native, oracle, cfg, frames, rows):
    """The north-star tolerance at the BASELINE.json resolutions: the default
    (t-culled) GPU render of the whole frame against the oracle with glibc's
    libm (the semantics of the survey's probe of the reference), per-pixel
    radiance accum/frames over the rendered rows (`rows`: an oracle/vro.c row
    range, None = all): image RMSE < TOL_RMSE and >= TOL_PIX_FRAC of pixels
    within 1e-3."""
    sc = scenes.make_scene(cfg)
    times = [sc["time"] + 13 * i for i in range(frames)]
    ga, _, _, nf = gpu_render(sc, frames, times)
    assert nf == frames
    H = (sc["height"] // 16) * 16
    r0, r1 = rows if rows else (0, H)
    oa, _, _, _ = po.render(sc, frames=frames, times=times, libm=po.LIBM_GLIBC, rows=(r0, r1))
    g = rendered(ga, sc)[r0:r1, ..., :3] / frames
    o = rendered(oa, sc)[r0:r1, ..., :3] / frames
    assert np.any(o != 0)
    d = np.abs(g - o).max(-1)
    rmse = float(np.sqrt(((g - o) ** 2).mean()))
    frac = float((d <= 1e-3).mean())
    print(f"{cfg} {sc['width']}x{sc['height']} rows {r0}-{r1} {frames} frames vs glibc oracle: RMSE {rmse:.3e}, "
          f"{frac:.6f} of {d.size} pixels within 1e-3")
    assert rmse < TOL_RMSE, rmse
    assert frac >= TOL_PIX_FRAC, frac


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C4", "C5"])
def test_render_bitexact_vs_portable_oracle_baseline_size(native, oracle, cfg):
    """Every BASELINE.json configuration at its own resolution (C2 / C3
    1280x720, C4 1920x1080, C5 3840x2160 with the 1M-triangle knot), whole
    frames, two frames in one launch, the default (t-culled) traversal:
    accum, RGBA8 and depth bit-identical to the oracle in portable-libm
    mode."""
    sc = scenes.make_scene(cfg)
    times = [sc["time"] + 5, sc["time"] + 6]
    ga, gr, gd, nf = gpu_render(sc, 2, times)
    assert nf == 2
    oa, orgba, od, _ = po.render(sc, frames=2, times=times, libm=po.LIBM_PORTABLE)
    assert np.any(rendered(oa, sc)[..., :3] != 0)
    assert_bitexact(ga, oa, sc, f"{cfg} accum")
    assert_bitexact(gr, orgba, sc, f"{cfg} rgba8")
    assert_bitexact(gd, od, sc, f"{cfg} depth8")


@pytest.mark.parametrize("cfg,w,h", [("C5", 96, 64), ("C5", 64, 48)])
def test_c5_tree_bitexact_vs_portable_oracle(native, oracle, cfg, w, h):
    """C5's 1M-triangle knot (depth-22 SBVH-class tree, the 24-entry-stack
    kernels the 4K bench runs): strict traversal bit-exact against the
    oracle (accum, RGBA8, depth), the default t-culled traversal too."""
    sc = scenes.make_scene(cfg, w, h)
    times = [sc["time"], sc["time"] + 1, sc["time"] + 2]
    oa, orgba, od, _ = po.render(sc, frames=3, times=times, libm=po.LIBM_PORTABLE)
    sa, srgba, sd, _ = gpu_render(sc, 3, times, strict=True)
    assert_bitexact(sa, oa, sc, "accum (strict)")
    assert_bitexact(srgba, orgba, sc, "rgba8 (strict)")
    assert_bitexact(sd, od, sc, "depth8 (strict)")
    ca, crgba, _, _ = gpu_render(sc, 3, times)
    assert_bitexact(ca, oa, sc, "accum (culled)")
    assert_bitexact(crgba, orgba, sc, "rgba8 (culled)")


@pytest.mark.parametrize("cfg,w,h,frames", [("C2", 160, 96, 3), ("C3", 160, 96, 2), ("C4", 144, 96, 2),
                                            ("C4", 144, 96, 8), ("C5", 96, 64, 2), ("C1", 96, 96, 3)])
def test_profiled_render_is_the_production_render(native, cfg, w, h, frames):
    """vrhip_render_profiled (the instrumented copy of the production kernels
    that the roofline's executed bytes come from) renders the same bits as
    vrhip_render, and its counts are consistent with the reference-algorithm
    counts: the same rays, no more node visits or triangle tests."""
    sc = scenes.make_scene(cfg, w, h)
    times = [sc["time"] + i for i in range(frames)]
    base = gpu_render(sc, frames, times)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    e = r.render_profiled(frames=frames, times=times)
    r_kind = r.last_launch_info()["kind"]
    got = r.read_accum(), r.read_rgba8(), r.read_depth8()
    r.set_strict_traversal(True)
    r.clearBuffer()
    ref = r.render_counted(frames=frames, times=times)
    r.cleanUp()
    for g, b, what in zip(got, base, ("accum", "rgba8", "depth8")):
        assert_bitexact(g, b, sc, what)
    assert e["node_visits_lds"] <= e["node_visits"] <= ref["node_visits"]
    assert e["tri_tests"] <= ref["tri_tests"] and e["tri_loads"] >= e["tri_tests"]
    assert e["nmap_hits"] <= e["mesh_hits"]
    # escaped camera rays of HDRI scenes are fetched once per pixel (shared_miss_paths); the
    # path pool over listed pixels (F_SPARSE) pads its last chunk of each path index with
    # the last listed pixel, whose duplicate paths (< 64 per path index) are counted too
    pad = 63 * 2 * frames if r_kind == "path_pool" else 0
    assert e["hdr_fetches"] <= ref["hdr_fetches"] + 4 * pad and e["brdf_fetches"] <= ref["brdf_fetches"] + 4 * pad
    assert e["hdr_fetches"] + e["shared_miss_paths"] >= ref["hdr_fetches"]
    if sc.get("mesh_flat") is None:
        assert e["node_visits"] == 0 and e["mesh_hits"] == 0
    else:
        assert e["mesh_hits"] > 0 and e["tri_loads"] > 0


def test_vmem_roof_microbench(native):
    """The live gather-roof micro-benchmark (vrhip_microbench_vmem) runs and
    reports finite, ordered rates for every load width."""
    from vrenderer_pathtracer_amd import microbench_vmem
    for w in (16, 12, 8, 4):
        rates = [microbench_vmem(w, d) for d in (1, 64)]
        print(f"b{8 * w}: {rates[0] / 1e9:.1f} / {rates[1] / 1e9:.1f} G lane-loads/s (1 / 64 addresses per instruction)")
        assert all(1e9 < x < 1e14 for x in rates)


def test_comm_gather_single_rank_through_c_abi(native):
    """vrhip_comm_unique_id / _init / _gather / _destroy (RCCL ncclGather) on a
    one-rank communicator: the gathered RGBA8 and accumulation equal the plain
    render (RCCL refuses two ranks on one GPU; the 8-GPU path runs in the
    driver's scaling bench, the multi-rank logic in the gloo tests)."""
    from vrenderer_pathtracer_amd.renderer import comm_unique_id
    from vrenderer_pathtracer_amd.tiles import WHAT_ACCUM, WHAT_RGBA8
    sc = scenes.make_scene("C2", 160, 96)
    times = [sc["time"], sc["time"] + 1]
    base = gpu_render(sc, 2, times)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.comm_init(0, 1, comm_unique_id())
    # the gather buffers are sized for the communicator's tiling: changing
    # it while the communicator exists is refused (vrhip_set_tiling)
    with pytest.raises(VRHIPError):
        r.set_tiling(0, 2)
    r.render(frames=2, times=times, sync=False)
    r.comm_gather(WHAT_RGBA8)
    r.comm_gather(WHAT_ACCUM)
    r.sync()
    acc, rgba = r.read_accum(), r.read_rgba8()
    r.comm_destroy()
    r.set_tiling(0, 2)              # free again once the communicator is gone
    r.set_tiling(0, 1)
    r.cleanUp()
    assert_bitexact(acc, base[0], sc, "accum")
    assert_bitexact(rgba, base[1], sc, "rgba8")


def test_grid_truncation_untouched_rows(native, oracle):
    # 1920x1080-like truncation: rows >= (H/16)*16 are never rendered (PathTracer.cu:888-889)
    sc = scenes.make_scene("C1", 72, 40)
    ga, _, _, _ = gpu_render(sc, 1)
    assert np.all(ga[32:] == 0) and np.all(ga[:, 64:] == 0)
    assert np.any(ga[:32, :64, :3] != 0)


@pytest.mark.parametrize("n", [3, 8])
def test_tiling_union_equals_single_gpu(native, n):
    from vrenderer_pathtracer_amd.tiles import owned_pixels
    sc = scenes.make_scene("C2", 160, 112)
    W, H = sc["width"], sc["height"]
    full, rgba, depth, _ = gpu_render(sc, 2)
    acc = np.zeros_like(full).reshape(H * W, 4)
    seen = np.zeros(H * W, bool)
    for rank in range(n):
        part, prgba, pdepth, _ = gpu_render(sc, 2, tiling=(rank, n))
        pix = owned_pixels(W, H, rank, n)
        mine = np.zeros(H * W, bool)
        mine[pix] = True
        assert not seen[pix].any()
        seen |= mine
        acc[pix] = part.reshape(H * W, 4)[pix]
        assert np.all(part.reshape(H * W, 4)[~mine] == 0)                 # nothing outside our tiles
        assert np.array_equal(prgba.reshape(H * W, 4)[pix], rgba.reshape(H * W, 4)[pix])
        assert np.array_equal(pdepth.reshape(H * W, 4)[pix], depth.reshape(H * W, 4)[pix])
    assert np.array_equal(acc.view(np.uint32), full.reshape(H * W, 4).view(np.uint32))


def test_device_pack_unpack_matches_host(native):
    """vrhip_pack_tiles / vrhip_unpack_tiles against the host packing of the same tiles."""
    import torch
    from vrenderer_pathtracer_amd.tiles import WHAT_ACCUM, pack_host, max_owned_pixels
    sc = scenes.make_scene("C1", 96, 80)
    W, H = sc["width"], sc["height"]
    n = 4
    cap = max_owned_pixels(W, H, n)
    recv = torch.zeros(n * cap * 16, dtype=torch.uint8, device="cuda")
    full = None
    for rank in range(n):
        r = VRendererHIP(0)
        scenes.load_into(r, sc)
        r.set_tiling(rank, n)
        r.render(frames=1, times=[sc["time"]])
        accum = r.read_accum()
        buf = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()          # the zero-fill runs on torch's stream, the pack on the renderer's
        r.pack_tiles(WHAT_ACCUM, buf.data_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.float32).reshape(cap, 4)[:r.owned_pixels()]
        assert np.array_equal(got.view(np.uint32), pack_host(accum, rank, n).view(np.uint32))
        recv[rank * cap * 16:(rank + 1) * cap * 16] = buf
        r.cleanUp()
    ref, _, _, _ = gpu_render(sc, 1, [sc["time"]])
    g = VRendererHIP(0)
    scenes.load_into(g, sc)
    g.unpack_tiles(WHAT_ACCUM, recv.data_ptr(), n, cap * 16)
    g.sync()
    full = g.read_accum()
    g.cleanUp()
    assert_bitexact(full, ref, sc, "unpacked accum")


@pytest.mark.parametrize("cfg,frames", [("C2", 3), ("C3", 2), ("C4", 5), ("C1", 8)])
def test_path_split_is_result_invariant(native, cfg, frames):
    """Splitting a pixel's 2k paths over workgroups (vrhip_set_path_split) changes nothing."""
    sc = scenes.make_scene(cfg, 96, 64)
    times = [sc["time"] + 7 * i for i in range(frames)]
    base = gpu_render(sc, frames, times, split=1)
    for split in (2, 3, 4, 2 * frames, 0):
        got = gpu_render(sc, frames, times, split=split)
        assert_bitexact(got[0], base[0], sc, f"accum split={split}")
        assert_bitexact(got[1], base[1], sc, f"rgba split={split}")
        assert_bitexact(got[2], base[2], sc, f"depth split={split}")


@pytest.mark.parametrize("cfg,w,h,frames,tiling", [("C4", 144, 96, 8, None), ("C4", 96, 64, 70, None),
                                                    ("C4", 144, 96, 6, (1, 3)), ("C4", 400, 240, 4, None)])
def test_split_sphere_launch_bitexact_vs_portable_oracle(native, oracle, cfg, w, h, frames, tiling):
    """Sphere-only HDRI scenes, launches of >= 4 frames: each pixel's paths in
    4 path groups (VR_SPHERE_SPLIT), an escaped pixel's one shared result
    stored once (kSharedMissW) -- equal to the oracle and to render_kernel's
    direct accumulation (one path group) bit for bit, also over several
    launches (70 frames) and on a tiled rank."""
    sc = scenes.make_scene(cfg, w, h)
    times = [sc["time"] + 5 * i for i in range(frames)]
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    if tiling:
        r.set_tiling(*tiling)
    r.render(frames=frames, times=times)
    info = r.last_launch_info()
    got = r.read_accum(), r.read_rgba8(), r.read_depth8()
    r.cleanUp()
    assert info["kind"] == "render_kernel" and info["use_scratch"] == 1 and info["split"] >= 4, info
    direct = gpu_render(sc, frames, times, tiling=tiling, split=1)
    for g, b, what in zip(got, direct, ("accum", "rgba8", "depth8")):
        assert_bitexact(g, b, sc, f"{what} vs one path group")
    if tiling is None:
        oa, orgba, od, _ = po.render(sc, frames=frames, times=times, libm=po.LIBM_PORTABLE)
        assert_bitexact(got[0], oa, sc, "accum vs oracle")
        assert_bitexact(got[1], orgba, sc, "rgba8 vs oracle")
        assert_bitexact(got[2], od, sc, "depth8 vs oracle")


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C5"])
@pytest.mark.parametrize("sync", [True, False])
def test_multi_frame_launch_equals_frame_by_frame(native, cfg, sync):
    """One frame per call -- mesh scenes then trace the camera ray inside the
    path kernel (no primary pass), synchronous calls run on the context stream
    and unsynchronised ones overlap on the path streams -- accumulates exactly
    what one multi-frame launch (shared primary records) does."""
    sc = scenes.make_scene(cfg, 64, 64) if cfg != "C5" else scenes.make_scene(cfg, 96, 64)
    times = [sc["time"] + i for i in range(4)] if cfg != "C1" else [5, 6, 7, 8]
    a4, r4, d4, _ = gpu_render(sc, 4, times)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    for t in times:
        r.render(frames=1, times=[t], sync=sync)
    a1, rgba1, d1 = r.read_accum(), r.read_rgba8(), r.read_depth8()
    assert r.getFrameCount() == 4
    r.cleanUp()
    assert np.array_equal(a4.view(np.uint32), a1.view(np.uint32))
    assert np.array_equal(r4, rgba1) and np.array_equal(d4, d1)


def test_pipelined_steps_bitexact_vs_portable_oracle(native, oracle):
    """Back-to-back render calls without a sync (the launches of consecutive
    calls overlap on the two path streams) accumulate exactly what the
    oracle's frame-by-frame loop does."""
    sc = scenes.make_scene("C2", 96, 64)
    times = [sc["time"] + 3 * i for i in range(7)]
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.render(frames=2, times=times[0:2], sync=False)
    r.render(frames=1, times=times[2:3], sync=False)
    r.render(frames=4, times=times[3:7], sync=False)
    got = r.read_accum(), r.read_rgba8(), r.read_depth8()
    assert r.getFrameCount() == 7
    r.cleanUp()
    ref = po.render(sc, frames=7, times=times, libm=po.LIBM_PORTABLE)
    for g, o, what in zip(got, ref, ("accum", "rgba8", "depth8")):
        assert_bitexact(g, o, sc, what)


@pytest.mark.parametrize("cfg,overlap", [("C3", 1), ("C4", 1), ("C3", 0)])
def test_pipelined_steps_with_scene_changes_equal_synchronous(native, cfg, overlap):
    """Uploads, Fresnel and tiling changes between unsynchronised render calls
    take effect exactly where they were issued (the path streams join the
    render stream after any buffer change), with and without launch overlap."""
    sc = scenes.make_scene(cfg, 96, 64)
    t = sc["time"]

    def run(sync):
        r = VRendererHIP(0)
        scenes.load_into(r, sc)
        r.set_overlap(overlap)
        r.render(frames=2, times=[t, t + 1], sync=sync)
        r.render(frames=3, times=[t + 2, t + 3, t + 4], sync=sync)
        r.loadHDR(np.ascontiguousarray(sc["hdr"][::-1]))
        r.render(frames=2, times=[t + 5, t + 6], sync=sync)
        r.setFresnelCoef(0.4)
        r.render(frames=1, times=[t + 7], sync=sync)
        r.set_tiling(0, 2)
        r.render(frames=2, times=[t + 8, t + 9], sync=sync)
        out = r.read_accum(), r.read_rgba8(), r.getFrameCount()
        r.cleanUp()
        return out

    a_sync, c_sync, n_sync = run(True)
    a_pipe, c_pipe, n_pipe = run(False)
    assert n_sync == n_pipe
    assert np.array_equal(a_sync.view(np.uint32), a_pipe.view(np.uint32))
    assert np.array_equal(c_sync, c_pipe)


def _random_soup(seed, n, leaf, cluster=1):
    """n random triangles; with cluster > 1, groups of `cluster` near-copies
    of one triangle (boxes no split separates: leaves of up to `leaf`)."""
    from vrenderer_pathtracer_amd import build_flat
    rng = np.random.default_rng(seed)
    c = np.repeat(rng.uniform(-30, 30, (n // cluster, 1, 3)), cluster, axis=0)
    if cluster == 1:
        P = (c + rng.normal(0, 4, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    else:                             # near-copies of one triangle per group
        base = np.repeat(rng.normal(0, 4, (n // cluster, 3, 3)), cluster, axis=0)
        P = (c + base + rng.normal(0, 0.05, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    T = rng.normal(0, 1, (3 * n, 3)).astype(np.float32)
    m = dict(positions=P, normals=(T / np.linalg.norm(T, axis=1, keepdims=True)).astype(np.float32),
             tangents=np.tile([1, 0, 0], (3 * n, 1)).astype(np.float32),
             uvs=rng.uniform(0, 1, (3 * n, 2)).astype(np.float32),
             tris=np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))
    return build_flat(m, max_leaf_tris=leaf)


@pytest.mark.parametrize("cfg,leaf", [("C2", 3), ("C3", 5), ("C2", 1), ("C2", 16), ("C3", 40)])
def test_random_soup_bitexact_vs_portable_oracle(native, oracle, cfg, leaf):
    """Overlapping random triangles (odd leaf sizes exercise the paired
    triangle loads' tail): strict traversal bit-exact against the oracle, the
    default t-culled traversal equal to strict (DESIGN.md "Equal-t ties": the
    tie-break makes the hit independent of the visit order; what could still
    differ is a triangle whose hit distance exceeds the slab entry of its box
    by more than the 2^-10 culling margin through fp32 rounding -- none
    measured)."""
    sc = scenes.make_scene(cfg, 96, 64)
    sc["mesh_flat"] = _random_soup(11 + leaf, 1500, leaf, cluster=20 if leaf > 8 else 1)
    if leaf > 8:                      # wide leaves reach the leaf loop's longer runs of pairs
        v = sc["mesh_flat"]["verts"].view(np.uint32)
        ends = np.flatnonzero((v[:, 0] == 0x80000000) & (v[:, 1] == 0) & (v[:, 2] == 0))
        assert int(np.diff(np.concatenate([[-1], ends])).max() - 1) // 3 > 8
    times = [sc["time"], sc["time"] + 1]
    oa, orgba, _, _ = po.render(sc, frames=2, times=times, libm=po.LIBM_PORTABLE)
    sa, srgba, _, _ = gpu_render(sc, 2, times, strict=True)
    assert_bitexact(sa, oa, sc, "accum (strict)")
    assert_bitexact(srgba, orgba, sc, "rgba8 (strict)")
    ca, _, _, _ = gpu_render(sc, 2, times)
    diff = (rendered(ca, sc).view(np.uint32) != rendered(sa, sc).view(np.uint32)).any(-1)
    assert int(diff.sum()) == 0, int(diff.sum())


@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_stack24_tree_bitexact_vs_portable_oracle(native, oracle, cfg):
    """The torus knot with one triangle per leaf is 16 levels deep, so the
    launches take the 24-entry-stack kernels (trees of depth 16-23, C5's
    class): strict bit-exact against the oracle, culled equal to strict."""
    from vrenderer_pathtracer_amd import build_flat, validate_flat
    sc = scenes.make_scene(cfg, 96, 64)
    sc["mesh_flat"] = build_flat(scenes.torus_knot(100, 50), max_leaf_tris=1)
    depth, _ = validate_flat(sc["mesh_flat"])
    assert 15 < depth <= 23, depth
    times = [sc["time"], sc["time"] + 1]
    oa, orgba, _, _ = po.render(sc, frames=2, times=times, libm=po.LIBM_PORTABLE)
    sa, srgba, _, _ = gpu_render(sc, 2, times, strict=True)
    assert_bitexact(sa, oa, sc, "accum (strict)")
    assert_bitexact(srgba, orgba, sc, "rgba8 (strict)")
    ca, _, _, _ = gpu_render(sc, 2, times)
    diff = (rendered(ca, sc).view(np.uint32) != rendered(sa, sc).view(np.uint32)).any(-1)
    assert int(diff.sum()) == 0, int(diff.sum())


@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_large_and_small_launch_blocks_agree(native, cfg):
    """A 20-frame 1280x720 launch (36.9 M paths) runs the path kernel in
    768-thread blocks (C3; C2's Cornell kernel: 256-thread blocks at 7 waves)
    on 64 queue heads, one frame per call (1.8 M paths) in 256-thread blocks on
    16: the accumulations are identical bit for bit."""
    sc = scenes.make_scene(cfg)
    times = [sc["time"] + i for i in range(20)]
    big, _, _, n_big = gpu_render(sc, 20, times)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    for t in times:
        r.render(frames=1, times=[t])
    small, n_small = r.read_accum(), r.getFrameCount()
    r.cleanUp()
    assert n_big == n_small
    assert np.array_equal(big.view(np.uint32), small.view(np.uint32))


@pytest.mark.parametrize("overlap", [1, 0])
def test_more_frames_than_one_launch_bitexact(native, oracle, overlap):
    """A render call of 70 frames is two launches (64 + 6); with overlap they
    run on different path streams."""
    sc = scenes.make_scene("C2", 32, 32)
    times = [sc["time"] + i for i in range(70)]
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.set_overlap(overlap)
    r.render(frames=70, times=times)
    got = r.read_accum()
    assert r.getFrameCount() == 70
    r.cleanUp()
    ref, _, _, _ = po.render(sc, frames=70, times=times, libm=po.LIBM_PORTABLE)
    assert_bitexact(got, ref, sc, "accum")


def test_single_tile_and_empty_rank(native, oracle):
    """One 16x16 tile (4 chunks per path for 256 resident blocks) renders
    correctly; a rank that owns no tile renders nothing and does not hang."""
    sc = scenes.make_scene("C3", 16, 16)
    times = [sc["time"], sc["time"] + 1]
    a, _, _, _ = gpu_render(sc, 2, times)
    ref, _, _, _ = po.render(sc, frames=2, times=times, libm=po.LIBM_PORTABLE)
    assert_bitexact(a, ref, sc, "accum")
    empty, _, _, nf = gpu_render(sc, 2, times, tiling=(1, 2))
    assert nf == 2 and not empty.any()


@pytest.mark.parametrize("cfg,w,h,overlap", [("C2", 16, 16, 1), ("C3", 32, 16, -1), ("C2", 48, 32, 0)])
def test_tiny_one_frame_calls_bitexact(native, oracle, cfg, w, h, overlap):
    """One-frame launches far smaller than the resident pool: almost every
    wave finds the queues drained at once and retires through the launch's
    drained-queue mask (vr_kernel.hip grab), back to back on one or three
    path streams; the accumulation equals the oracle bit for bit."""
    sc = scenes.make_scene(cfg, w, h)
    times = [sc["time"] + 3 * i for i in range(6)]
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.set_overlap(overlap)
    for t in times:
        r.render(frames=1, times=[t], sync=False)
    r.sync()
    acc = r.read_accum()
    nf = r.getFrameCount()
    r.cleanUp()
    ref, _, _, _ = oracle.render(sc, frames=len(times), times=times, libm=oracle.LIBM_PORTABLE)
    assert nf == len(times)
    assert_bitexact(acc, ref, sc, f"{cfg} {w}x{h} one-frame calls")


@pytest.mark.parametrize("cfg,w,h", [("C2", 96, 64), ("C3", 96, 64), ("C4", 96, 64)])
def test_strict_counts_equal_oracle_counts(native, oracle, cfg, w, h):
    """Strict traversal visits exactly the nodes and tests exactly the
    triangles the reference algorithm does (oracle counting mode)."""
    sc = scenes.make_scene(cfg, w, h)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.set_strict_traversal(True)
    g = r.render_counted(frames=1, time_seed=sc["time"])
    r.set_strict_traversal(False)
    r.clearBuffer()
    gc = r.render_counted(frames=1, time_seed=sc["time"])
    r.cleanUp()
    _, _, _, o = po.render(sc, frames=1, count=True, libm=po.LIBM_PORTABLE)
    assert g["rays"] == o["rays"]
    assert g["node_visits"] == o["node_visits"]
    assert g["tri_tests"] == o["tri_tests"]
    assert g["hdr_fetches"] == o["hdr_fetches"] and g["brdf_fetches"] == o["brdf_fetches"]
    assert gc["rays"] == o["rays"] and gc["node_visits"] <= o["node_visits"]
    print(f"{cfg}: nodes/ray strict {g['node_visits'] / g['rays']:.2f} culled {gc['node_visits'] / gc['rays']:.2f}; "
          f"tris/ray strict {g['tri_tests'] / g['rays']:.2f} culled {gc['tri_tests'] / gc['rays']:.2f}")


@pytest.mark.parametrize("cfg,w,h", [("C2", 160, 96), ("C3", 160, 96)])
def test_strict_traversal_bitexact_vs_portable_oracle(native, oracle, cfg, w, h):
    sc = scenes.make_scene(cfg, w, h)
    ga, gr, gd, _ = gpu_render(sc, 2, strict=True)
    oa, orgba, od, _ = po.render(sc, frames=2, libm=po.LIBM_PORTABLE)
    assert_bitexact(ga, oa, sc, "accum")
    assert_bitexact(gr, orgba, sc, "rgba8")


@pytest.mark.parametrize("cfg,frames", [("C2", 2), ("C3", 2), ("C5", 1)])
def test_culled_vs_strict_full_frame(native, cfg, frames):
    """t-culled traversal against the reference's visit-every-pierced-box
    traversal at full BASELINE resolution: identical (DESIGN.md "Equal-t
    ties" and the 2^-10 culling margin; 0 pixels measured since round 2)."""
    sc = scenes.make_scene(cfg)
    a_cull, _, _, _ = gpu_render(sc, frames)
    a_strict, _, _, _ = gpu_render(sc, frames, strict=True)
    diff = (rendered(a_cull, sc).view(np.uint32) != rendered(a_strict, sc).view(np.uint32)).any(-1)
    n = int(diff.sum())
    print(f"{cfg}: {n} of {diff.size} pixels differ between culled and strict traversal")
    assert n == 0


@pytest.mark.parametrize("cfg,tiling,overlap,size", [("C3", None, 0, (160, 112)), ("C2", (1, 3), -1, (160, 112)),
                                                     ("C5", (0, 2), 1, (96, 64)),
                                                     ("C2", None, 0, (320, 224)), ("C2", None, 1, (320, 224))])
def test_longest_first_order_is_scheduling_only(native, oracle, cfg, tiling, overlap, size):
    """Small launches (one frame per call, shards) take their sub-tiles in the
    order the previous launch on the same scratch measured (per-path costs
    summed per sub-tile by the finish pass, sorted per XCD by order_kernel).
    Consecutive one-frame calls -- the second and later ones ordered, on one
    path stream or on three -- equal the band-order render bit for bit, and
    the oracle.  320x224 has 1,120 sub-tiles, more than 8 XCDs x
    kXcdBands = 1,024: the order lists' second band (g >= 1 in grab's
    lookup, every 720p and 4K one-frame launch) is exercised too."""
    w, h = size
    sc = scenes.make_scene(cfg, w, h) if cfg != "C5" else scenes.make_scene("C5", w, h, knot=(150, 75))
    times = [sc["time"] + 7 * i for i in range(7)]
    outs = []
    for order in ("1", "0"):
        old = os.environ.get("VRHIP_COST_ORDER")
        os.environ["VRHIP_COST_ORDER"] = order
        try:
            r = VRendererHIP(0)
        finally:
            if old is None:
                del os.environ["VRHIP_COST_ORDER"]
            else:
                os.environ["VRHIP_COST_ORDER"] = old
        scenes.load_into(r, sc)
        r.set_overlap(overlap)
        if tiling:
            r.set_tiling(*tiling)
        for t in times:
            r.render(frames=1, times=[t], sync=False)
        r.sync()
        outs.append((r.read_accum(), r.read_rgba8()))
        r.cleanUp()
    (acc1, rgba1), (acc0, rgba0) = outs
    assert np.array_equal(acc1.view(np.uint32), acc0.view(np.uint32))
    assert np.array_equal(rgba1, rgba0)
    if tiling is None:
        ref, _, _, _ = oracle.render(sc, frames=len(times), times=times, libm=oracle.LIBM_PORTABLE)
        assert_bitexact(acc1, ref, sc, f"{cfg} ordered one-frame calls")


@pytest.mark.parametrize("halves", [True, False])
def test_hdr_storage_bitexact_vs_portable_oracle(native, oracle, halves):
    """Environment maps whose values are all halves (the reference's
    Imf::Rgba input, and the procedural map) and float maps that are not
    (every colour one ulp above a half) both equal the oracle bit for bit.
    (A half4 device copy of half-valued maps was measured and not kept:
    DESIGN.md section 4 table.)"""
    sc = scenes.make_scene("C3", 96, 64)
    if not halves:
        h = sc["hdr"].copy()
        h[..., :3] = np.nextafter(h[..., :3], np.float32(np.inf))
        assert not np.array_equal(h.astype(np.float16).astype(np.float32), h)
        sc["hdr"] = h
    times = [sc["time"], sc["time"] + 1]
    oa, orgba, _, _ = po.render(sc, frames=2, times=times, libm=po.LIBM_PORTABLE)
    ga, grgba, _, _ = gpu_render(sc, 2, times)
    assert_bitexact(ga, oa, sc, "accum")
    assert_bitexact(grgba, orgba, sc, "rgba8")


def test_kernel_timing_switch(native):
    """vrhip_set_kernel_timing(0) (the Qt adapter's setting): no kernel-span
    events on the launch path -- kernel_stats counts no launch and
    last_kernel_ms reads 0 -- and the images are those of the default; back
    on, the next launch is timed again."""
    sc = scenes.make_scene("C2", 96, 64)
    times = [sc["time"] + i for i in range(3)]

    def run(timing):
        r = VRendererHIP(0)
        scenes.load_into(r, sc)
        r.set_kernel_timing(timing)
        r.kernel_stats(reset=True)
        for t in times:
            r.render(frames=1, times=[t])
        ms, n = r.kernel_stats()
        last = r.last_kernel_ms()
        out = r.read_accum(), r.read_rgba8()
        if not timing:
            r.set_kernel_timing(True)
            r.render(frames=1, times=[times[-1] + 1])
            ms2, n2 = r.kernel_stats()
            assert n2 == 1 and ms2 > 0 and r.last_kernel_ms() > 0
        r.cleanUp()
        return out, n, last

    (a0, c0), n0, last0 = run(False)
    (a1, c1), n1, last1 = run(True)
    assert n0 == 0 and last0 == 0.0
    assert n1 == 3 and last1 > 0
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(c0, c1)
