"""The HIP kernels on the inputs shading sees (tests/shading_cases.py):
odd-shaped maps, uvs far outside [0, 1], zero tangents and normals, extreme
texels -- against the portable-libm oracle, over both traversal modes, three
launch kinds and a tiled render on one live context per case.

tex_addr, the HDRI lookup and the mesh / example-sphere branches of hit
materialisation (vr_kernel.hpp) are compiled into every kernel; every other
image in the suite goes through them with square power-of-two maps of one
size, a 2:1 power-of-two HDRI, unit tangents and uvs in [-1, 2).  What these
cases would catch is measured in tests/test_shading_cpu.py.

Rules.  A case without NaNs: accumulation, RGBA8 and depth8 equal the oracle
bit for bit on every pixel.  A NaN case (a normal-map texel of exactly 0.5, or
zero normals under a normal map: the shading normal is 0 / 0): RGBA8 and
depth8 equal on every pixel; accumulation equal bit for bit or NaN in both,
per channel (NaN sign and payload differ between x86 and the GPU); w never
NaN; so the NaN pixel sets are identical.  The reference fixtures of the
cases that a host build of the reference can render are compared in
tests/test_reference_fixtures.py; here the yardstick is the oracle alone.

Also here: device-built meshes with missing attributes, a refit that keeps
them, maps re-uploaded with another shape between renders and inside a
render-service session, and a float16 HDRI of odd size.
"""
import time

import numpy as np
import pytest

import pyoracle as po
import shading_cases as sh
from device_mesh_cases import BUILDERS, deform, device_build

pytestmark = pytest.mark.gpu

LAUNCH_KINDS = ("two_frames", "one_frame_launch", "one_frame_service")
SERVICE = {"two_frames": -1, "one_frame_launch": 0, "one_frame_service": 1}


# ---- comparison --------------------------------------------------------------------
def differences(got, want, where, nan_case, mask=None):
    """Failure lines of (accum, rgba8, depth8) against the oracle's, by the
    module's rules; mask: the pixels compared (all by default)."""
    out = []
    ga, wa = got[0].view(np.uint32), want[0].view(np.uint32)
    bad = ga != wa
    if nan_case:
        bad &= ~(np.isnan(got[0]) & np.isnan(want[0]))
        if np.isnan(got[0][..., 3]).any():
            out.append(f"{where} accum: a NaN depth term")
    elif np.isnan(got[0]).any():
        out.append(f"{where} accum: NaNs in a case that has none")
    for what, d, g, w in (("accum", bad.any(-1), got[0], want[0]), ("rgba8", (got[1] != want[1]).any(-1), got[1], want[1]),
                          ("depth8", (got[2] != want[2]).any(-1), got[2], want[2])):
        if mask is not None:
            d = d & mask
        if d.any():
            y, x = np.argwhere(d)[0]
            out.append(f"{where} {what}: {int(d.sum())} pixels differ, first at x={x} y={y}: "
                       f"{g[y, x].tolist()} for {w[y, x].tolist()}")
    return out


def owned_by_rank0_of_2():
    """The 16 x 16 tiles rank 0 of 2 renders: every second tile of the
    row-rotated order (include/vrhip.h vrhip_set_tiling)."""
    tiles_x = sh.W // 16
    own = np.zeros((sh.H, sh.W), bool)
    for t in range(0, tiles_x * (sh.H // 16), 2):
        ty = t // tiles_x
        tx = (t % tiles_x + ty) % tiles_x
        own[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = True
    return own


def images(r):
    return r.read_accum(), r.read_rgba8(), r.read_depth8()


def launch(r, kind, times=sh.TIMES):
    """Render `times` by a launch kind, unsynchronised as the UI does, then synchronise."""
    r.set_service(SERVICE[kind])
    if kind == "two_frames":
        r.render(frames=len(times), times=times, sync=False)
    else:
        for t in times:
            r.render(frames=1, times=[t], sync=False)
    r.sync()


def render_walk(r):
    """2 traversal modes x 3 launch kinds, then one tiled render, on a loaded
    context.  Returns [(strict, kind, launch info kind, frames, images)]."""
    out = []
    for strict in (False, True):
        for kind in LAUNCH_KINDS:
            r.set_strict_traversal(strict)
            r.clearBuffer()
            launch(r, kind)
            out.append((strict, kind, r.last_launch_info()["kind"], r.getFrameCount(), images(r)))
    r.set_strict_traversal(False)
    r.set_tiling(0, 2)
    r.clearBuffer()
    launch(r, "two_frames")
    out.append((False, "tiled", r.last_launch_info()["kind"], r.getFrameCount(), images(r)))
    r.set_tiling(0, 1)
    return out


def check_walk(r, sc, want, what, nan_case):
    """The walk of a loaded context against the oracle images `want`."""
    t0 = time.perf_counter()
    renders = render_walk(r)
    t_gpu = time.perf_counter() - t0
    has_mesh = sc.get("mesh_flat") is not None and not sc.get("example_sphere")
    failures, kinds = [], {}
    own = owned_by_rank0_of_2()
    for strict, kind, info, frames, got in renders:
        where = f"{what} [{'strict' if strict else 'culled'}, {kind} as {info}]"
        kinds[(kind, info)] = kinds.get((kind, info), 0) + 1
        if frames != len(sh.TIMES):
            failures.append(f"{where}: frame count {frames}")
        if info == "service" and (kind != "one_frame_service" or not has_mesh):
            failures.append(f"{where}: a service session where none can be")
        failures += differences(got, want, where, nan_case, own if kind == "tiled" else None)
        if kind == "tiled" and got[0][~own].any():
            failures.append(f"{where}: accumulation on tiles of the other rank")
    print(f"{what}: {len(renders)} renders in {t_gpu:.2f} s; launches {kinds}")
    if failures:
        pytest.fail(f"{what}: {len(failures)} differences from the oracle:\n" + "\n".join(failures), pytrace=False)
    if has_mesh:                                      # the render service takes mesh launches: these found a session
        assert kinds.get(("one_frame_service", "service"), 0) >= 1, kinds
    return kinds


def loaded(sc):
    from vrenderer_pathtracer_amd import VRendererHIP, scenes
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    return r


def run_case(name):
    sc = sh.make_case(name)
    want = sh.oracle_render(name)
    nan_case = name in sh.NAN_CASES
    assert bool(sh.nan_pixels(want[0]).any()) == nan_case
    r = loaded(sc)
    try:
        check_walk(r, sc, want, f"{name} ({sh.kernel_of(name)})", nan_case)
    finally:
        r.cleanUp()


# ---- 1. every case over traversal modes and launch kinds ----------------------------------------
@pytest.mark.parametrize("name", [n for n in sh.CASES if n not in sh.NAN_CASES])
def test_kernels_equal_oracle_on_shading_cases(native, oracle, name):
    run_case(name)


@pytest.mark.parametrize("name", sh.NAN_CASES)
def test_kernels_equal_oracle_on_nan_cases(native, oracle, name):
    """A NaN direction fails every slab and sphere test and ends in the HDRI
    lookup at address 0 (f2i(NaN) = 0); nothing indexes out of range."""
    run_case(name)


# ---- 2. device-resident meshes with missing attributes --------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("variant", list(sh.DEVICE_VARIANTS))
@pytest.mark.parametrize("scene", sh.DEVICE_SCENES)
def test_device_mesh_with_missing_attributes(native, oracle, scene, variant, builder):
    """normals, tangents or uvs None in initMeshDevice are zeros: the render
    equals the oracle on the exported mesh, whose missing arrays are zero."""
    sc, mesh = sh.device_scene(scene, variant), sh.device_mesh(variant)
    nan_case = variant in sh.DEVICE_NAN_VARIANTS
    r = loaded(sc)
    try:
        device_build(r, mesh, sh.LEAF, builder)
        flat = r.export_mesh_flat()
        for key in sh.DEVICE_VARIANTS[variant]:
            assert not flat[key].any(), key
        want = sh.render_on(sc, flat)
        n_nan = int(sh.nan_pixels(want[0]).sum())
        assert (sh.MIN_NAN * sh.W * sh.H <= n_nan <= sh.MAX_NAN * sh.W * sh.H) if nan_case else n_nan == 0, n_nan
        assert np.any(want[0][..., :3] != 0)
        check_walk(r, dict(sc, mesh_flat=flat), want, f"{scene} {variant} {builder}", nan_case)
    finally:
        r.cleanUp()


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("variant", [None, "no_tangents"])
def test_refit_keeps_the_attributes_it_is_not_given(native, oracle, variant, builder):
    """refitMeshDevice(positions) with normals = tangents = None keeps the
    resident ones, real or zero: the render equals the oracle on the re-exported mesh."""
    import torch
    sc, mesh = sh.device_scene("C3", variant), sh.device_mesh(variant)
    r = loaded(sc)
    try:
        device_build(r, mesh, sh.LEAF, builder)
        before = r.export_mesh_flat()
        r.refitMeshDevice(torch.from_numpy(deform(mesh["positions"])).cuda(0))
        flat = r.export_mesh_flat()
        assert flat["verts"].tobytes() != before["verts"].tobytes()
        for key in ("normals", "tangents", "uvs"):
            assert flat[key].tobytes() == before[key].tobytes(), key
        assert flat["tangents"].any() == (variant is None)
        want = sh.render_on(sc, flat)
        assert not np.isnan(want[0]).any() and np.any(want[0][..., :3] != 0)
        assert np.any(want[0] != sh.render_on(sc, before)[0])              # the refit shows in the image
        check_walk(r, dict(sc, mesh_flat=flat), want, f"refit {variant} {builder}", False)
    finally:
        r.cleanUp()


# ---- 3. maps re-uploaded with another shape ------------------------------------------------------
def load_maps(r, maps):
    for t, key in enumerate(sh.TEX_KEYS):
        r.loadTexture(maps[key], 1.0, t)
    r.loadHDR(maps["hdr"])


@pytest.mark.parametrize("session", [False, True], ids=["between_renders", "in_a_session"])
def test_maps_reuploaded_with_another_shape(native, oracle, session):
    """upload() frees and reallocates, and the size fields are written after
    the copy: a stale size or pointer would show as another image.  The frames
    before the swap equal the oracle with the first maps; frames accumulated
    across the swap equal the oracle's, rendered the same way; after a
    clearBuffer the images equal a fresh context's and the oracle's with the
    final maps.  Three swaps: every map larger, smaller, then back."""
    first = sh.make_case("S_odd_C3")
    order = ("tall", "dot", "odd")
    kind = "one_frame_service" if session else "two_frames"
    later = [t + 2018 for t in sh.TIMES]
    t0 = time.perf_counter()
    r = loaded(first)
    failures = []
    try:
        r.set_service(SERVICE[kind])
        sc = first
        for step, set_name in enumerate(order):
            # two frames with the current maps, not synchronised in a session: the upload finds it open
            r.clearBuffer()
            if session:
                for t in sh.TIMES:
                    r.render(frames=1, times=[t], sync=False)
            else:
                r.render(frames=2, times=sh.TIMES)
            nxt = dict(sc, **sh.maps_of(set_name))
            load_maps(r, nxt)
            want = po.render(sc, frames=2, times=sh.TIMES, libm=po.LIBM_PORTABLE)
            failures += differences(images(r), want[:3], f"step {step}: before the swap to {set_name}", False)
            # two more frames on the same accumulation, with the new maps
            launch(r, kind, later)
            assert r.getFrameCount() == 4
            mixed = po.render(nxt, frames=2, times=later, first_frame=3, libm=po.LIBM_PORTABLE, accum=want[0].copy())
            failures += differences(images(r), mixed[:3], f"step {step}: across the swap to {set_name}", False)
            # from a cleared buffer: a fresh context with the final maps, and the oracle
            r.clearBuffer()
            launch(r, kind)
            got = images(r)
            f = loaded(nxt)
            try:
                launch(f, kind)
                fresh = images(f)
            finally:
                f.cleanUp()
            for a, b in zip(got, fresh):
                assert a.tobytes() == b.tobytes(), f"step {step}: differs from a fresh context with the {set_name} maps"
            final = po.render(nxt, frames=2, times=sh.TIMES, libm=po.LIBM_PORTABLE)
            failures += differences(got, final[:3], f"step {step}: after the swap to {set_name}", False)
            assert np.any(final[0] != want[0])
            sc = nxt
        assert (r.service_info()["served"] > 0) == session
    finally:
        r.cleanUp()
    print(f"map swaps ({kind}): {time.perf_counter() - t0:.2f} s")
    if failures:
        pytest.fail("\n".join(failures), pytrace=False)


@pytest.mark.parametrize("shape", [(19, 53), (1, 1), (1, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_half_hdri_of_odd_size_equals_the_widened_upload(native, shape):
    """loadHDR of a float16 array (converted on the device) against the same
    texels widened on the host and uploaded as float32."""
    w, h = shape
    rng = np.random.default_rng(77)
    half = np.ones((h, w, 4), np.float16)
    half[..., :3] = rng.uniform(0.0, 4.0, (h, w, 3))
    half[0, 0, 0] = 65504.0
    half[-1, -1, 1] = 6e-8                               # a subnormal half
    sc = dict(sh.make_case("S_odd_C3"), hdr=half.astype(np.float32))
    got = {}
    for dtype in (np.float16, np.float32):
        r = loaded(sc)
        try:
            r.loadHDR(half.astype(dtype))
            r.clearBuffer()
            launch(r, "two_frames")
            got[dtype] = images(r)
        finally:
            r.cleanUp()
    for a, b in zip(got[np.float16], got[np.float32]):
        assert a.tobytes() == b.tobytes()
    assert np.any(got[np.float16][0][..., :3] != 0)
