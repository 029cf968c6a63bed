"""The surface query without a device (vrhip_trace_surface, vrhip_camera_rays).

The yardstick first (tests/surface_cases.py): the oracle's own intersect_scene
on arbitrary rays, with the closest sphere restated and the mesh part from the
product's host walk.  Here the restated parts are tied to the oracle's record
(o + d * t is its hitPoint bit for bit, the sphere named has its colour and
emission), the record is tied to the reference-pinned renders through the
depth image, and the conditions on the ray sets are asserted.  Then what the C
ABI refuses before any device call, and the size of the record."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import flag_lattice as fl
import pyoracle as po
import radiance_cases as rc
import shading_cases as sh
import surface_cases as sf

SCENES = [(n, "shallow") for n in sf.COMBO_NAMES + sf.SHADING_NAMES] + [("cornell+mesh", "deep")]
IDS = [n if m == "shallow" else f"{n}-{m}" for n, m in SCENES]


def depth_of(o, position):
    """trace's depth term of a first hit (vro.c trace, :656-661) in float32."""
    l = np.asarray(o, np.float32) - np.asarray(position, np.float32)
    dd = (l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2]
    out = np.sqrt(dd) / np.float32(150.0)
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("name,mesh", SCENES, ids=IDS)
def test_restated_hit_agrees_with_the_oracle(oracle, native, name, mesh):
    sc = sf.scene_named(name, mesh)
    for which in sf.sets_of(sc):
        o, d = sf.ray_set(which, sc)
        rec, ok = sf.reference(name, which, mesh)
        f = sf.floats(rec)
        hit = rec[:, sf.KIND] != sf.NONE
        assert hit.any()
        # the restated t: the oracle computed its hitPoint as o + d * t from the t it kept
        with np.errstate(all="ignore"):
            hp = o + sf.normalised(d) * f[:, sf.T:sf.T + 1]
        assert hp.dtype == np.float32
        assert (sf.u32(hp[hit]) == rec[hit, sf.POSITION]).all(), f"{name} set {which}"
        assert np.isfinite(f[hit, sf.T]).all() and (f[hit, sf.T] > 0).all() and (f[hit, sf.T] < sf.NO_HIT).all()
        # the restated sphere: the one whose colour and emission the record holds
        for kind, count in ((sf.CORNELL, 6), (sf.SMALL, 2), (sf.EXAMPLE, 1)):
            for index in range(count):
                rows = (rec[:, sf.KIND] == kind) & (rec[:, sf.PRIM] == index)
                color, emission = sf.sphere_of(kind, index)
                assert (rec[rows, sf.EMISSION] == sf.u32(emission)).all(), (name, which, kind, index)
                if kind != sf.EXAMPLE or sc.get("tex_diffuse") is None or sc.get("view_brdf"):
                    assert (rec[rows, sf.COLOR] == sf.u32(color)).all(), (name, which, kind, index)
            assert (rec[rec[:, sf.KIND] == kind, sf.PRIM] < count).all()
        # what only a mesh hit carries
        mesh_hit = rec[:, sf.KIND] == sf.MESH
        assert not rec[~mesh_hit][:, [sf.BARY_U, sf.BARY_V, sf.TEX_U, sf.TEX_V]].any()
        assert not rec[:, [sf.PAD0, sf.PAD1]].any()
        # a miss is {1e20, NONE, MISS, 0 ...}
        miss = rec[~hit]
        assert (miss[:, sf.T] == sf.u32(sf.NO_HIT)).all() and (miss[:, sf.PRIM] == sf.MISS).all() and not miss[:, 3:].any()
        # normals are unit vectors where they are finite
        n = f[hit][:, sf.NORMAL]
        fin = np.isfinite(n).all(-1)
        assert np.allclose((n[fin] * n[fin]).sum(-1), 1.0, atol=1e-5)
        if sf.nan_case(name):
            assert ok.all()
        else:
            assert (ok == sf.finite(rec)).all() and (~ok).sum() <= sf.MAX_DROPPED * len(ok)


@pytest.mark.parametrize("name,mesh", SCENES, ids=IDS)
def test_ray_sets_reach_every_kind(oracle, native, name, mesh):
    """The caps on the yardstick itself: every kind the scene can produce at
    least 16 times over its sets, at least 400 rays of C on the mesh."""
    counts = sf.check_coverage(name, mesh)
    print(f"{name} {mesh}: {counts}")
    sc = sf.scene_named(name, mesh)
    assert sum(counts.values()) == sum(len(sf.ray_set(w, sc)[0]) for w in sf.sets_of(sc))


@pytest.mark.parametrize("name", sf.ZERO_TANGENT_CASES + tuple(n for n in sf.SHADING_NAMES if n in sh.NAN_CASES))
def test_where_the_nans_are(oracle, native, name):
    """Zero tangents: the tangent of every mesh hit is NaN (the reference's
    normalize of a zero vector) and no other word of any record is.  The NaN
    shading case: NaN records are a minority, and t and the position are never NaN."""
    sc = sf.scene_named(name)
    for which in sf.sets_of(sc):
        rec, ok = sf.reference(name, which)
        f = sf.floats(rec).copy()
        f[:, [sf.KIND, sf.PRIM, sf.TYPE]] = 0.0
        bad = ~np.isfinite(f)
        assert not np.isinf(f).any()
        mesh_hit = rec[:, sf.KIND] == sf.MESH
        if name in sf.ZERO_TANGENT_CASES:
            assert bad[mesh_hit][:, sf.TANGENT].all() and mesh_hit.any()
            bad[:, sf.TANGENT] = False
            assert not bad.any()
        else:
            rows = bad.any(-1)
            print(f"{name} set {which}: {int(rows.sum())} of {len(rows)} records hold a NaN")
            assert not rows[~mesh_hit].any() and 1 <= rows[mesh_hit].sum() < mesh_hit.sum() // 2
            assert not bad[:, sf.T].any() and not bad[:, sf.POSITION].any()
    got = np.zeros((2, sf.WORDS), np.uint32)
    want = got.copy()
    got[:, sf.NORMAL], want[0, sf.NORMAL], want[1, sf.NORMAL] = 0x7FC00000, 0xFFC00001, sf.u32(np.float32(0.5))
    got[:, sf.KIND] = want[:, sf.KIND] = 0x7FC00000                   # an integer word is never a NaN
    assert sf.same_or_nan_in_both(got, want).tolist() == [True, False]
    want[0, sf.KIND] = 0x7FC00001
    assert sf.same_or_nan_in_both(got, want).tolist() == [False, False]


@pytest.mark.parametrize("name", sf.COMBO_NAMES)
def test_yardstick_equals_the_oracle_render(oracle, native, name):
    """Set A is the camera: where a pixel's camera ray hits, the depth image
    of pyoracle.render's first frame shows the depth term of the yardstick's
    position -- unless the frame's last path left the Cornell box on a later
    bounce, which returns w = 0 (vro.c trace, :649-652); at a miss it shows the
    miss value."""
    sc = fl.scene_of(rc.combo_of(name))
    _, _, depth, _ = po.render(sc, frames=1, times=[rc.TIME], libm=po.LIBM_PORTABLE)
    o, d = sf.ray_set("A", sc)
    rec, ok = sf.reference(name, "A")
    assert ok.all()
    hit = rec[:, sf.KIND] != sf.NONE
    want = rc.depth_byte(depth_of(o, sf.floats(rec)[:, sf.POSITION]))
    want[~hit] = rc.depth_byte(np.float32(0.0 if sc["cornell"] else 1.0))
    shown = depth[..., 0].reshape(-1)
    differ = shown != want
    if sc["cornell"]:                                 # a path that escaped after its first hit: white
        paths, _ = rc.reference(name, "A")
        escaped = hit & (paths[:, 1, 3] == 0.0)
        assert (shown[escaped] == 255).all()
        differ &= ~escaped
        assert escaped.sum() <= 4
    assert not differ.any(), f"{name}: {int(differ.sum())} pixels"
    assert hit.sum() > 900 if sc["cornell"] else hit.sum() >= 30
    assert len(np.unique(want[hit])) > 8


def test_set_c_is_aimed_at_the_mesh():
    flat = fl.mesh_of("shallow")
    tris = sf.triangles_of(flat)
    v = np.asarray(flat["verts"], np.float32).reshape(-1, 4)
    assert tris.shape[1:] == (3, 3) and 3 * len(tris) == (v[:, 0].view(np.uint32) != 0x80000000).sum()
    o, d = sf.aimed_rays(flat)
    assert o.shape == d.shape == (512, 3) and np.abs(o).max() <= 40.0
    length = np.sqrt((d.astype(np.float64) ** 2).sum(-1))
    assert length.min() >= 0.1 - 1e-6 and length.max() <= 10.0 + 1e-6
    o2, d2 = sf.ray_set("D")
    assert o2.shape == d2.shape == (64, 3)


# ---- the C ABI ----------------------------------------------------------------------------------
def test_symbols_are_exported(native):
    assert hasattr(native, "vrhip_trace_surface") and hasattr(native, "vrhip_camera_rays")


def test_c_abi_refuses_without_a_device(native):
    L = native
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.vrhip_trace_surface(None, p, p, 1, p) == -1
    assert b"null ctx" in L.vrhip_last_error()
    assert L.vrhip_trace_surface(None, p, p, 1, ctypes.c_void_p(p.value + 4)) == -1          # a misaligned d_hits
    assert L.vrhip_trace_surface(None, None, None, 0, None) == -1
    assert L.vrhip_camera_rays(None, p, p) == -1
    assert b"null ctx" in L.vrhip_last_error()


def test_record_layout(tmp_path):
    """sizeof(vrhip_surface_hit) == 112, seven 16-byte rows, as a C compiler sees the header."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "vrhip.h"\n'
                   "_Static_assert(sizeof(vrhip_surface_hit) == 112, \"size\");\n"
                   "_Static_assert(offsetof(vrhip_surface_hit, kind) == 4 && offsetof(vrhip_surface_hit, prim) == 8 && "
                   "offsetof(vrhip_surface_hit, type) == 12, \"row 0\");\n"
                   "_Static_assert(offsetof(vrhip_surface_hit, position) == 16 && offsetof(vrhip_surface_hit, bary_u) == 28 && "
                   "offsetof(vrhip_surface_hit, normal) == 32 && offsetof(vrhip_surface_hit, bary_v) == 44 && "
                   "offsetof(vrhip_surface_hit, tangent) == 48 && offsetof(vrhip_surface_hit, pad0) == 60 && "
                   "offsetof(vrhip_surface_hit, color) == 64 && offsetof(vrhip_surface_hit, tex_u) == 76 && "
                   "offsetof(vrhip_surface_hit, specular) == 80 && offsetof(vrhip_surface_hit, tex_v) == 92 && "
                   "offsetof(vrhip_surface_hit, emission) == 96 && offsetof(vrhip_surface_hit, pad1) == 108, \"rows\");\n"
                   "_Static_assert(VRHIP_SURF_NONE == 0 && VRHIP_SURF_CORNELL == 1 && VRHIP_SURF_SMALL == 2 && "
                   "VRHIP_SURF_EXAMPLE == 3 && VRHIP_SURF_MESH == 4, \"kinds\");\n")
    res = subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu11", "-fsyntax-only", "-I", os.path.join(repo, "include"), str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert (sf.BARY_U, sf.BARY_V, sf.PAD0, sf.TEX_U, sf.TEX_V, sf.PAD1) == (7, 11, 15, 19, 23, 27) and sf.WORDS * 4 == 112


def test_wrapper_rejects_wrong_tensors(native):
    import torch
    from vrenderer_pathtracer_amd import VRendererHIP
    r = VRendererHIP(0)
    r._ctx = ctypes.c_void_p(1)          # never reaches the library: the tensors are checked first
    r._lib = native
    try:
        o, d = torch.zeros((8, 3)), torch.ones((8, 3))
        assert hasattr(r, "traceSurface") and hasattr(r, "cameraRays")
        wrong = [dict(origins=o, dirs=d), dict(origins=o.numpy(), dirs=d), dict(origins=None, dirs=d),
                 dict(origins=o.double(), dirs=d), dict(origins=o[:, :2], dirs=d)]
        for kw in wrong:                 # a CPU tensor, not a tensor, missing, wrong dtype, wrong shape
            with pytest.raises(ValueError):
                r.traceSurface(**kw)
    finally:
        r._ctx = ctypes.c_void_p(None)
