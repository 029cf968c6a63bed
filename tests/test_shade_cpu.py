"""Radiance from surface records without a device (vrhip_shade_surface).

The yardstick first.  tests/shade_driver.c restates the oracle's trace with
bounce 0's hit given by the caller; here it is pinned to the trace the
reference-rendered fixtures pin: fed the surface oracle's own records it must
return radiance_cases.oracle_paths' rgb bit for bit, on every scene and ray set
of the surface tests.  Then the yardstick's own conditions on the edited
records the GPU tests use (lightmap records, the mixed set M), and what the C
ABI and the Python wrapper refuse before any device call."""
import ctypes

import numpy as np
import pytest

import radiance_cases as rc
import shade_cases as sc
import surface_cases as sf

NAMES = rc.COMBO_NAMES + rc.SHADING_NAMES


def oracle_paths(name, which, scene):
    """The first CPU_PATHS paths of the oracle's trace along the set's rays."""
    o, d, s = sc.ray_set(which, scene)
    if which in ("A", "B") and name in rc.COMBO_NAMES:
        return rc.reference(name, which)[0][:, :sc.CPU_PATHS]       # the radiance tests' own, shared
    return rc.oracle_paths(scene, o, d, s, sc.CPU_PATHS)


@pytest.mark.parametrize("name", NAMES)
def test_restated_trace_equals_the_oracle_trace(oracle, native, name):
    scene = sf.scene_named(name)
    total = 0
    for which in sf.sets_of(scene):
        want = oracle_paths(name, which, scene)
        rec, d, s, paths, ok = sc.reference(name, which)
        got = paths[:, :sc.CPU_PATHS]
        fin = np.isfinite(want).all((1, 2))
        print(f"{name} set {which}: {len(rec)} records, {int((~fin).sum())} not finite under the oracle's trace")
        assert (got[..., 3] == 0).all()
        if sc.nan_case(name):
            bad = ~sc.same_or_nan_in_both(got[..., :3].reshape(len(got), -1), want[..., :3].reshape(len(got), -1))
            assert not np.isinf(got).any() and 1 <= (~fin).sum() < len(fin) // 2         # NaN, a minority
        else:
            assert (~fin).sum() <= rc.MAX_DROPPED * len(fin), f"{name} set {which}: {(~fin).sum()} records dropped"
            bad = (rc.u32(got[..., :3]) != rc.u32(want[..., :3])).any((1, 2)) & fin
        assert not bad.any(), f"{name} set {which}: {int(bad.sum())} of {len(bad)} records differ (first " \
                              f"{np.flatnonzero(bad)[:5].tolist()})"
        assert np.any(got[fin][..., :3] != 0)
        total += len(rec)
    assert total >= 1024 + 512 + 64


@pytest.mark.parametrize("name", NAMES)
def test_lightmap_records(oracle, native, name):
    """Type 1, colour 1, specular 0, emission 0 on the oracle's hits: finite,
    lit, and independent of the direction bit for bit (in the NaN case: equal
    or NaN in both, and no claim of finiteness)."""
    scene = sf.scene_named(name)
    for which in sf.sets_of(scene):
        rec, d, s, paths, ok = sc.reference(name, which, "lightmap")
        hit = rec[:, sf.KIND] != sf.NONE
        assert (rec[hit, sf.TYPE] == 1).all() and (sf.floats(rec)[hit][:, sf.COLOR] == 1).all()
        assert not rec[hit][:, sf.SPECULAR].any() and not rec[hit][:, sf.EMISSION].any()
        assert (hit == (sf.reference(name, which)[0][:, sf.KIND] != sf.NONE)).all()
        fin = sc.finite(paths)
        if not sc.nan_case(name):       # (there a later bounce meets the NaN normals that are the scene's point)
            assert fin.all(), f"{name} set {which}: {int((~fin).sum())} lightmap records are not finite"
        lit = (paths[..., :3] != 0).any((1, 2))
        print(f"{name} set {which}: {lit[hit].mean():.3f} of the hit records are non-zero")
        if scene.get("cornell"):
            assert lit[hit].mean() >= sc.MIN_LIT
        # the direction plays no part in a hit record: pass the set's directions in reverse order
        rev = np.ascontiguousarray(d[::-1])
        again = sc.driver_paths(scene, rec[hit], rev[hit], s[hit], sc.CPU_PATHS)
        assert sc.same_or_nan_in_both(again.reshape(len(again), -1), paths[hit, :sc.CPU_PATHS].reshape(len(again), -1)).all()


@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_mixed_records(oracle, native, name):
    """Set M on every ray set of the scene: the cap
    on non-finite records holds (reference() checks it), every edit occurs,
    an unedited record keeps its result, and the edits that must change a
    result whatever the material was (emission added, a hit made a miss, and
    the lightmap edit somewhere) do."""
    scene = sf.scene_named(name)
    count = np.zeros(len(sc.EDITS), np.int64)
    moved = np.zeros(len(sc.EDITS), np.int64)
    for which in sf.sets_of(scene):
        rec, d, s, paths, ok = sc.reference(name, which, "mixed")
        base = sc.reference(name, which)
        assert ok.sum() >= (1.0 - sc.MAX_DROPPED) * len(ok)
        hit = base[0][:, sf.KIND] != sf.NONE
        e = np.arange(len(rec)) % len(sc.EDITS)
        same = (rc.u32(paths) == rc.u32(base[3])).all((1, 2))
        assert same[(e == 0) | ~hit].all()
        for k in range(len(sc.EDITS)):
            m = hit & (e == k)
            count[k] += m.sum()
            moved[k] += (~same[m]).sum()
        assert (rec[hit & (e == 6), sf.KIND] == sf.NONE).all()
        assert (rec[~hit] == base[0][~hit]).all()
    print(name, dict(zip(sc.EDITS, zip(count.tolist(), moved.tolist()))))
    assert (count >= 4).all(), dict(zip(sc.EDITS, count.tolist()))
    assert moved[0] == 0 and moved[1] > 0 and moved[5] > 0 and moved[6] > 0


@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_a_miss_made_a_hit_is_nan(oracle, native, name):
    """A miss record's vectors are zero.  As a diffuse hit its zero normal
    gives a NaN direction (normalize of the zero cross product) and a NaN
    mask; in an HDRI scene the next bounce's escape adds mask * environment
    (NaN), in the Cornell box a path that escapes returns 0 whatever it holds."""
    scene = sf.scene_named(name)
    rec, d, s, _, _ = sc.reference(name, "D")
    one, i = sc.miss_made_a_hit(rec)
    paths = sc.driver_paths(scene, one, d[i:i + 1], s[i:i + 1], sc.CPU_PATHS)
    assert not np.isinf(paths).any()
    if scene.get("cornell"):
        assert (np.isnan(paths[..., :3]) | (paths[..., :3] == 0)).all()
    else:
        assert np.isnan(paths[..., :3]).all()


def test_result_is_the_in_order_fp32_sum_with_w_zero():
    r = np.array([[[0.1, 0.2, 0.3, 0.5], [1e-9, 7.0, -0.0, 0.25], [3.0, 1e8, 0.7, 0.0]]], np.float32)
    c = np.float32(1.0) / np.float32(3)
    want = ((np.float32(0) + r[0, 0, :3] * c) + r[0, 1, :3] * c) + r[0, 2, :3] * c
    got = sc.result_of(r, 3)
    assert (rc.u32(got[0, :3]) == rc.u32(want)).all() and rc.u32(got[0, 3]) == 0
    assert rc.u32(sc.result_of(r, 2)[0, 3]) == 0


def test_slice_length_is_whole_waves():
    assert sc.slice_length() >= 64 and sc.slice_length() % 64 == 0


def test_c_abi_refuses_without_a_device(native):
    L = native
    assert hasattr(L, "vrhip_shade_surface")
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.vrhip_shade_surface(None, p, p, p, 1, 2, p) == -1
    assert b"null ctx" in L.vrhip_last_error()
    assert L.vrhip_shade_surface(None, None, None, None, 0, 2, None) == -1


def test_wrapper_rejects_wrong_tensors(native):
    import torch
    from vrenderer_pathtracer_amd import VRendererHIP
    r = VRendererHIP(0)
    r._ctx = ctypes.c_void_p(1)          # never reaches the library: the tensors are checked first
    r._lib = native
    try:
        h, d = torch.zeros((8, 28)), torch.ones((8, 3))
        assert hasattr(r, "shadeSurface") and hasattr(r, "diffuseRecords")
        wrong = [dict(hits=h, dirs=d), dict(hits=h.numpy(), dirs=d), dict(hits=None, dirs=d), dict(hits={}, dirs=d),
                 dict(hits=h.double(), dirs=d), dict(hits=h[:, :27], dirs=d), dict(hits={"record": h}, dirs=d)]
        for kw in wrong:                 # a CPU tensor, not a tensor, missing, an empty dict, wrong dtype, wrong shape
            with pytest.raises(ValueError):
                r.shadeSurface(**kw)
        for kw in (dict(points=d, normals=d), dict(points=None, normals=d), dict(points=d.numpy(), normals=d)):
            with pytest.raises(ValueError):
                r.diffuseRecords(**kw)
    finally:
        r._ctx = ctypes.c_void_p(None)
