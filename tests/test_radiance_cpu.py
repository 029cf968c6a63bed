"""The radiance query without a device (vrhip_trace_radiance).

The yardstick first: tests/radiance_cases.py traces arbitrary rays with the
oracle's own trace through a camera whose up and right are zero.  Here it is
tied to the reference-pinned renders: the camera directions of a scene, traced
that way with the seeds render gives each pixel, must give pyoracle.render's
first frame bit for bit.  Then what the C ABI and the Python wrapper refuse
before any device call."""
import ctypes

import numpy as np
import pytest

import flag_lattice as fl
import pyoracle as po
import radiance_cases as rc


@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_yardstick_equals_the_oracle_render(oracle, native, name):
    sc = fl.scene_of(rc.combo_of(name))
    accum, _, depth, _ = po.render(sc, frames=1, times=[rc.TIME], libm=po.LIBM_PORTABLE)
    paths, ok = rc.reference(name, "A")
    assert ok.all() and np.isfinite(accum).all()
    rec = rc.record_of(paths, 2).reshape(fl.H, fl.W, 4)
    assert (rc.u32(rec[..., :3]) == rc.u32(accum[..., :3])).all(), name
    assert (rc.depth_byte(rec[..., 3]) == depth[..., 0]).all(), name
    assert np.any(rec[..., :3] != 0)
    # the direction the kernels normalise is the camera ray's, in its operation order
    d4 = (ctypes.c_float * 4)()
    o4 = (ctypes.c_float * 4)()
    osc = po.OracleScene(sc, libm=po.LIBM_PORTABLE)
    dirs = rc.camera_dirs(sc).reshape(fl.H, fl.W, 3)
    for x, y in ((0, 0), (31, 0), (7, 19), (31, 31)):
        po.lib().vro_primary_ray(ctypes.byref(osc.s), x, y, o4, d4)
        d = dirs[y, x]
        inv = np.float32(1.0) / np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        assert (rc.u32(d * inv) == rc.u32(np.array(d4[:3], np.float32))).all()


@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_random_rays_stay_finite(oracle, native, name):
    """Set B on the five scenes: within the cap on dropped rays (checked by
    reference()), and not a set of escapes only."""
    paths, ok = rc.reference(name, "B")
    assert ok.sum() >= (1.0 - rc.MAX_DROPPED) * len(ok)
    assert len(np.unique(rc.u32(rc.record_of(paths, 5)[ok, :3]), axis=0)) > len(ok) // 4


@pytest.mark.parametrize("name", rc.SHADING_NAMES)
def test_shading_scenes_under_the_yardstick(oracle, native, name):
    """The shading cases the radiance kernels are run on: within the cap on
    dropped rays, except the NaN case, where NaN records are kept, are a
    minority and never reach w."""
    import shading_cases as sh
    for which in ("A", "B"):
        paths, ok = rc.shading_reference(name, which)
        bad = ~np.isfinite(paths).all((1, 2))
        if name in sh.NAN_CASES:
            assert ok.all() and not np.isnan(paths[..., 3]).any()
            assert not np.isinf(paths).any()                             # NaN, not infinite
            print(f"{name} set {which}: {int(bad.sum())} of {len(bad)} rays hold a NaN")
            assert 1 <= bad.sum() < len(bad) // 10
        else:
            assert bad.sum() <= rc.MAX_DROPPED * len(bad) and (ok == ~bad).all()
        assert np.any(rc.record_of(paths, 2)[ok, :3] != 0)
    got = np.array([[1.0, np.nan, 0.0, 2.0], [1.0, np.nan, 0.0, 2.0]], np.float32)
    want = np.array([[1.0, -np.nan, 0.0, 2.0], [1.0, 0.5, 0.0, 2.0]], np.float32)
    assert rc.same_or_nan_in_both(got, want).tolist() == [True, False]


def test_record_is_the_in_order_fp32_sum():
    r = np.array([[[0.1, 0.2, 0.3, 0.5], [1e-9, 7.0, -0.0, 0.25], [3.0, 1e8, 0.7, 0.0]]], np.float32)
    c = np.float32(1.0) / np.float32(3)
    want = ((np.float32(0) + r[0, 0, :3] * c) + r[0, 1, :3] * c) + r[0, 2, :3] * c
    got = rc.record_of(r, 3)
    assert (rc.u32(got[0, :3]) == rc.u32(want)).all() and got[0, 3] == 0.0
    assert rc.record_of(r, 2)[0, 3] == 0.25


def test_c_abi_refuses_without_a_device(native):
    L = native
    assert hasattr(L, "vrhip_trace_radiance")
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.vrhip_trace_radiance(None, p, p, p, 4, 2, p) == -1
    assert b"null ctx" in L.vrhip_last_error()
    assert L.vrhip_trace_radiance(None, None, None, None, 0, 2, None) == -1


def test_wrapper_rejects_wrong_tensors(native):
    import torch
    from vrenderer_pathtracer_amd import VRendererHIP
    r = VRendererHIP(0)
    r._ctx = ctypes.c_void_p(1)          # never reaches the library: the tensors are checked first
    r._lib = native
    try:
        o, d = torch.zeros((8, 3)), torch.ones((8, 3))
        assert hasattr(r, "traceRadiance")
        wrong = [dict(origins=o, dirs=d), dict(origins=o.numpy(), dirs=d), dict(origins=None, dirs=d),
                 dict(origins=o.double(), dirs=d), dict(origins=o[:, :2], dirs=d)]
        for kw in wrong:                 # a CPU tensor, not a tensor, missing, wrong dtype, wrong shape
            with pytest.raises(ValueError):
                r.traceRadiance(**kw)
    finally:
        r._ctx = ctypes.c_void_p(None)
