"""The device BVH builder's C ABI without a device: the new symbols exist and
are declared for ctypes, and the argument checks that come before any device
call answer VRHIP_ERR_INVALID."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from half_ref import half_reference, half_values
from vrenderer_pathtracer_amd import LIB_PATH, _native, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["vrhip_upload_mesh_device", "vrhip_export_mesh_flat", "vrhip_selftest_half_box"]


def test_new_symbols_exported_and_declared(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vrhip_\w+)", out))
    declared = set(_native.header_symbols())
    for name in NEW:
        assert name in exported, name
        assert name in declared, name
        assert name in _native._SIGNATURES, name
        assert getattr(native, name).argtypes is not None
    assert native.vrhip_abi_version() == 6             # symbols were added, none changed


def test_upload_mesh_device_rejects_null_arguments_without_a_device(native):
    one = ctypes.c_void_p(16)                          # never dereferenced: the checks come first
    ctx = ctypes.c_void_p(16)
    f = native.vrhip_upload_mesh_device
    assert f(None, one, None, None, None, 3, one, 1, 2) == -1
    assert b"null ctx" in native.vrhip_last_error()
    # the remaining checks read nothing of the context either
    assert f(ctx, None, None, None, None, 3, one, 1, 2) == -1
    assert f(ctx, one, None, None, None, 3, None, 1, 2) == -1
    assert f(ctx, one, None, None, None, 3, one, 0, 2) == -1
    assert f(ctx, one, None, None, None, 0, one, 1, 2) == -1
    assert f(ctx, one, None, None, None, 3, one, 1 << 24, 2) == -1
    assert f(ctx, one, None, None, None, 3, one, 1, 128) == -1


def test_export_mesh_flat_rejects_null_context(native):
    n_bvh = ctypes.c_size_t(0)
    n_slots = ctypes.c_size_t(0)
    assert native.vrhip_export_mesh_flat(None, None, ctypes.byref(n_bvh), None, None, None, None,
                                         ctypes.byref(n_slots)) == -1
    assert b"null ctx" in native.vrhip_last_error()


def test_selftest_half_box_rejects_null_arrays(native):
    a = np.zeros(4, np.float32)
    h = np.zeros(4, np.uint16)
    hp = h.ctypes.data_as(_native._u16)
    assert native.vrhip_selftest_half_box(0, None, 4, hp, hp) == -1
    assert native.vrhip_selftest_half_box(0, _native.fptr(a), 4, None, hp) == -1
    assert native.vrhip_selftest_half_box(0, _native.fptr(a), 4, hp, None) == -1


def test_half_directed_on_the_host_matches_numpy_reference(tmp_path):
    """vr::half_directed is plain integer arithmetic shared by host and
    device: compiled here for the host and compared with the reference on the
    issue's values and a million random finite floats of both signs."""
    cxx = shutil.which("g++") or shutil.which("clang++") or build._hipcc()
    exe = str(tmp_path / "half_driver")
    res = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC,
                          os.path.join(REPO, "tests", "half_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    rng = np.random.default_rng(23)
    bits = rng.integers(0, 0x7F800000, 1000000, dtype=np.uint32) | (rng.integers(0, 2, 1000000, dtype=np.uint32) << np.uint32(31))
    x = np.concatenate([half_values(), bits.view(np.float32)])
    out = subprocess.run([exe], input="\n".join("%x" % b for b in x.view(np.uint32)), capture_output=True, text=True,
                         check=True).stdout
    got = np.array(out.split(), np.uint32).reshape(-1, 2).astype(np.uint16)
    assert len(got) == len(x)
    assert np.array_equal(got[:, 0], half_reference(x, False))
    assert np.array_equal(got[:, 1], half_reference(x, True))
