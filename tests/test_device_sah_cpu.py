"""The device SAH builder without a device: the decisions it shares with its
kernels (csrc/vr_devsah.hpp), run serially on the host by tests/sah_driver.cpp
with a stable partition, give the node array vrhip_build_flat gives, and the
new entry point's argument checks answer before any device call."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from extreme_cases import EXTREME_KINDS, extreme_mesh
from vrenderer_pathtracer_amd import LIB_PATH, _native, build, build_flat, scenes, validate_flat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def soup(n, seed=5, spread=30.0, sigma=4.0):
    """The generator of test_capi.test_random_soup_bvh_equals_brute_force."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    P = (c + rng.normal(0, sigma, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return dict(positions=P, normals=rng.normal(0, 1, (3 * n, 3)).astype(np.float32),
                tangents=rng.normal(0, 1, (3 * n, 3)).astype(np.float32),
                uvs=rng.uniform(0, 1, (3 * n, 2)).astype(np.float32),
                tris=np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))


def fnv1a_words(a):
    h = 0xcbf29ce484222325
    for w in np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist():
        h = ((h ^ w) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


CASES = ([("soup%d" % n, lambda n=n: soup(n), leaf) for n in (2, 3, 5, 63, 64, 65, 257, 1000) for leaf in (1, 2, 4)]
         + [("knot40x20", lambda: scenes.torus_knot(40, 20), 2), ("knot100x50", lambda: scenes.torus_knot(100, 50), 2),
            ("knot40x20", lambda: scenes.torus_knot(40, 20), 4), ("knot100x50", lambda: scenes.torus_knot(100, 50), 4)]
         # the extremes of float: an overflowed extent and centroid (sah_bin's NaN), the depth cap, denormals
         + [(kind, lambda kind=kind: extreme_mesh(kind), leaf) for kind in EXTREME_KINDS for leaf in (1, 3)])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or build._hipcc()
    exe = str(tmp_path_factory.mktemp("sah") / "sah_driver")
    res = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", build.CSRC,
                          os.path.join(REPO, "tests", "sah_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def test_host_run_of_the_device_decisions_gives_the_host_tree(native, driver, tmp_path, monkeypatch):
    monkeypatch.delenv("VRHIP_SAH_NODE_COST", raising=False)
    monkeypatch.delenv("VRHIP_SBVH_ALPHA", raising=False)
    files, want = [], []
    for i, (name, make, leaf) in enumerate(CASES):
        mesh = make()
        flat = build_flat(mesh, max_leaf_tris=leaf)
        depth, _ = validate_flat(flat)
        want.append((name, leaf, "%d %d %s" % (len(flat["bvh"]), depth, fnv1a_words(flat["bvh"]))))
        path = str(tmp_path / ("m%02d.bin" % i))
        with open(path, "wb") as f:
            f.write(np.array([len(mesh["positions"]), len(mesh["tris"]), leaf], np.uint32).tobytes())
            f.write(np.ascontiguousarray(mesh["positions"], np.float32).tobytes())
            f.write(np.ascontiguousarray(mesh["tris"], np.uint32).tobytes())
        files.append(path)
    env = {k: v for k, v in os.environ.items() if k not in ("VRHIP_SAH_NODE_COST", "VRHIP_SBVH_ALPHA")}
    out = subprocess.run([driver] + files, capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert len(got) == len(want)
    bad = [(name, leaf, g, w) for g, (name, leaf, w) in zip(got, want) if g != w]
    assert not bad, bad


def test_new_symbols_exported_and_declared(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vrhip_\w+)", out))
    declared = set(_native.header_symbols())
    for name in ("vrhip_upload_mesh_device_ex", "vrhip_device_sah_scratch_bytes"):
        assert name in exported and name in declared and name in _native._SIGNATURES, name
    assert native.vrhip_abi_version() == 6             # symbols were added, none changed


@pytest.mark.parametrize("builder", [0, 1])
def test_upload_mesh_device_ex_rejects_bad_arguments_without_a_device(native, builder):
    one = ctypes.c_void_p(16)                          # never dereferenced: the checks come first
    ctx = ctypes.c_void_p(16)
    f = native.vrhip_upload_mesh_device_ex
    assert f(None, one, None, None, None, 3, one, 1, 2, builder) == -1
    assert b"null ctx" in native.vrhip_last_error()
    assert f(ctx, None, None, None, None, 3, one, 1, 2, builder) == -1
    assert f(ctx, one, None, None, None, 3, None, 1, 2, builder) == -1
    assert f(ctx, one, None, None, None, 3, one, 0, 2, builder) == -1
    assert f(ctx, one, None, None, None, 0, one, 1, 2, builder) == -1
    assert f(ctx, one, None, None, None, 3, one, 1 << 24, 2, builder) == -1
    assert f(ctx, one, None, None, None, 3, one, 1, 128, builder) == -1


def test_unknown_builder_is_invalid_without_a_device(native):
    one = ctypes.c_void_p(16)
    assert native.vrhip_upload_mesh_device_ex(ctypes.c_void_p(16), one, None, None, None, 3, one, 1, 2, 7) == -1
    assert b"unknown device builder" in native.vrhip_last_error()
