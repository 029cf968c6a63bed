"""The host ray query (vr_raycast.cpp, behind vrhip_flat_trace_rays) under CPU
AddressSanitizer + UndefinedBehaviorSanitizer: tests/raycast_driver.cpp, a
stand-alone program, is compiled with g++
-fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all
together with vr_raycast.cpp and the tree validator it calls (vr_bvh.cpp; no
HIP) and walks a built tree, a chain tree 40 levels deep (the walk's stack),
trees over meshes at the extremes of float with rays of every magnitude a
float holds, and malformed trees -- child offsets out of range, a
missing terminator, cycles -- which must come back as VRHIP_ERR_BVH.  No
sanitizer report, no crash."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "vrenderer_pathtracer_amd", "csrc")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("san") / "raycast_driver")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-fsanitize=address,undefined,float-cast-overflow",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(REPO, "tests", "raycast_driver.cpp"),
           os.path.join(CSRC, "vr_raycast.cpp"), os.path.join(CSRC, "vr_bvh.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return out


def test_host_ray_query_under_sanitizers(driver):
    res = subprocess.run([driver], capture_output=True, text=True, env=SAN_ENV, timeout=600)
    report = res.stderr
    assert "AddressSanitizer" not in report and "runtime error" not in report and "LeakSanitizer" not in report, \
        report[-4000:]
    assert res.returncode == 0, (res.returncode, report[-4000:])
    mode, ok, rej = res.stdout.strip().splitlines()[-1].split()
    assert mode == "raycast"
    assert int(ok.split("=")[1]) == 8 and int(rej.split("=")[1]) == 8, res.stdout
