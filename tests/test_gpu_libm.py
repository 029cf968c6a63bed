"""The device functions every pinned result rests on, one at a time on the GPU,
against tests/libm_driver.c (the oracle's own functions in batch loops) on the
input sets of tests/libm_cases.py: sincos_p, acos_p, atan2_p and pow_p in both
constant forms of vr_math.hpp; f2i, d2i and f2u8; sqrt_exact and
inv_sqrt_exact with waves of mixed range; lookup_brdf; and the direction ->
HDRI texel address of bounce_step through traceRadiance in both traversal
modes.  Every comparison is of uint32 bit patterns, NaN equal to NaN, and
asks for zero mismatches; a failure names the function, the operand bits and
both results (or the decoded table indices)."""
import numpy as np
import pytest

import libm_cases as lc
from vrenderer_pathtracer_amd import VRendererHIP, scenes, selftest_brdf, selftest_math

pytestmark = pytest.mark.gpu

IDS = lc.libm_ids()
FORMS = [(0, "per_use"), (lc.HOISTED, "hoisted")]


def report(fn, a, b, got, want, names=("device", "oracle")):
    bad = np.flatnonzero(~lc.same_or_nan_in_both(got, want))
    if len(bad) == 0:
        return
    lines = []
    for i in bad[:4]:
        ops = f"{int(lc.bits(a)[i]):#010x}" + ("" if b is None else f", {int(lc.bits(b)[i]):#010x}")
        lines.append(f"{lc.FN_NAMES[fn & 0xff]}({ops}) [element {i}, lane {i % 64}]: {names[0]} "
                     f"{int(lc.bits(got)[i]):#010x} {names[1]} {int(lc.bits(want)[i]):#010x}")
    pytest.fail(f"{len(bad)} of {a.size} results differ: " + "; ".join(lines))


@pytest.mark.parametrize("i", range(lc.N_LIBM_SETS), ids=IDS)
@pytest.mark.parametrize("form,form_name", FORMS, ids=[f[1] for f in FORMS])
def test_device_libm_on_every_set(native, oracle, i, form, form_name):
    fn, a, b = lc.libm_set(i)
    got = selftest_math(fn | form, a, b)
    report(fn | form, a, b, got, lc.libm_reference(i))


@pytest.mark.parametrize("name,fn,a,b", lc.conversion_sets(), ids=[c[0] for c in lc.conversion_sets()])
def test_device_conversions(native, oracle, name, fn, a, b):
    report(fn, a, b, selftest_math(fn, a, b), lc.oracle_batch(fn, a, b))


@pytest.mark.parametrize("fn", [lc.SQRT, lc.INV_SQRT], ids=["sqrt_exact", "inv_sqrt_exact"])
def test_device_sqrt_in_mixed_waves(native, fn):
    """Waves wholly inside the short sequence's range, the same waves with one
    lane outside it (the whole wave then takes the IEEE expansion), one wave
    wholly outside, and a last wave of 17 lanes: sqrtf and 1 / sqrtf, correctly
    rounded, whichever path the wave's vote takes."""
    a = lc.sqrt_waves(fn)
    report(fn, a, None, selftest_math(fn, a), lc.sqrt_reference(fn, a), names=("device", "numpy"))


def test_device_lookup_brdf(native, oracle):
    want = lc.merl_reference()[0]
    got = selftest_brdf(lc.merl_table(), lc.merl_frames())
    bad = np.flatnonzero((lc.bits(got) != lc.bits(want)).any(-1))
    if len(bad):
        dg, dw = lc.merl_decode(got[bad[:4]]), lc.merl_decode(want[bad[:4]])
        fr = lc.merl_frames()
        pytest.fail(f"{len(bad)} of {len(want)} frames differ; (phi_diff, theta_diff, theta_half) indices device against "
                    f"oracle: " + "; ".join(f"frame {i}: {g.tolist()} against {w.tolist()}, refl/cur/normal/tangent bits "
                                            f"{[hex(v) for v in lc.bits(fr[i, :, :3]).reshape(-1)]}"
                                            for i, g, w in zip(bad[:4], dg, dw)))


# ---- the HDRI address, through the radiance query ------------------------------------------------
def dev(a, dtype=np.float32):
    import torch
    a = np.array(a, dtype=dtype, order="C")              # a copy: the shared ray sets are read-only
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda(0)


def check_hdri(w, h, storage, strict):
    o, d, s, kind, bnd = lc.hdri_rays(w, h)
    want, esc = lc.hdri_reference(w, h)
    r = VRendererHIP(0)
    try:
        scenes.load_into(r, lc.hdri_scene(w, h, storage))
        r.set_strict_traversal(strict)
        got = r.traceRadiance(dev(o), dev(d), dev(s, np.uint32), samples=1).cpu().numpy()
    finally:
        r.cleanUp()
    bad = np.flatnonzero(~lc.same_or_nan_in_both(got, want).all(-1))
    if len(bad):
        def texel(rec):
            return f"texel ({rec[0] / 2:g}, {rec[1] / 2:g}) address {rec[2] / 2:g}"
        pytest.fail(f"{w}x{h} strict={strict}: {len(bad)} of {len(o)} records differ: " + "; ".join(
            f"ray {i} (kind {kind[i]}, boundary {bnd[i]}, escapes at bounce 0: {bool(esc[i])}) direction bits "
            f"{[hex(v) for v in lc.bits(d[i])]}: device {texel(got[i])} against oracle {texel(want[i])}" for i in bad[:4]))


@pytest.mark.parametrize("w,h", lc.HDRI_MAPS, ids=[f"{w}x{h}" for w, h in lc.HDRI_MAPS])
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
def test_hdri_address_float_storage(native, oracle, w, h, strict):
    check_hdri(w, h, np.float32, strict)


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
def test_hdri_address_half_storage(native, oracle, strict):
    check_hdri(*lc.HDRI_HALF_MAP, np.float16, strict)
