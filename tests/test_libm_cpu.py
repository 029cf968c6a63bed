"""The yardsticks and input sets of tests/libm_cases.py, checked without a GPU.

1. The oracle's portable libm (vro_p_*) against float64 on every set: NaN for
   NaN, infinities and the sign of every result identical, finite results
   within the bounds tests/test_oracle.py uses (0.501 ulp for sin, cos and pow,
   1.0 for acos).  atan2: the largest error measured on these sets against
   float64 is 1.4353 ulp (set atan2-uniform; 1.3898 on atan2-lattice, 1.3773
   on atan2-expdiff, 1.3807 on atan2-denormal, 0.8296 on atan2-x_one), so the
   bound asserted is the next quarter-ulp step above it, 1.5.  The bit compare
   of test_gpu_libm.py is the exact pin; this bound only has to catch a branch
   that is wrong by several ulp.  An overflowed result is measured as 2^128.
   These checks found two deviations, mended in oracle/vro_math.c and
   vr_math.hpp together: sin(-0) was +0, and pow(-inf, y) was NaN for a
   non-integer y (it is +inf for y > 0 and +0 for y < 0).
2. vr_math.hpp compiled for the host in its VR_DK_HOISTED form
   (tests/libm_host.cpp behind tests/stubs/hip/hip_runtime.h) equals the
   oracle on every set, bit for bit.
3. Every mutant of tests/libm_driver.c changes an output of the sets that
   claim to cover it; mutant 6 is caught by every libm set of 2^20 or more
   elements.
4. Coverage, from the oracle alone: the MERL frames reach every value of each
   of the three indices and all three arms of lookup_brdf; at least 90 % of the
   HDRI rays escape at bounce 0, they read every texel of every map of at most
   2,048 texels, and the ring at each column and row boundary reads the texels
   on both sides of it.
"""
import numpy as np
import pytest

import libm_cases as lc

BOUNDS = {lc.SIN: 0.501, lc.COS: 0.501, lc.POW: 0.501, lc.ACOS: 1.0, lc.ATAN2: 1.5}
IDS = lc.libm_ids()
ALL = range(lc.N_LIBM_SETS)


def describe(fn, a, b, i, **results):
    s = f"{lc.FN_NAMES[fn & 0xff]}({int(lc.bits(a)[i]):#010x}"
    if b is not None:
        s += f", {int(lc.bits(b)[i]):#010x}"
    return s + ") " + " ".join(f"{k} {int(lc.bits(v)[i]):#010x}" for k, v in results.items())


def max_error(fn, a, b, got):
    """The checks of part 1 on one set; returns the largest error in ulp."""
    exact = lc.exact64(fn, a, b)
    nan = np.isnan(exact)
    bad = np.flatnonzero(np.isnan(got) != nan)
    assert len(bad) == 0, f"NaN in one only: {describe(fn, a, b, bad[0], got=got)}"
    ok = ~nan
    bad = np.flatnonzero(ok & (np.signbit(got) != np.signbit(exact)))
    assert len(bad) == 0, f"sign differs: {describe(fn, a, b, bad[0], got=got)} exact {exact[bad[0]]!r}"
    bad = np.flatnonzero(ok & np.isinf(exact) & (got.astype(np.float64) != exact))
    assert len(bad) == 0, f"infinity expected: {describe(fn, a, b, bad[0], got=got)}"
    bad = np.flatnonzero(ok & (exact == 0) & (got != 0))
    assert len(bad) == 0, f"zero expected: {describe(fn, a, b, bad[0], got=got)}"
    # overflow: an infinite result stands for 2^128, the value the float format rounds to infinity from, and so
    # does every exact value beyond it; the spacing there is that of the last binade
    g = got.astype(np.float64)
    g = np.where(np.isinf(g), np.copysign(2.0 ** 128, g), g)
    with np.errstate(all="ignore"):
        x = np.clip(exact, -2.0 ** 128, 2.0 ** 128)
        mag = np.abs(x)
        e = np.floor(np.log2(np.where(mag > 0, mag, 1.0)))
        err = np.abs(g - x) / np.exp2(np.clip(e, -126, 127) - 23)
    err = np.where(ok & np.isfinite(exact), err, 0.0)
    worst = int(np.argmax(err))
    assert err[worst] <= BOUNDS[fn], f"{err[worst]:.4f} ulp: {describe(fn, a, b, worst, got=got)} exact {exact[worst]!r}"
    return float(err[worst])


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_oracle_libm_against_float64(oracle, i):
    fn, a, b = lc.libm_set(i)
    worst = max_error(fn, a, b, lc.libm_reference(i))
    print(f"{IDS[i]}: {a.size} elements, max error {worst:.4f} ulp (bound {BOUNDS[fn]})")


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_host_compiled_header_equals_oracle(oracle, i):
    fn, a, b = lc.libm_set(i)
    got, want = lc.host_batch(fn, a, b), lc.libm_reference(i)
    bad = np.flatnonzero(~lc.same_or_nan_in_both(got, want))
    assert len(bad) == 0, f"{len(bad)} of {a.size} differ: {describe(fn, a, b, bad[0], header=got, oracle=want)}"


@pytest.mark.parametrize("name,fn,a,b", lc.conversion_sets(), ids=[c[0] for c in lc.conversion_sets()])
def test_host_compiled_conversions(oracle, name, fn, a, b):
    """f2i, d2i and f2u8: header == oracle, and both equal a saturating
    truncation written with numpy."""
    got, want = lc.host_batch(fn, a, b), lc.oracle_batch(fn, a, b)
    bad = np.flatnonzero(lc.bits(got) != lc.bits(want))
    assert len(bad) == 0, describe(fn, a, b, bad[0], header=got, oracle=want)
    with np.errstate(all="ignore"):
        x = a.astype(np.float64) if b is None else a.astype(np.float64) * b.astype(np.float64)
        t = np.trunc(np.nan_to_num(x, nan=0.0, posinf=1e300, neginf=-1e300))
    if fn == lc.F2U8:
        assert np.array_equal(want, np.clip(t, 0, 255).astype(np.float32))
    else:
        assert np.array_equal(want.view(np.int32), np.clip(t, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64).astype(np.int32))


@pytest.mark.parametrize("fn", [lc.SQRT, lc.INV_SQRT], ids=["sqrt_exact", "inv_sqrt_exact"])
def test_host_compiled_sqrt(fn):
    """The waves hold what they claim, and the header's short sequences (one
    lane per wave on the host) equal the correctly rounded reference."""
    a = lc.sqrt_waves(fn)
    lo = 2.0 ** -96 if fn == lc.SQRT else 2.0 ** -64
    with np.errstate(invalid="ignore"):
        inside = (a >= lo) & (a <= np.finfo(np.float32).max)
    full, tail = inside[:-17].reshape(-1, 64), inside[-17:]
    assert a.size % 64 == 17 and tail.sum() == 16
    per_wave = full.sum(-1)
    assert (per_wave == 64).sum() >= 64 and (per_wave == 63).sum() == 4 * len(lc.OUTSIDE) and (per_wave == 0).sum() == 1
    mixed = np.flatnonzero(per_wave == 63)
    assert {int(np.flatnonzero(~full[w])[0]) for w in mixed} >= {0, 31, 63}
    got, want = lc.host_batch(fn, a), lc.sqrt_reference(fn, a)
    bad = np.flatnonzero(~lc.same_or_nan_in_both(got, want))
    assert len(bad) == 0, describe(fn, a, None, bad[0], header=got, numpy=want)


# the functions whose sets must notice each mutant (every other function's sets are not asked; cos and acos
# of a denormal are 1 and pi/2 whether or not the operand is flushed, and no cos or acos is a denormal)
MUTANT_COVER = {1: ("sin", "atan2", "pow"), 2: ("sin", "atan2", "pow"), 3: ("atan2",), 4: ("pow",), 5: ("acos",),
                6: ("sin", "cos", "acos", "atan2", "pow")}


def _changed(fn, a, b, mutant, want=None):
    want = lc.oracle_batch(fn, a, b) if want is None else want
    return int((~lc.same_or_nan_in_both(lc.oracle_batch(fn, a, b, mutant), want)).sum())


@pytest.mark.parametrize("mutant", lc.LIBM_MUTANTS)
def test_libm_sets_catch_mutant(oracle, mutant):
    total = {}
    for i in ALL:
        name = lc.FN_NAMES[lc.LIBM_SPECS[i][0]]
        if name not in MUTANT_COVER[mutant]:
            continue
        fn, a, b = lc.libm_set(i)
        c = _changed(fn, a, b, mutant, lc.libm_reference(i))
        total[name] = total.get(name, 0) + c
        if mutant == 6 and a.size >= 1 << 20:
            assert c > 0, f"{IDS[i]} ({a.size} elements) does not notice mutant 6"
    old = {lc.FN_NAMES[fn]: _changed(fn, *lc.old_draws(fn), mutant) for fn in (lc.SIN, lc.COS, lc.ACOS, lc.ATAN2, lc.POW)
           if lc.FN_NAMES[fn] in MUTANT_COVER[mutant]}
    print(f"mutant {mutant} ({lc.MUTANTS[mutant]}): new sets {total}, the draws of test_device_libm_bitexact {old}")
    for f in MUTANT_COVER[mutant]:
        assert total[f] > 0, f"mutant {mutant} ({lc.MUTANTS[mutant]}) changes no output of the {f} sets"


def test_merl_frames_cover_the_index_maps(oracle):
    out, index, arm, differ = lc.merl_reference()
    assert differ == 0, f"the driver's restated brdf_index differs from the oracle's on {differ} frames"
    assert index.min() >= 0 and index.max() < lc.N_IND
    phi, td, th = index % lc.N_PHI, (index // lc.N_PHI) % lc.N_TD, index // (lc.N_PHI * lc.N_TD)
    for name, got, n in (("phi_diff", phi, lc.N_PHI), ("theta_diff", td, lc.N_TD), ("theta_half", th, lc.N_TH)):
        missing = np.setdiff1d(np.arange(n), got)
        assert len(missing) == 0, f"{name} index values never reached: {missing.tolist()}"
    counts = np.bincount(arm, minlength=3)
    assert (counts > 0).all(), f"frames per arm (theta_diff < 1e-3, general, theta_H <= 1e-3): {counts.tolist()}"
    dec = lc.merl_decode(out)
    nan = np.isnan(out[:, :3]).any(-1)
    assert not nan.any()
    assert np.array_equal(dec, np.stack([phi, td, th], -1)), "the table does not decode to the index"
    print(f"{len(index)} frames, per arm {counts.tolist()}, {len(np.unique(index))} distinct entries")


@pytest.mark.parametrize("mutant", lc.MERL_MUTANTS)
def test_merl_frames_catch_mutant(oracle, mutant):
    want = lc.merl_reference()[0]
    got = lc.merl_reference(mutant)[0]
    n = int((lc.bits(got) != lc.bits(want)).any(-1).sum())
    print(f"mutant {mutant} ({lc.MUTANTS[mutant]}): {n} of {len(want)} frames change")
    assert n > 0


def hdri_texels(w, h, rec):
    """(x, y, address) an escaping ray's record names; asserts that the three agree."""
    x, y, a = (rec[:, c].astype(np.float64) / 2 for c in range(3))
    assert np.array_equal(a, x + y * w) and (rec[:, 3] == 1).all()
    return x.astype(np.int64), y.astype(np.int64), a.astype(np.int64)


@pytest.mark.parametrize("w,h", lc.HDRI_MAPS, ids=[f"{w}x{h}" for w, h in lc.HDRI_MAPS])
def test_hdri_rays_cover_the_map(oracle, w, h):
    """From the oracle alone: at least 90 % of the rays escape at bounce 0;
    they reach every texel (maps of at most 2,048 texels), and the ring at
    every column and row boundary reaches the texels on both sides of it."""
    o, d, s, kind, bnd = lc.hdri_rays(w, h)
    rec, esc = lc.hdri_reference(w, h)
    assert esc.mean() >= lc.HDRI_MIN_ESCAPED, esc.mean()
    x, y, a = hdri_texels(w, h, rec[esc])
    assert a.min() >= 0 and a.max() < w * h
    if w * h <= lc.HDRI_COVERED_TEXELS:
        missing = np.setdiff1d(np.arange(w * h), a)
        assert len(missing) == 0, f"texels never read: {missing[:10].tolist()}"
    k_esc, b_esc = kind[esc], bnd[esc]
    for k in range(w + 1):                                    # boundary k lies between columns k - 1 and k, cyclically
        got = set(x[(k_esc == lc.COLUMN_RING) & (b_esc == k)].tolist())
        assert {(k - 1) % w, k % w} <= got, f"column boundary {k}: columns {sorted(got)}"
    for k in range(1, h):
        got = set(y[(k_esc == lc.ROW_RING) & (b_esc == k)].tolist())
        assert {k - 1, k} <= got, f"row boundary {k}: rows {sorted(got)}"
    print(f"{w}x{h}: {len(d)} rays, {esc.mean():.4f} escape at bounce 0, {len(np.unique(a))} texels read")


def test_selftest_entries_check_their_arguments(native):
    """Before any device call: null arrays, a function the hoisted form does
    not hold and a table of the wrong size are VRHIP_ERR_INVALID; n == 0
    launches nothing and is VRHIP_OK."""
    from vrenderer_pathtracer_amd import _native
    a = np.ones(4, np.float32)
    p = _native.fptr(a)
    assert native.vrhip_selftest_math(0, 0, None, p, p, 4) == -1
    assert native.vrhip_selftest_math(0, 0, p, p, None, 4) == -1
    assert native.vrhip_selftest_math(0, 5 | lc.HOISTED, p, p, p, 4) == -1
    assert b"hoisted" in native.vrhip_last_error()
    for fn in (0, 4, 10, 4 | lc.HOISTED):
        assert native.vrhip_selftest_math(0, fn, p, p, p, 0) == 0
    t = lc.merl_table()
    f = np.zeros(16, np.float32)
    o = np.zeros(4, np.float32)
    assert native.vrhip_selftest_brdf(0, _native.fptr(t), t.size - 3, _native.fptr(f), 1, _native.fptr(o)) == -1
    assert native.vrhip_selftest_brdf(0, _native.fptr(t), t.size, None, 1, _native.fptr(o)) == -1
    assert native.vrhip_selftest_brdf(0, _native.fptr(t), t.size, _native.fptr(f), 0, _native.fptr(o)) == 0
