"""The denoiser without a device (vrhip_denoise, vrhip_denoise_frame).

Pins the yardstick, tests/denoise_driver.c, by what the definition
(include/vrhip.h) makes it do on its own: exact properties, one bounded one,
what each parity case of test_gpu_denoise.py can catch (mutants), the
condition on those cases, and that the filter with the default parameters is
of use on rendered views.  The GPU result is the yardstick's bit for bit, so
the usefulness ratio is a CPU fact.
"""
import ctypes

import numpy as np
import pytest

import denoise_cases as dc
import surface_cases as sf


def u32(a):
    return dc.u32(a)


def flat_grid(w, h, normal=(0.0, 0.0, 1.0), albedo=(0.5, 0.5, 0.5)):
    """Guides of a flat w x h sheet in the plane z = 0."""
    y, x = np.divmod(np.arange(w * h), w)
    pos = np.stack([x, y, np.zeros(w * h)], -1).astype(np.float32)
    return dc.records(pos, np.tile(np.asarray(normal, np.float32), (w * h, 1)), np.tile(np.asarray(albedo, np.float32), (w * h, 1)))


# ---- exact properties ---------------------------------------------------------------------------
@pytest.mark.parametrize("demod", [False, True])
def test_orthogonal_half_planes_do_not_leak(demod):
    """Normals (0,0,1) left and (1,0,0) right: across the edge dn = 0 exactly,
    so wn = 0 and each side's result depends only on its own side."""
    w, h = 24, 10
    rng = np.random.default_rng(1)
    rec = flat_grid(w, h)
    right = (np.arange(w * h) % w) >= w // 2
    rec[right, sf.NORMAL] = u32(np.array((1.0, 0.0, 0.0), np.float32))
    col = rng.uniform(0.1, 1.0, (h, w, 4)).astype(np.float32)
    col[:, w // 2:, :3] += 5.0
    base = dc.filtered(col, rec, w, h, 4, demod, 2)
    other = col.copy()
    other[:, w // 2:, :3] = rng.uniform(20.0, 30.0, (h, w - w // 2, 3)).astype(np.float32)      # another right side
    got = dc.filtered(other, rec, w, h, 4, demod, 2)
    assert (u32(got[:, :w // 2]) == u32(base[:, :w // 2])).all()
    assert base[:, :w // 2, :3].max() <= 1.0 and base[:, w // 2:, :3].min() >= 5.0
    assert (u32(base[..., :3]) != u32(col[..., :3])).any()              # and the filter did something


def test_an_invalid_cell_keeps_its_bits_and_changes_nothing_else():
    w, h = 15, 9
    col, rec = (np.array(a) for a in dc.grid(w, h))
    i = (h // 2) * w + w // 2
    for kind in (0, 5, 0xFFFFFFFF):
        rec[i, sf.KIND] = kind
        a = dc.filtered(col, rec, w, h, 3, True, 1)
        flipped = col.copy()
        flipped.reshape(-1, 4)[i] = (-7.0, 1e30, np.nan, 3.0)
        b = dc.filtered(flipped, rec, w, h, 3, True, 1)
        assert (u32(a).reshape(-1, 4)[i] == u32(col).reshape(-1, 4)[i]).all()
        assert (u32(b).reshape(-1, 4)[i] == u32(flipped).reshape(-1, 4)[i]).all()
        keep = np.arange(w * h) != i
        assert (u32(a).reshape(-1, 4)[keep] == u32(b).reshape(-1, 4)[keep]).all()
    rec[i, sf.KIND] = sf.MESH                                          # the same cell, valid: now it matters
    c = dc.filtered(flipped, rec, w, h, 3, True, 1)
    assert not dc.same_or_nan_in_both(c, a).reshape(-1)[keep].all()


def test_no_passes_is_the_identity_and_w_is_untouched():
    w, h = 13, 7
    col, rec = (np.array(a) for a in dc.grid(w, h))
    col.reshape(-1, 4)[3] = (np.nan, np.inf, -0.0, 1.0)
    for demod in (False, True):
        assert (u32(dc.filtered(col, rec, w, h, 0, demod, 3)) == u32(col)).all()
        for passes in (1, 5):
            out = dc.filtered(col, rec, w, h, passes, demod, 3)
            assert (u32(out[..., 3]) == u32(col[..., 3])).all()


def test_a_single_valid_cell_returns_its_input():
    """Alone, a cell sees one tap, itself: sum = (h wn 1 1) C and ws = h wn with
    a unit normal whose dn is exactly 1, so C' = (k C) (1 / k) with k = 0.140625 a
    power-of-two multiple of 9: exact for colours of few mantissa bits."""
    w, h = 9, 6
    rec = flat_grid(w, h)
    i = 2 * w + 4
    rec[np.arange(w * h) != i, sf.KIND] = sf.NONE
    col = np.random.default_rng(2).integers(0, 64, (h, w, 4)).astype(np.float32) / np.float32(8.0)
    out = dc.filtered(col, rec, w, h, 5, False, 3)
    assert (u32(out) == u32(col)).all()
    one = dc.filtered(col.reshape(-1, 4)[i:i + 1], rec[i:i + 1], 1, 1, 5, False, 3)
    assert (u32(one).reshape(-1) == u32(col).reshape(-1, 4)[i]).all()


# ---- bounded ------------------------------------------------------------------------------------------
def test_a_constant_colour_comes_back_within_64_ulp():
    """Where every C_q equals C_p, wc = 1 and sum.ch = C (w_1 + ... + w_k) but
    for rounding, so C' = sum.ch / ws = C but for rounding.  The bound: 25
    products and sums and one reciprocal per pass are about 30 roundings of at
    most half an ulp each on the way to a channel, with no cancellation (every
    term has one sign).  All 150 roundings of five passes erring the same way
    would be 75 ulp; with signs at random they make sqrt(150) / 2, about 6 ulp,
    and the test prints what it finds (5 and 7 ulp).  64 ulp lies between: ten
    times what independent roundings give, below what only a systematic error
    could reach."""
    w, h = 33, 21
    _, rec = (np.array(a) for a in dc.grid(w, h))
    valid = ((rec[:, sf.KIND] >= 1) & (rec[:, sf.KIND] <= 4)).reshape(h, w)
    col = np.empty((h, w, 4), np.float32)
    col[...] = np.array((0.7310586, 3.1415927, 0.011718750), np.float32).tolist() + [1.0]
    for m in (0, 4):
        out = dc.filtered(col, rec, w, h, 5, False, m)
        ulp = np.abs(u32(out[..., :3]).astype(np.int64) - u32(col[..., :3]).astype(np.int64))
        print(f"m={m}: worst {ulp[valid].max()} ulp")
        assert ulp[valid].max() <= 64
        assert (ulp[~valid] == 0).all()


# ---- the parity cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.cases(), ids=dc.case_id)
def test_parity_cases_exercise_every_weight(case):
    frac = dc.check_condition(case)
    print(dc.case_id(case), frac)


@pytest.mark.parametrize("mutant", sorted(dc.MUTANTS), ids=lambda k: dc.MUTANTS[k].replace(" ", "_"))
def test_each_mutant_changes_every_case_that_covers_it(mutant):
    covered = [c for c in dc.cases() if dc.covers(c, mutant)]
    assert len(covered) >= len(dc.cases()) // 2 - 2
    for c in covered:
        want, _ = dc.reference(*c)
        got, _ = dc.reference(*c, mutant=mutant)
        assert (u32(got) != u32(want)).any(), f"{dc.case_id(c)} does not notice mutant {mutant} ({dc.MUTANTS[mutant]})"


def test_every_special_albedo_and_kind_occurs():
    """The grids hold albedo 0, 0x1p-8f and its next float up, and every kind from invalid to valid."""
    for w, h, _ in dc.SHAPES[3:]:
        _, rec = dc.grid(w, h)
        alb = rec[:, sf.COLOR].view(np.float32)
        thr = np.float32(2.0 ** -8)
        assert (alb == 0).any() and (alb == thr).any() and (alb == np.nextafter(thr, np.float32(1))).any()
        assert set(np.unique(rec[:, sf.KIND]).tolist()) >= {0, 1, 2, 3, 4, 5, 0xFFFFFFFF}


def test_in_place_is_out_of_place():
    w, h = 37, 23
    col, rec = (np.array(a) for a in dc.grid(w, h))
    want = dc.filtered(col, rec, w, h, 3, True, 0)
    c = np.ascontiguousarray(col)
    err = dc.driver().denoise_driver(c.ctypes.data, rec.ctypes.data, w, h, 3, 1, 0, dc.SIGMA_COLOR, dc.SIGMA_POSITION,
                                     c.ctypes.data, None)
    assert err == 0 and (u32(c) == u32(want)).all()


# ---- usefulness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.VIEW_NAMES)
def test_the_defaults_reduce_the_error_of_a_one_frame_view(oracle, name):
    """A 64 x 48 view, 1 frame against the mean of 256: with the default
    parameters RMSE(denoised, converged) < RMSE(noisy, converged).  Measured
    ratios: profiles/denoise/README.md."""
    from vrenderer_pathtracer_amd import VRendererHIP
    d = VRendererHIP.DENOISE_DEFAULTS
    noisy, conv, rec = dc.view(name)
    kinds = rec[:, sf.KIND]
    valid = ((kinds >= 1) & (kinds <= 4)).mean()         # the HDRI view is mostly background, which the filter leaves alone
    assert valid > 0.04
    out = dc.filtered(noisy, rec, dc.VIEW_W, dc.VIEW_H, d["passes"], True, d["normal_power_log2"], d["sigma_color"],
                      d["sigma_position"])
    before, after = dc.rmse(noisy, conv), dc.rmse(out, conv)
    print(f"{name}: {valid:.3f} of the pixels valid; RMSE noisy {before:.5f}, denoised {after:.5f}, ratio {after / before:.4f}")
    assert after < before


# ---- the C ABI -----------------------------------------------------------------------------------------------
def test_symbols_are_exported(native):
    from vrenderer_pathtracer_amd import _native
    assert hasattr(native, "vrhip_denoise") and hasattr(native, "vrhip_denoise_frame")
    assert {"vrhip_denoise", "vrhip_denoise_frame"} <= set(_native.header_symbols())
    assert ctypes.sizeof(_native.DenoiseParams) == 20
    assert native.vrhip_abi_version() == 6


def params(n_passes=5, flags=1, m=1, sigma_color=1.0, sigma_position=1.0):
    from vrenderer_pathtracer_amd import _native
    return _native.DenoiseParams(n_passes, flags, m, sigma_color, sigma_position)


def refused_arguments(buf):
    """Every argument error of vrhip_denoise that is decided before a device
    call, as (what, kwargs) over a valid call; shared with test_gpu_denoise.py,
    which repeats them on a live context and reads the message."""
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = dict(color=p, guides=p, w=4, h=4, prm=params(), out=p)
    inf, nan = float("inf"), float("nan")
    bad = [("null colour", dict(color=None)), ("null colour", dict(guides=None)), ("null colour", dict(out=None)),
           ("d_color is not 16-byte", dict(color=p + 4)), ("d_guides is not 16-byte", dict(guides=p + 8)),
           ("d_out is not 16-byte", dict(out=p + 12)),
           ("grid", dict(w=0)), ("grid", dict(h=0)), ("grid", dict(w=65536, h=32768)), ("grid", dict(w=0xFFFFFFFF, h=0xFFFFFFFF)),
           ("null denoise params", dict(prm=None)), ("n_passes", dict(prm=params(n_passes=9))),
           ("normal_power_log2", dict(prm=params(m=9))), ("unknown denoise flags", dict(prm=params(flags=2))),
           ("unknown denoise flags", dict(prm=params(flags=0x80000001)))]
    for name in ("sigma_color", "sigma_position"):
        bad += [(name, dict(prm=params(**{name: v}))) for v in (0.0, -1.0, inf, -inf, nan)]
    return ok, bad


def call_denoise(L, ctx, a):
    prm = a["prm"]
    return L.vrhip_denoise(ctx, a["color"], a["guides"], a["w"], a["h"], None if prm is None else ctypes.byref(prm), a["out"])


def test_c_abi_refuses_without_a_device(native):
    """No context exists without a device, so every refusal here is also the
    null context's; test_gpu_denoise.py repeats the list on a live context."""
    L = native
    buf = (ctypes.c_float * 64)()
    ok, bad = refused_arguments(buf)
    assert call_denoise(L, None, ok) == -1 and b"null ctx" in L.vrhip_last_error()
    for what, change in bad:
        assert call_denoise(L, None, dict(ok, **change)) == -1, what
    p = ctypes.cast(buf, ctypes.c_void_p)
    prm = params()
    assert L.vrhip_denoise_frame(None, ctypes.byref(prm), p, p) == -1 and b"null ctx" in L.vrhip_last_error()
    assert L.vrhip_denoise_frame(None, None, None, None) == -1
    assert not any(buf)


def test_wrapper_rejects_wrong_tensors(native):
    import torch
    from vrenderer_pathtracer_amd import VRendererHIP
    r = VRendererHIP(0)
    r._ctx = ctypes.c_void_p(1)          # never reaches the library: the tensors are checked first
    r._lib = native
    try:
        c, g = torch.zeros((4, 4, 4)), torch.zeros((16, 28))
        wrong = [dict(color=c, guides=g), dict(color=c.numpy(), guides=g), dict(color=c.view(16, 4), guides=g),
                 dict(color=c[..., :3], guides=g), dict(color=c, guides=None), dict(color=torch.zeros((0, 4, 4)), guides=g)]
        for kw in wrong:                 # CPU tensors, not a tensor, wrong rank, wrong channels, missing, empty
            with pytest.raises(ValueError):
                r.denoise(**kw)
        for kw in (dict(passes=1.5), dict(passes=-1), dict(normal_power_log2=0.5)):
            with pytest.raises(ValueError):
                r._denoise_params(**dict(dict(VRendererHIP.DENOISE_DEFAULTS, demodulate=True), **kw))
        d = r._denoise_params(demodulate=True, **VRendererHIP.DENOISE_DEFAULTS)
        assert (d.n_passes, d.flags, d.normal_power_log2) == (5, 1, VRendererHIP.DENOISE_DEFAULTS["normal_power_log2"])
        import inspect
        for fn in (VRendererHIP.denoise, VRendererHIP.denoiseFrame):
            sig = inspect.signature(fn).parameters
            assert {k: sig[k].default for k in VRendererHIP.DENOISE_DEFAULTS} == VRendererHIP.DENOISE_DEFAULTS
    finally:
        r._ctx = ctypes.c_void_p(None)
