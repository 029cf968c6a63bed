"""GPU tests of the denoiser (vrhip_denoise, vrhip_denoise_frame).

The yardstick is tests/denoise_driver.c (denoise_cases.py), which
test_denoise_cpu.py pins on its own; every comparison here is as uint32.
"""
import ctypes

import numpy as np
import pytest

import denoise_cases as dc
import surface_cases as sf
from device_mesh_cases import fresh
from test_denoise_cpu import call_denoise, params, refused_arguments
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, scenes

pytestmark = pytest.mark.gpu

KW = dict(sigma_color=dc.SIGMA_COLOR, sigma_position=dc.SIGMA_POSITION)


def u32(a):
    return dc.u32(a)


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda(0)      # a copy: the shared inputs are read-only


def guides_dev(rec):
    """The (n, 28) records on the device as the float32 tensor the wrapper takes (a bit copy)."""
    return dev(np.ascontiguousarray(rec, np.uint32).view(np.float32))


@pytest.fixture(scope="module")
def r(native):
    q = VRendererHIP(0)
    q.init(32, 32)                       # vrhip_denoise needs a context and nothing in it: no scene, no mesh
    yield q
    q.cleanUp()


def run(q, color, rec, passes, demod, m, in_place=False, **kw):
    h, w = color.shape[:2]
    c, g = dev(color), guides_dev(rec)
    out = q.denoise(c, g, passes=passes, normal_power_log2=m, demodulate=demod, out=c if in_place else None, **dict(KW, **kw))
    assert tuple(out.shape) == (h, w, 4) and (out.data_ptr() == c.data_ptr()) == in_place
    if not in_place:
        assert (u32(c.cpu().numpy()) == u32(color)).all()                   # the input is only read
    assert (g.cpu().numpy().view(np.uint32) == np.asarray(rec, np.uint32)).all()
    return out.cpu().numpy()


def same(got, want, what):
    bad = np.argwhere((u32(got) != u32(want)).any(-1))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} cells differ, first (y, x) {bad[:5].tolist()}: "
                           f"{got[tuple(bad[0])].tolist()} against {want[tuple(bad[0])].tolist()}")


# ---- 1. parity with the driver on grid shapes ------------------------------------------------------
@pytest.mark.parametrize("case", dc.cases(), ids=dc.case_id)
def test_parity_on_grid_shapes(r, case):
    w, h, passes, demod, m = case
    color, rec = dc.grid(w, h)
    want, _ = dc.reference(*case)
    for in_place in (False, True):
        same(run(r, color, rec, passes, demod, m, in_place), want, f"{dc.case_id(case)} in_place={in_place}")


def test_dict_guides_and_a_second_grid_on_the_same_scratch(r):
    """A larger grid grows the kept scratch, a smaller one reuses it."""
    for w, h in ((70, 45), (16, 16), (129, 65), (37, 23)):
        color, rec = dc.grid(w, h)
        want, _ = dc.reference(w, h, 3, True, 0)
        got = r.denoise(dev(color), {"record": guides_dev(rec)}, passes=3, normal_power_log2=0, **KW).cpu().numpy()
        same(got, want, f"{w}x{h}")


# ---- 2. guide extremes --------------------------------------------------------------------------------
def check(r, color, rec, passes=4, demod=True, m=1, what=""):
    h, w = color.shape[:2]
    want = dc.filtered(color, rec, w, h, passes, demod, m)
    got = run(r, color, rec, passes, demod, m)
    same(got, want, what)
    return got


def test_all_cells_invalid(r):
    color, rec = (np.array(a) for a in dc.grid(37, 23))
    rec[:, sf.KIND] = np.array([0, 5, 77, 0xFFFFFFFF], np.uint32)[np.arange(len(rec)) % 4]
    got = check(r, color, rec, what="all invalid")
    assert (u32(got) == u32(color)).all()


def test_checkerboard_validity(r):
    color, rec = (np.array(a) for a in dc.grid(37, 23))
    y, x = np.divmod(np.arange(len(rec)), 37)
    rec[:, sf.KIND] = np.where((x + y) % 2 == 0, sf.MESH, sf.NONE)
    got = check(r, color, rec, passes=5, what="checkerboard")
    off = ((x + y) % 2 == 1).reshape(23, 37)
    assert (u32(got)[off] == u32(color)[off]).all() and (u32(got)[~off] != u32(color)[~off]).any()


def test_zero_normals_keep_the_colour(r):
    """dn = 0 on every tap, the centre included: ws = 0 and the cell keeps its colour."""
    color, rec = (np.array(a) for a in dc.grid(37, 23))
    rec[:, sf.NORMAL] = 0
    got = check(r, color, rec, demod=False, what="zero normals")
    assert (u32(got) == u32(color)).all()
    rec[::3, sf.NORMAL] = u32(np.array((0.0, 0.0, 1.0), np.float32))       # a third of the cells have one again
    check(r, color, rec, demod=True, what="a third with normals")


def test_albedo_at_the_threshold_and_next_to_it(r):
    w, h = 21, 18
    color, rec = (np.array(a) for a in dc.grid(w, h))
    thr = np.float32(2.0 ** -8)
    up = np.nextafter(thr, np.float32(1.0))
    for alb in ((thr, thr, thr), (up, up, up), (thr, up, 0.0)):
        rec[:, sf.COLOR] = u32(np.asarray(alb, np.float32))
        got = check(r, color, rec, what=f"albedo {alb}")
        plain = run(r, color, rec, 4, False, 1)
        if all(a <= thr for a in alb):                  # at the threshold nothing is demodulated: the plain filter
            assert (u32(got) == u32(plain)).all()
        else:                                           # one float above it the channel is
            assert (u32(got) != u32(plain)).any()


def test_a_nan_and_an_inf_colour_cell(r):
    """Equal bits or NaN in both, and the poisoned region is exactly the driver's."""
    w, h = 40, 30
    color, rec = (np.array(a) for a in dc.grid(w, h))
    rec[:, sf.KIND] = sf.MESH
    clean = dc.filtered(color, rec, w, h, 3, True, 0)
    color[7, 9, 1] = np.nan
    color[20, 28, 0] = np.inf
    want = dc.filtered(color, rec, w, h, 3, True, 0)
    got = run(r, color, rec, 3, True, 0)
    assert dc.same_or_nan_in_both(got, want).all()
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all()
    poisoned = ~np.isfinite(want).all(-1)
    assert 2 <= poisoned.sum() < w * h // 2
    untouched = (u32(want) == u32(clean)).all(-1)
    assert (u32(got)[untouched] == u32(clean)[untouched]).all() and untouched.sum() > 0


def test_no_passes_copies_bit_for_bit(r):
    color, rec = (np.array(a) for a in dc.grid(37, 23))
    color[3, 5] = (np.nan, np.inf, -0.0, 1e-42)
    for in_place in (False, True):
        assert (u32(run(r, color, rec, 0, True, 3, in_place)) == u32(color)).all()


# ---- 3. the frame call against the product itself ----------------------------------------------------------
FRAME_W, FRAME_H, FRAMES, TIMES = 96, 64, 3, [21, 22, 23]


def frame_renderer(name, strict):
    sc = dict(sf.scene_named(name), width=FRAME_W, height=FRAME_H)
    q = VRendererHIP(0)
    scenes.load_into(q, sc)
    q.set_strict_traversal(strict)
    return q


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("name", dc.VIEW_NAMES)
def test_frame_call(oracle, name, strict):
    coef = np.float32(1.0) / np.float32(FRAMES)
    state = {}
    for query in (False, True):
        q = frame_renderer(name, strict)
        try:
            q.render(frames=FRAMES, times=TIMES)
            if query:
                before = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount())
                accum = before[0]
                color = accum.copy()
                color[..., :3] = accum[..., :3] * coef          # the tonemap's own operation: rgb scaled, w as accumulated
                f0, b0 = q.denoiseFrame(passes=0, rgba8=True)
                assert (u32(f0.cpu().numpy()) == u32(color)).all()
                assert b0.cpu().numpy().tobytes() == before[1].tobytes()
                o, d = q.cameraRays()
                guides = q.traceSurface(o, d)
                rec = guides["record"].cpu().numpy().view(np.uint32)
                assert ((rec[:, sf.KIND] >= 1) & (rec[:, sf.KIND] <= 4)).any()
                for passes, demod in ((1, True), (5, True), (5, False)):
                    got, img = q.denoiseFrame(passes=passes, demodulate=demod, rgba8=True)
                    got = got.cpu().numpy()
                    by_hand = q.denoise(dev(color), guides, passes=passes, demodulate=demod).cpu().numpy()
                    assert (u32(got) == u32(by_hand)).all()
                    dflt = VRendererHIP.DENOISE_DEFAULTS
                    want = dc.filtered(color, rec, FRAME_W, FRAME_H, passes, demod, dflt["normal_power_log2"],
                                       dflt["sigma_color"], dflt["sigma_position"])
                    same(got, want, f"{name} passes={passes} demod={demod}")
                    assert (u32(got[..., :3]) != u32(color[..., :3])).any()
                    # the image is the render's tonemap of the filtered colour: where the colour is the render's, so is the byte
                    img = img.cpu().numpy()
                    assert (img[..., 3] == 0xff).all()
                    kept = (u32(got) == u32(color)).all(-1)
                    assert (img[kept] == before[1][kept]).all()
                only = q.denoiseFrame(passes=0)
                assert (u32(only.cpu().numpy()) == u32(color)).all()
                after = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount())
                for x, y in zip(before[:3], after[:3]):
                    assert x.tobytes() == y.tobytes()
                assert before[3] == after[3] == FRAMES
            q.render(frames=1, times=[24])
            state[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount())
        finally:
            q.cleanUp()
    for x, y in zip(state[False][:3], state[True][:3]):
        assert x.tobytes() == y.tobytes()
    assert state[False][3] == state[True][3] == FRAMES + 1


def test_frame_bytes_only(oracle):
    """The RGBA8 output alone (d_out_f32 NULL) is the byte image of the pair."""
    import torch
    q = frame_renderer(dc.VIEW_NAMES[0], False)
    try:
        q.render(frames=FRAMES, times=TIMES)
        _, img = q.denoiseFrame(rgba8=True)
        alone = torch.zeros((FRAME_H, FRAME_W, 4), dtype=torch.uint8, device="cuda:0")
        prm = q._denoise_params(demodulate=True, **VRendererHIP.DENOISE_DEFAULTS)
        torch.cuda.synchronize()
        assert q._lib.vrhip_denoise_frame(q._ctx, ctypes.byref(prm), None, ctypes.c_void_p(alone.data_ptr())) == 0
        assert alone.cpu().numpy().tobytes() == img.cpu().numpy().tobytes()
    finally:
        q.cleanUp()


# ---- 4. refusals --------------------------------------------------------------------------------------------
def test_refusals_of_denoise(r):
    import torch
    L = r._lib
    buf = torch.zeros(28 * 16 + 16, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ok, bad = refused_arguments(ctypes.c_void_p(buf.data_ptr()))
    for what, change in bad:
        assert call_denoise(L, r._ctx, dict(ok, **change)) == -1, what
        assert what.encode() in L.vrhip_last_error(), (what, L.vrhip_last_error())
    assert not buf.cpu().numpy().any()                   # nothing was written by any of them
    assert call_denoise(L, r._ctx, ok) == 0              # and the call they were made from is a valid one
    q = VRendererHIP([0])                                # a multi-device context of one device
    q.init(32, 32)
    try:
        assert call_denoise(L, q._ctx, ok) == -1 and b"multi-device" in L.vrhip_last_error()
        with pytest.raises(VRHIPError) as e:
            q.denoiseFrame()
        assert e.value.code == -1 and "multi-device" in str(e.value)
    finally:
        q.cleanUp()


def test_refusals_of_the_frame_call():
    import torch
    q = fresh()                                          # HDRI mode, no environment, nothing rendered
    try:
        out = torch.zeros((q.height, q.width, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        L, p = q._lib, ctypes.c_void_p(out.data_ptr())
        prm = params()
        with pytest.raises(VRHIPError) as e:
            q.denoiseFrame()
        assert e.value.code == -1 and "no frame rendered" in str(e.value)          # before the first render
        assert L.vrhip_denoise_frame(q._ctx, ctypes.byref(prm), None, None) == -1 and b"no output" in L.vrhip_last_error()
        assert L.vrhip_denoise_frame(q._ctx, ctypes.byref(prm), ctypes.c_void_p(p.value + 4), None) == -1
        assert b"16-byte" in L.vrhip_last_error()
        assert L.vrhip_denoise_frame(q._ctx, ctypes.byref(prm), None, ctypes.c_void_p(p.value + 2)) == -1
        assert b"4-byte" in L.vrhip_last_error()
        assert L.vrhip_denoise_frame(q._ctx, None, p, None) == -1 and b"null denoise params" in L.vrhip_last_error()
        for bad in (params(n_passes=9), params(m=9), params(flags=4), params(sigma_color=0.0), params(sigma_position=float("nan"))):
            assert L.vrhip_denoise_frame(q._ctx, ctypes.byref(bad), p, None) == -1
        q.useCornellBox(True)
        q.render(frames=1, times=[5])
        q.useCornellBox(False)                           # frames rendered, HDRI mode, no map
        with pytest.raises(VRHIPError) as e:
            q.denoiseFrame()
        assert e.value.code == -3
        q.useCornellBox(True)
        q.set_tiling(1, 2)                               # a tiled rank
        with pytest.raises(VRHIPError) as e:
            q.denoiseFrame()
        assert e.value.code == -1 and "tiled rank" in str(e.value)
        q.set_tiling(0, 1)
        assert not out.cpu().numpy().any()               # nothing was written by any of them
        assert np.isfinite(q.denoiseFrame().cpu().numpy()).all()
        q.clearBuffer()
        with pytest.raises(VRHIPError) as e:
            q.denoiseFrame()
        assert e.value.code == -1 and "no frame rendered" in str(e.value)          # and after a clear
    finally:
        q.cleanUp()


# ---- 5. session closing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["denoise", "denoiseFrame"])
def test_between_unsynchronised_renders_of_a_session(oracle, call):
    sc = sf.scene_named("cornell+mesh")
    color, rec = dc.grid(37, 23)
    want, _ = dc.reference(37, 23, 3, True, 0)
    images = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, sc)
        q.set_service(1)
        q.render(frames=2, times=[11, 12], sync=False)
        if query:
            s0 = q.service_info()["sessions"]
            if call == "denoise":
                same(q.denoise(dev(color), guides_dev(rec), passes=3, normal_power_log2=0, **KW).cpu().numpy(), want, "inside a session")
            else:
                got = q.denoiseFrame(passes=0).cpu().numpy()         # the session's two frames, complete
                mid = q.read_accum()
                assert (u32(got[..., :3]) == u32(mid[..., :3] * (np.float32(1.0) / np.float32(2.0)))).all()
                assert np.isfinite(q.denoiseFrame().cpu().numpy()).all()
        q.render(frames=2, times=[13, 14], sync=False)
        q.sync()
        if query:
            assert q.service_info()["sessions"] > s0 >= 1        # the call closed the first session
        assert q.getFrameCount() == 4
        images[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8())
        q.cleanUp()
    for a, b in zip(images[False], images[True]):
        assert a.tobytes() == b.tobytes()
    assert np.any(images[True][0][..., :3] != 0)
