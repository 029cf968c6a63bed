"""WHEN the library's work runs relative to everyone else's: rendering and
queries on a stream the caller owns or holds, and device inputs that are
still being produced when the call is made.

A. a context whose stream is the caller's (vrhip_set_stream) or was handed out
   (vrhip_get_stream) renders what an untouched context and the oracle render,
   through every launch kind;
B. work the caller queues on the context stream behind vrhip_render, with no
   library call in between, sees the renders (the promise above vrhip_render in
   include/vrhip.h);
C. the C ABI's device inputs may be pending on the context stream;
D. VRendererHIP's tensor-taking methods wait for torch's current stream before
   a query that runs on the renderer's own stream.

Every case that depends on ordering puts a bounded device-side delay (about 30
ms, stream_cases.delay) ahead of the work that must be waited for, measures it,
and asserts that it lasted 20 ms: without it the case would pass by luck.
Nothing sleeps on the host."""
import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

IMAGES = ("accum", "rgba8", "depth8")
MESH_SEQUENCES_A = ("multi3", "sync1x6", "lanes1x6", "service213", "graph1x6")
CASES_A = ([("C2", s) for s in MESH_SEQUENCES_A + ("rank1of3",)] + [("C3", s) for s in MESH_SEQUENCES_A] +
           [("C4", s) for s in MESH_SEQUENCES_A])
CASES_B = [("C2", "b_multi3"), ("C2", "b_1x3_overlap1"), ("C2", "b_1x3_overlap0"), ("C2", "b_2x2_auto"),
           ("C3", "b_2x2_auto"), ("C4", "b_2x2_direct"), ("C2", "b_rank1of3"), ("C2", "b_2x2_service")]


@pytest.fixture(autouse=True)
def _fresh_delays():
    sc.forget_delays()
    yield
    sc.forget_delays()


def _no_difference(got, want, what, rows=None):
    for k in IMAGES:
        g, w = got[k], want[k]
        if rows is not None:
            g, w = g.reshape(-1, 4)[rows], w.reshape(-1, 4)[rows]
        n = sc.differing(g, w)
        assert n == 0, f"{what}: {k}: {n} pixels differ"


def _against_oracle(scene_name, seq, got, what):
    """The rendered region (whole 16x16 tiles; a rank's own tiles) against the portable oracle."""
    s = sc.scene(scene_name)
    w, h = s["width"], s["height"]
    want = sc.oracle_images(scene_name, sum(seq["calls"]))
    if "tiling" in seq:
        rows = sc.owned_pixels(w, h, *seq["tiling"])
    else:
        yy, xx = np.mgrid[0:(h // 16) * 16, 0:(w // 16) * 16]
        rows = (yy * w + xx).reshape(-1)
    _no_difference(got, want, what, rows)


def test_delay_calibration_and_host_path(native):
    """The delay every other test leans on: torch.cuda._sleep calibrated with
    torch events to about 30 ms (never above 100 ms), and the host's way from
    enqueuing it to the library's launch -- delay, copy, an unsynchronised
    render call -- a tenth of the 20 ms the delay must last, or less."""
    import torch
    cal = sc.calibration()
    s = sc.scene("C2")
    r = sc.new_renderer(s, {})
    side = torch.cuda.Stream(0)
    host = sc.host_path_ms(r, s, side)
    r.cleanUp()
    ms = sc.check_delays(expected=3)
    print(f"\nstreams: torch.cuda._sleep {cal['cycles_per_ms']:.0f} cycles/ms (probes {cal['probes']}), "
          f"{cal['delay_cycles']} cycles per delay, measured {[round(m, 2) for m in ms]} ms; host path {host:.3f} ms")
    assert max(ms) <= sc.MAX_DELAY_MS
    assert host <= sc.MAX_HOST_PATH_MS, f"host path {host:.3f} ms: 20 ms is not ten times it"


# ---- A. results do not depend on whose stream it is -----------------------------------------
@pytest.mark.parametrize("placement", sc.PLACEMENTS)
@pytest.mark.parametrize("scene_name,seq_name", CASES_A)
def test_render_on_callers_stream_equals_untouched_context_and_oracle(native, oracle, scene_name, seq_name, placement):
    """Every launch kind on a context whose stream is the caller's: accum,
    RGBA8, depth and the frame count equal, bit for bit, the same calls on a
    context that never handed anything out and (mesh scenes) the oracle; the
    launch kind is the one the sequence is there for; no synchronisation of a
    shared context ends by the completion flag."""
    s, seq = sc.scene(scene_name), sc.SEQUENCES[seq_name]
    r = sc.new_renderer(s, seq)
    shared = sc.Shared(r, placement)
    kinds = sc.run_calls(r, s, seq)
    got = sc.read_all(r)
    info = r.sync_info()
    r.cleanUp()
    del shared
    want = sc.untouched(scene_name, seq_name)
    expected = seq["kind"] if scene_name != "C4" else "render_kernel"
    # (a launch a retiring session kernel refused, or a one-frame call the graph did not take, is a plain launch)
    for ks in (kinds, want["kinds"]):
        assert expected in ks and set(ks) <= {expected, "path_pool"}, (kinds, want["kinds"])
    assert got["frames"] == want["frames"] == sum(seq["calls"])
    assert info["flag"] == 0, info
    _no_difference(got, want, f"{scene_name} {seq_name} on a {placement} stream vs an untouched context")
    if scene_name != "C4":
        _against_oracle(scene_name, seq, got, f"{scene_name} {seq_name} on a {placement} stream vs the oracle")


@pytest.mark.parametrize("scene_name", ["C2", "C3"])
def test_switching_streams_mid_run(native, oracle, scene_name):
    """Two unsynchronised frames on s1, vrhip_set_stream(s2), two more, back
    to the context's own stream, two more: the six frames of one context and
    of the oracle."""
    import torch
    s = sc.scene(scene_name)
    seq = dict(calls=[1, 1], sync=False)
    r = sc.new_renderer(s, seq)
    s1, s2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
    r.set_stream(s1.cuda_stream)
    sc.run_calls(r, s, seq, 0)
    r.set_stream(s2.cuda_stream)
    sc.run_calls(r, s, seq, 2)
    r.set_stream(0)
    sc.run_calls(r, s, seq, 4)
    got = sc.read_all(r)
    r.cleanUp()
    want = sc.untouched(scene_name, "sync1x6")
    assert got["frames"] == want["frames"] == 6
    _no_difference(got, want, f"{scene_name} over three streams vs one context")
    _against_oracle(scene_name, sc.SEQUENCES["sync1x6"], got, f"{scene_name} over three streams vs the oracle")


# ---- B. work queued behind a render sees it ----------------------------------------------------
@pytest.mark.parametrize("placement", sc.PLACEMENTS)
@pytest.mark.parametrize("scene_name,seq_name", CASES_B)
def test_copy_queued_behind_render_sees_it(native, scene_name, seq_name, placement):
    """The stream and the buffers are fetched once, up front.  Behind a delay
    (so that every launch is still pending when the next call and the copies
    are made) the unsynchronised renders, then at once device-to-device copies
    of accum, RGBA8 and depth queued on the caller's stream, then a wait for
    that stream alone: the copies equal, bit for bit, what an untouched
    context reads back.  In the default service mode this fails if a context
    whose stream is shared joins a render service session by itself (the
    second call's frames then arrive with the next closing call); in explicit
    mode the closing call (vrhip_device_buffers) must order the session's
    finish pass on the caller's stream without waiting on the host."""
    import torch
    s, seq = sc.scene(scene_name), sc.SEQUENCES[seq_name]
    w, h = s["width"], s["height"]
    r = sc.new_renderer(s, seq)
    shared = sc.Shared(r, placement)
    bufs = r.device_buffers()
    sizes = (16 * w * h, 4 * w * h, 4 * w * h)
    dst = [torch.zeros(n, dtype=torch.uint8, device="cuda:0") for n in sizes]
    torch.cuda.synchronize()
    sc.delay(shared.s)
    sc.run_calls(r, s, seq)
    use_scratch = r.last_launch_info()["use_scratch"]
    if seq.get("reclose"):
        assert r.device_buffers() == bufs
    for d, p, n in zip(dst, bufs, sizes):
        sc.copy_on(shared.s, d, p, n)
    shared.s.synchronize()
    got = {"accum": dst[0].cpu().numpy().view(np.float32).reshape(h, w, 4),
           "rgba8": dst[1].cpu().numpy().reshape(h, w, 4), "depth8": dst[2].cpu().numpy().reshape(h, w, 4)}
    sc.check_delays(expected=1)
    r.cleanUp()
    del shared
    if seq_name == "b_2x2_direct":
        assert use_scratch == 0                       # direct mode: the render kernel itself wrote the images
    want = sc.untouched(scene_name, seq_name)
    for k in IMAGES:
        n = sc.differing(got[k], want[k])
        assert n == 0, f"{scene_name} {seq_name}, {placement} stream: {k} copied behind the renders: {n} pixels differ"


@pytest.mark.parametrize("placement", sc.PLACEMENTS)
def test_sync_waits_for_callers_work_on_shared_stream(native, placement):
    """vrhip_sync on a handed-out stream waits for the whole stream: with a
    delay queued behind a render, the stream has nothing left when it returns."""
    s = sc.scene("C2")
    r = sc.new_renderer(s, {})
    shared = sc.Shared(r, placement)
    r.render(frames=1, times=[s["time"]], sync=False)
    sc.delay(shared.s)
    r.sync()
    done = shared.s.query()
    shared.s.synchronize()
    sc.check_delays(expected=1)
    r.cleanUp()
    assert done, "vrhip_sync returned while the caller's work on the context stream was still running"


# ---- C. inputs still being produced on the context stream ---------------------------------------
@pytest.mark.parametrize("placement", sc.PLACEMENTS)
@pytest.mark.parametrize("case_name,pending", sc.case_inputs())
def test_input_pending_on_context_stream(native, case_name, pending, placement):
    """The raw C ABI (no wrapper synchronisation) on the caller's stream: the
    input holds a valid decoy A, and on that stream a delay, the copy of B
    over it, then the call.  The result is B's on a quiescent context, word
    for word, and is not A's (or the case would prove nothing)."""
    import torch
    case = sc.CASES[case_name]
    want, decoy = sc.quiet(case_name, None, "raw"), sc.quiet(case_name, pending, "raw")
    assert not sc.same(want, decoy), f"{case_name}: decoy and input {pending} give the same result"
    r = case.context()
    shared = sc.Shared(r, placement)
    got = sc.pending_call(case, r, pending, shared.s, "raw")
    torch.cuda.synchronize()
    sc.check_delays(expected=1)
    r.cleanUp()
    del shared
    assert not sc.same(got, decoy), f"{case_name}: {pending} was read before the copy queued ahead of the call"
    assert sc.same(got, want), f"{case_name}: {pending} pending on the context stream: " \
                               f"{int((got != want).sum()) if got.shape == want.shape else 'all'} words differ"


CONTROL_STREAMS = 4


@pytest.mark.parametrize("case_name,pending", [("trace_rays", "origins"), ("denoise", "color")])
def test_control_input_pending_on_another_stream_is_not_waited_for(native, case_name, pending):
    """The control that shows the delay bites: the same raw call on a context
    that kept its OWN stream, the input pending on a torch side stream.
    Nothing in the library orders the two, so the call returns the decoy's
    result -- unless the runtime has put both streams on one hardware queue
    (it has four by default and deals streams over them), which serialises
    them by accident.  So the control runs on four torch streams taken one
    after the other, each with a fresh context: every result is A's or B's,
    and A's on at least one.  (A is valid data and the copy lands tens of
    milliseconds after the query has finished: nothing is read while it is
    written.)"""
    import torch
    case = sc.CASES[case_name]
    want, decoy = sc.quiet(case_name, None, "raw"), sc.quiet(case_name, pending, "raw")
    assert not sc.same(want, decoy)
    sides = [torch.cuda.Stream(0) for _ in range(CONTROL_STREAMS)]
    outcomes = []
    for side in sides:
        r = case.context()
        got = sc.pending_call(case, r, pending, side, "raw")
        torch.cuda.synchronize()
        r.cleanUp()
        outcomes.append("A" if sc.same(got, decoy) else "B" if sc.same(got, want) else "other")
    sc.check_delays(expected=CONTROL_STREAMS)
    print(f"\nstreams: control {case_name}: {outcomes}")
    assert set(outcomes) <= {"A", "B"}, outcomes
    assert "A" in outcomes, f"{case_name}: no stream of {CONTROL_STREAMS} returned the decoy's result: {outcomes}"


# ---- D. the wrappers' synchronisation ------------------------------------------------------------
def _current_stream(which):
    import torch
    return torch.cuda.default_stream(0) if which == "default" else torch.cuda.Stream(0)


@pytest.mark.parametrize("current", ["default", "side"])
@pytest.mark.parametrize("case_name,pending", sc.case_inputs())
def test_wrapper_waits_for_torchs_current_stream(native, case_name, pending, current):
    """VRendererHIP on a context with its own stream, torch's current stream
    the default stream or a side stream: decoy A in the input, then on the
    current stream a delay and the copy of B, then the method.  The result is
    B's and not A's.  This fails if the method's
    torch.cuda.current_stream(dev).synchronize() goes missing: the query runs
    on the renderer's own non-blocking stream, which waits for no torch stream.
    (With Stream.synchronize made a no-op all 54 cases and the four
    drawn-seed cases fail: profiles/streams/README.md.)"""
    import torch
    case = sc.CASES[case_name]
    want, decoy = sc.quiet(case_name, None, "wrapped"), sc.quiet(case_name, pending, "wrapped")
    assert not sc.same(want, decoy), f"{case_name}: decoy and input {pending} give the same result"
    r = case.context()
    got = sc.pending_call(case, r, pending, _current_stream(current), "wrapped")
    torch.cuda.synchronize()
    sc.check_delays(expected=1)
    r.cleanUp()
    assert not sc.same(got, decoy), f"{case.method}: {pending} was read before torch's {current} stream had written it"
    assert sc.same(got, want), f"{case.method}: {pending} pending on torch's {current} stream: result differs from B's"


@pytest.mark.parametrize("current", ["default", "side"])
@pytest.mark.parametrize("method", ["traceRadiance", "shadeSurface"])
def test_wrapper_drawn_seeds_wait_for_current_stream(native, method, current):
    """seeds=None draws the seeds with torch.randint on torch's current
    stream.  Behind a delay on that stream, two calls under the same
    torch.manual_seed each give the result of the same seeds passed explicitly,
    and neither gives the result of zero seeds.  The explicit and the zero-seed
    calls come first, so that no later call allocates (an allocation may wait
    for the device and order the draw by accident);
    before each seeds=None call a zeroed block of the seeds' size goes back to
    torch's allocator, so a query that ran ahead of the draw reads zeros or
    other stale words, never the seeds.  This fails if the method's
    torch.cuda.current_stream(dev).synchronize() goes missing."""
    import torch
    case = sc.CASES["trace_radiance" if method == "traceRadiance" else "shade_surface"]
    r = case.context()
    t = sc.device_inputs(case)
    first = t["origins"] if method == "traceRadiance" else t["records"]
    call = getattr(r, method)
    outs = []
    with torch.cuda.stream(_current_stream(current)):
        cur = torch.cuda.current_stream(0)
        torch.manual_seed(20250607)
        seeds = torch.randint(-2**31, 2**31, (sc.N, 2), dtype=torch.int32, device="cuda:0")
        explicit = sc.words(call(first, t["dirs"], seeds, samples=2))
        zeros = sc.words(call(first, t["dirs"], torch.zeros_like(seeds), samples=2))
        del seeds
        for _i in range(2):
            stale = torch.zeros((sc.N, 2), dtype=torch.int32, device="cuda:0")
            cur.synchronize()
            del stale
            sc.delay(cur)
            torch.manual_seed(20250607)
            outs.append(sc.words(call(first, t["dirs"], samples=2)))
    torch.cuda.synchronize()
    sc.check_delays(expected=2)
    r.cleanUp()
    assert not sc.same(explicit, zeros), "the drawn seeds and zero seeds give the same result"
    for i, out in enumerate(outs):
        assert not sc.same(out, zeros), f"{method}(seeds=None), call {i}: the result of zero seeds"
        assert sc.same(out, explicit), f"{method}(seeds=None), call {i}: differs from the same seeds passed explicitly"
