"""The sphere test's tail without its range vote and without its sign test
(vr_kernel.hpp sphere_tail), restated in numpy float32 beside the tail it
replaces (sphere_intersect: det -> sqrtf -> the t select).

sqrt_rn is v_sqrt_f32 corrected to the nearest float.  From 2^-96 up it IS
sqrtf (the GPU's exhaustive check, vrhip_selftest_sqrt), so np.sqrt stands for
it there.  Below 2^-96 the kernel no longer asks what it returns: the comment
at sphere_tail bounds it by [0, 2^-47] and argues that no root in that range
changes an outcome, for any b; for a negative det the hardware root is a NaN.
That argument is what this file sweeps: every candidate root of the range
(ROOTS_BELOW) must give the old outcome, by bits.
"""
import numpy as np
import pytest

f32 = np.float32
EPS = f32(1e-4)
LO = f32(2.0 ** -96)


def u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def old_tail(b, det):
    """sphere_intersect from det on: 0 for a miss."""
    with np.errstate(invalid="ignore"):
        s = np.sqrt(det)
    t0, t1 = b - s, b + s
    t = np.where(t0 > EPS, t0, np.where(t1 > EPS, t1, f32(0)))
    return np.where(det < 0, f32(0), t).astype(f32)


def new_tail(b, det, root=None):
    """sphere_tail: +inf for a miss.  `root`: what sqrt_rn returns for the
    dets below 2^-96 (a function of det); negative dets give a NaN."""
    with np.errstate(invalid="ignore"):
        s = np.sqrt(det)
        if root is not None:
            s = np.where(det < LO, root(det), s)
        s = np.where(det < 0, f32(np.nan), s).astype(f32)          # (-0 < 0 is false: its root is sqrt(-0) = -0)
        t0, t1 = b - s, b + s
        return np.where(t0 > EPS, t0, np.where(t1 > EPS, t1, f32(np.inf))).astype(f32)


def _moved(k):
    def f(det):
        with np.errstate(invalid="ignore"):
            s = np.sqrt(np.maximum(det, f32(0)))
        for _ in range(abs(k)):
            s = np.nextafter(s, f32(np.inf if k > 0 else 0.0))
        return s.astype(f32)
    return f


# what sqrt_rn may return for 0 <= det < 2^-96: the true root and its
# neighbours (the hardware root within an ulp, corrected by at most one), 0
# (a denormal det read as 0), the smallest denormal, and the bound itself
ROOTS_BELOW = {"sqrtf": _moved(0), "-1 ulp": _moved(-1), "-2 ulp": _moved(-2), "+1 ulp": _moved(1), "+2 ulp": _moved(2),
               "zero": lambda det: np.zeros_like(det), "denormal": lambda det: np.full_like(det, f32(2.0 ** -149)),
               "2^-47": lambda det: np.full_like(det, f32(2.0 ** -47))}


def outcome(t_new):
    """The fold reads a miss as `not closer than anything`: the old tail's 0."""
    return np.where(np.isinf(t_new), f32(0), t_new).astype(f32)


def neighbours(x):
    x = np.asarray(x, f32)
    return np.unique(np.concatenate([x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))]))


def b_grid():
    """Signed logarithmic grid 2^-149 .. 2^17 (every power of two and a point
    between each pair), +-1e-4 and its neighbours, and 0."""
    e = np.arange(-149, 18, dtype=np.float64)
    mags = np.concatenate([np.exp2(e), np.exp2(e[:-1] + 0.5)]).astype(f32)
    near = neighbours(neighbours([EPS]))
    # the boundaries of the proof's two cases
    edge = neighbours(neighbours(np.array([2.0 ** -14, 2.0 ** -24, 2.0 ** -13], f32)))
    g = np.concatenate([mags, near, edge])
    return np.unique(np.concatenate([g, -g, [f32(0)]])).astype(f32)


def small_dets():
    """0, -0, every power of two from the smallest denormal to 2^-90 with its
    neighbours, and 10^5 random values below 2^-96."""
    pw = np.exp2(np.arange(-149, -89, dtype=np.float64)).astype(f32)
    rng = np.random.default_rng(960)
    # random bit patterns of [0, 2^-96): uniform over the floats, denormals included
    rnd = rng.integers(0, int(u32([LO])[0]), 100_000, dtype=np.uint32).view(f32)
    assert (rnd < LO).all() and (rnd >= 0).all()
    return np.unique(np.concatenate([neighbours(pw), rnd, [f32(0)]])), np.array([-0.0], f32)


def same(b, det, root=None, chunk=32):
    """Old and new outcomes over the grid b x det, equal by bits; returns
    whether the grid reached a miss and a hit."""
    miss = hit = False
    for i in range(0, len(b), chunk):
        B, D = np.meshgrid(b[i:i + chunk], det, indexing="ij")
        with np.errstate(over="ignore"):
            old, new = old_tail(B, D), outcome(new_tail(B, D, root))
        bad = np.argwhere(u32(old) != u32(new))
        assert len(bad) == 0, (f"{len(bad)} of {old.size} outcomes differ; first: b={B[tuple(bad[0])]!r} "
                               f"det={D[tuple(bad[0])]!r} old={old[tuple(bad[0])]!r} new={new[tuple(bad[0])]!r}")
        miss |= bool((old == 0).any())
        hit |= bool((old > EPS).any())
    return miss, hit


@pytest.mark.parametrize("root", list(ROOTS_BELOW))
def test_below_the_exact_range(root):
    """0 <= det < 2^-96 (and the powers up to 2^-90 around it): whichever
    root of [0, 2^-47] sqrt_rn returns there, the outcome is the old one for
    every b, by bits."""
    b = b_grid()
    dets, neg0 = small_dets()
    assert (dets < LO).sum() > 100_000 and (dets >= LO).any() and dets.min() == 0
    if root != "sqrtf":                      # the other candidates: every power of two and an eighth of the random values
        dets = np.unique(np.concatenate([dets[::8], neighbours(np.exp2(np.arange(-149, -89, dtype=np.float64)).astype(f32))]))
    miss, hit = same(b, dets, ROOTS_BELOW[root])
    assert miss and hit                      # the sweep reaches both outcomes: 0 and t = b
    assert (ROOTS_BELOW[root](dets[dets < LO]) <= f32(2.0 ** -47)).all()


def test_negative_and_minus_zero():
    """det < 0: the NaN root misses, as the reference's early return; -0: the root is -0 and t = b."""
    b = b_grid()
    dets, neg0 = small_dets()
    rng = np.random.default_rng(962)
    neg = np.concatenate([-dets[1:2000], -np.exp2(rng.uniform(-149, 84, 5000)).astype(f32), [f32(-np.inf)]])
    miss, hit = same(b, neg)
    assert miss and not hit
    same(b, neg0)
    assert np.signbit(np.sqrt(neg0)).all()


def test_in_the_exact_range():
    """det >= 2^-96: the tail is the old one with np.sqrt for sqrt_rn, up to the largest det a straight ray can give (< 2^127)."""
    b = b_grid()
    e = np.arange(-96, 127, dtype=np.float64)
    rng = np.random.default_rng(961)
    dets = np.concatenate([neighbours(np.exp2(e).astype(f32)), np.exp2(rng.uniform(-96, 127, 20_000)).astype(f32)])
    dets = dets[dets >= LO]
    miss, hit = same(b, dets)
    assert miss and hit
    # geometry-sized values: b and det of rays inside the box
    b2 = rng.uniform(-300.0, 300.0, 2_000).astype(f32)
    d2 = rng.uniform(0.0, 1.0e5, 2_000).astype(f32)
    same(b2, d2[d2 >= LO])


def test_root_at_zero():
    """sqrt_rn's arithmetic at +0 (vr_math.hpp: a draw's root needs no vote):
    s = +0, the lower neighbour's pattern is a NaN, both residual tests fail."""
    s = f32(0)
    sm = (u32([s]) - np.uint32(1)).view(f32)[0]
    sp = (u32([s]) + np.uint32(1)).view(f32)[0]
    assert np.isnan(sm) and sp == f32(2.0 ** -149)
    with np.errstate(invalid="ignore"):
        rm = f32(-np.float64(sm) * np.float64(s) + 0.0)     # the fma's exact product, rounded once
        rp = f32(-np.float64(sp) * np.float64(s) + 0.0)
        t = sm if rm <= 0 else s
        r = sp if rp > 0 else t
    assert u32([r])[0] == 0
    # a uniform draw is 0 or at least 2^-31, and so is 1 - u: multiples of 2^-31 rounded to fp32
    k = np.array([0, 1, 2, 3, 2**24 - 1, 2**24 + 1, 2**31 - 3, 2**31 - 2], np.uint32)
    u = k.astype(f32) * f32(4.656612873077392578125e-10)
    for x in (u, f32(1) - u):
        assert ((x == 0) | (x >= f32(2.0 ** -31))).all() and (x <= 1).all()
