"""The inputs shading sees: map shapes, uv ranges, degenerate attributes, texel values.

One recipe per case, in the manner of ref_cases.py and flag_lattice.py,
shared by tests/ref_cases.py (the `shading` family of reference-rendered
fixtures), tests/test_shading_cpu.py (what the case set pins, from the oracle
alone) and tests/test_gpu_shading.py (the HIP kernels against the oracle over
traversal modes and launch kinds).  Inputs are regenerated from fixed numpy
generators; nothing is stored.  Every case is a 64 x 48 image of the (24, 12)
knot with leaves of 2, two frames.

  S_<set>_<scene>  three maps of three different, non-square, non-power-of-two
                   sizes and an HDRI of another, over C3 and seven class scenes
  U_<scene>        the odd set with uvs in [-1, 2): a negative x wraps into the
                   previous row, which shows only when w is no power of two
  D_<what>_<scene> all tangents zero, every third vertex's tangent zero, every
                   third vertex's normal zero
  V_<what>         texels of exactly 0 and 1, HDRI rows of 65504, 0 and +inf
  X_<what>_<scene> inputs on which a host build of the reference has undefined
                   behaviour (a float -> int conversion out of range or of a
                   NaN): pinned to the oracle alone, which restates CUDA's
                   conversion (truncate, saturate, NaN -> 0)

What a shape case pins is measured, not assumed: mutant_counts() renders the
oracle on the case with its maps' sizes mangled the way a wrong kernel would
(MUTANTS) and counts the pixels whose accumulation changes; check_case()
asserts at least MIN_MUTANT of the rendered pixels for every mutant that
touches a map the scene reads.  The X_ cases that make NaNs must make them on
at least MIN_NAN and at most MAX_NAN of the rendered pixels.
"""
from __future__ import annotations

import functools

import numpy as np

import flag_lattice as fl
import pyoracle as po
import ref_cases as rc

W, H = rc.W, rc.H
KNOT, LEAF = (24, 12), 2
TIMES = [12345, 13354]                      # ref_cases.times_of: two frames
TEX_KEYS = ("tex_diffuse", "tex_normal", "tex_specular")
MAP_KEYS = TEX_KEYS + ("hdr",)
CLASS_SCENES = ("C2D", "C3D", "C2N", "C3B", "C1T", "C4D", "C3X")
MIN_MUTANT = 0.01
MIN_NAN, MAX_NAN = 0.01, 0.05

# (width, height) of the diffuse, normal and specular map, and of the HDRI.  Under the HDRI every hit of the
# example sphere reads the texel at uv (0.5, 0.5) (its uv comes from the previous hit's normal, and there is none):
# x + y * w there is the same for w x h and h x w when both are odd, so each set's diffuse map has an even side,
# and the `dot` set's seed is one whose normal-map texel there does not turn the sphere black.
SHAPES = {
    "odd": dict(seed=101, tex=((38, 101), (6, 3), (1, 1)), hdr=(19, 53)),
    "tall": dict(seed=102, tex=((6, 129), (1, 67), (3, 200)), hdr=(1, 33)),        # a one-column map, a one-column HDRI
    "dot": dict(seed=104, tex=((6, 11), (9, 2), (3, 6)), hdr=(1, 1)),
    "half": dict(seed=120, tex=((37, 101), (6, 5), (1, 1)), hdr=(19, 53)),         # X_: one normal-map texel of exactly 0.5
}

CASES = {}
for _set in ("odd", "tall", "dot"):
    for _scene in ("C3",) + CLASS_SCENES:
        CASES[f"S_{_set}_{_scene}"] = dict(scene=_scene, shapes=_set)
for _scene in ("C3", "C2D", "C2N"):
    CASES[f"U_{_scene}"] = dict(scene=_scene, shapes="odd", mesh="uv3")
for _what in ("tan0", "tan0_third", "nrm0_third"):
    for _scene in ("C3", "C3B", "C2N"):
        CASES[f"D_{_what}_{_scene}"] = dict(scene=_scene, shapes="odd", mesh=_what)
CASES["V_texels01_C3"] = dict(scene="C3", shapes="tall", values="texels01")
CASES["V_texels01_C1T"] = dict(scene="C1T", shapes="tall", values="texels01")
CASES["V_hdr_inf_C3"] = dict(scene="C3", shapes="odd", values="hdr_inf")
CASES["X_uv_huge_C3"] = dict(scene="C3", shapes="odd", mesh="uv_huge")
CASES["X_uv_huge_C2D"] = dict(scene="C2D", shapes="odd", mesh="uv_huge")
CASES["X_uv_nonfinite_C3"] = dict(scene="C3", shapes="odd", mesh="uv_nonfinite")
CASES["X_nmap_half_C3"] = dict(scene="C3", shapes="half", values="nmap_half", nan=True)
CASES["X_nmap_half_C1T"] = dict(scene="C1T", shapes="half", values="nmap_half")     # a NaN ray leaves the box: black
CASES["X_nrm0_tris_C3"] = dict(scene="C3", shapes="odd", mesh="nrm0_tris", nan=True)
CASES["X_nrm0_tris_C3B"] = dict(scene="C3B", shapes="odd", mesh="nrm0_tris", nan=True)
CASES["X_nrm0_tris_C2N"] = dict(scene="C2N", shapes="odd", mesh="nrm0_tris")           # likewise: no HDRI lookup
del _set, _scene, _what

NAN_CASES = tuple(n for n, c in CASES.items() if c.get("nan"))
ORACLE_ONLY = tuple(n for n in CASES if n.startswith("X_"))
SHAPE_CASES = tuple(n for n in CASES if n[:2] in ("S_", "U_"))


# ---- inputs ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def maps_of(shapes, values=None) -> dict:
    """The four maps of a shape set as float32 (h, w, 4), never written:
    uniform noise, so neighbouring texels differ; the normal map's z >= 0.6 so
    that no normal-map vector 2 t - 1 is near zero; the HDRI quantised to half
    as an OpenEXR image is."""
    s = SHAPES[shapes]
    rng = np.random.default_rng(s["seed"])
    out = {}
    for key, (w, h) in zip(TEX_KEYS, s["tex"]):
        t = np.ones((h, w, 4), np.float32)
        if key == "tex_normal":
            t[..., :2] = rng.uniform(0.2, 0.8, (h, w, 2))
            t[..., 2] = rng.uniform(0.6, 1.0, (h, w))
        else:
            t[..., :3] = rng.uniform(0.05, 0.95, (h, w, 3))
        out[key] = t
    w, h = s["hdr"]
    hdr = np.ones((h, w, 4), np.float32)
    hdr[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float16)
    out["hdr"] = hdr
    if values == "texels01":
        # a third of the diffuse and specular texels exactly 0, a third exactly 1; HDRI rows of 65504 and of 0
        for key in ("tex_diffuse", "tex_specular"):
            pick = rng.integers(0, 3, out[key].shape[:2])
            out[key][pick == 0, :3] = 0.0
            out[key][pick == 1, :3] = 1.0
        hdr[0::4, :, :3] = 65504.0
        hdr[1::4, :, :3] = 0.0
    elif values == "hdr_inf":
        hdr[0::4, :, :3] = np.inf
    elif values == "nmap_half":
        t = out["tex_normal"]
        t[t.shape[0] // 2, t.shape[1] // 2, :3] = 0.5                   # 2 t - 1 = 0: its normalisation is 0 / 0
    elif values is not None:
        raise ValueError(values)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mesh_of(kind="plain") -> dict:
    """The flat (24, 12) knot with leaves of 2, its attributes as `kind` says."""
    from vrenderer_pathtracer_amd import build_flat, scenes
    m = {k: np.array(v) for k, v in scenes.torus_knot(*KNOT).items()}
    nv = len(m["positions"])
    third = np.arange(nv) % 3 == 0
    if kind == "plain":
        pass
    elif kind == "uv3":                              # uvs in [-1, 2)
        m["uvs"] = (m["uvs"] * np.float32(3) - np.float32(1)).astype(np.float32)
    elif kind == "tan0":
        m["tangents"][:] = 0.0
    elif kind == "tan0_third":                       # the interpolated tangent is short, not zero
        m["tangents"][third] = 0.0
    elif kind == "nrm0_third":
        m["normals"][third] = 0.0
    elif kind == "uv_huge":                          # dim * u beyond the int range on both sides
        m["uvs"][np.arange(nv) % 5 == 0] *= np.float32(1e9)
        m["uvs"][np.arange(nv) % 5 == 1] *= np.float32(-1e9)
    elif kind == "uv_nonfinite":
        m["uvs"][np.arange(nv) % 7 == 0] = np.nan
        m["uvs"][np.arange(nv) % 7 == 1] = np.inf
        m["uvs"][np.arange(nv) % 7 == 2, 0] = -np.inf
    elif kind == "nrm0_tris":                        # every eighth triangle's three normals zero: unshared vertices
        t = m["tris"].astype(np.int64).reshape(-1)
        m = dict(positions=m["positions"][t], normals=m["normals"][t], tangents=m["tangents"][t], uvs=m["uvs"][t],
                 tris=np.arange(len(t), dtype=np.uint32).reshape(-1, 3))
        m["normals"].reshape(-1, 3, 3)[::8] = 0.0
    else:
        raise ValueError(kind)
    flat = build_flat(m, max_leaf_tris=LEAF)
    for a in flat.values():
        a.setflags(write=False)
    return flat


@functools.lru_cache(maxsize=None)
def _base(scene) -> dict:
    from vrenderer_pathtracer_amd import scenes
    if scene == "C3":
        return scenes.make_scene("C3", W, H, knot=KNOT)
    from test_gpu_classes import class_scene
    return class_scene(scene, W, H)


def make_case(name) -> dict:
    """The scene dict of a case: its base scene with every map it loads and
    its mesh replaced."""
    c = CASES[name]
    sc = dict(_base(c["scene"]))
    maps = maps_of(c["shapes"], c.get("values"))
    for key in MAP_KEYS:
        if sc.get(key) is not None:
            sc[key] = maps[key]
    if sc.get("mesh_flat") is not None:
        sc["mesh_flat"] = mesh_of(c.get("mesh", "plain"))
    sc["name"] = name
    return sc


def combo_of(sc) -> tuple:
    """The scene's flags as a combination of tests/flag_lattice.py."""
    return tuple(int(bool(v)) for v in (
        sc.get("cornell"), sc.get("example_sphere"), sc.get("view_brdf"), sc.get("mesh_flat") is not None,
        sc.get("brdf") is not None, sc.get("tex_diffuse") is not None, sc.get("tex_normal") is not None,
        sc.get("tex_specular") is not None))


def kernel_of(name, strict=False) -> str:
    return fl.kernel_of(combo_of(make_case(name)), strict)


# ---- the oracle ----------------------------------------------------------------------
def region(a):
    return a[:(H // 16) * 16, :(W // 16) * 16]


def _render(sc):
    po.build()
    return po.render(sc, frames=len(TIMES), times=TIMES, libm=po.LIBM_PORTABLE)[:3]


@functools.lru_cache(maxsize=None)
def oracle_render(name):
    """(accum, rgba8, depth8) of the portable-libm oracle: rendered once, shared, never written."""
    out = _render(make_case(name))
    for a in out:
        a.setflags(write=False)
    return out


def nan_pixels(accum) -> np.ndarray:
    return np.isnan(region(accum)).any(-1)


def nan_share(name) -> float:
    return float(nan_pixels(oracle_render(name)[0]).mean())


# ---- mutants ---------------------------------------------------------------------------
def _pow2(n):
    return 1 << (int(n).bit_length() - 1)


def _resized(a, w, h):
    """The buffer of map `a` read as w x h: cropped, or padded with zero texels."""
    flat = np.asarray(a, np.float32).reshape(-1, 4)
    out = np.zeros((w * h, 4), np.float32)
    n = min(len(flat), w * h)
    out[:n] = flat[:n]
    return out.reshape(h, w, 4)


def maps_read(sc) -> tuple:
    """The maps a scene's shading reads: those it loads, except that the BRDF
    view takes neither colour nor specular from a map."""
    keys = [k for k in MAP_KEYS if sc.get(k) is not None]
    if sc.get("view_brdf"):
        keys = [k for k in keys if k not in ("tex_diffuse", "tex_specular")]
    return tuple(keys)


def mutants(sc) -> dict:
    """{mutant: scene}: the case as a kernel with a wrong idea of a map's size
    would see it.  Only mutants that change a map the scene reads.
      swap        every map's width and height exchanged, the same buffers
      swap:<map>  one map's width and height exchanged
      first       every map after the first one loaded given that one's size
                  (map 1 and map 2 given map 0's), the buffer padded or cropped
      pow2        every size rounded down to a power of two, the buffer cropped"""
    read = maps_read(sc)
    out = {}
    swapped = {k: np.ascontiguousarray(sc[k]).reshape(sc[k].shape[1], sc[k].shape[0], 4)
               for k in read if sc[k].shape[0] != sc[k].shape[1]}
    if swapped:
        out["swap"] = dict(sc, **swapped)
        for key, a in swapped.items():
            out[f"swap:{key}"] = dict(sc, **{key: a})
    loaded = [k for k in TEX_KEYS if sc.get(k) is not None]
    if len(loaded) > 1:
        h0, w0 = sc[loaded[0]].shape[:2]
        changed = {k: _resized(sc[k], w0, h0) for k in loaded[1:] if sc[k].shape[:2] != (h0, w0)}
        if any(k in read for k in changed):
            out["first"] = dict(sc, **changed)
    changed = {}
    for key in [k for k in MAP_KEYS if sc.get(k) is not None]:
        h, w = sc[key].shape[:2]
        if (_pow2(w), _pow2(h)) != (w, h):
            changed[key] = _resized(sc[key], _pow2(w), _pow2(h))
    if any(k in read for k in changed):
        out["pow2"] = dict(sc, **changed)
    return out


@functools.lru_cache(maxsize=None)
def mutant_counts(name) -> dict:
    """{mutant: rendered pixels whose oracle accumulation the mutant changes}."""
    want = region(oracle_render(name)[0]).view(np.uint32)
    return {m: int((region(_render(sc)[0]).view(np.uint32) != want).any(-1).sum())
            for m, sc in mutants(make_case(name)).items()}


def check_case(name) -> None:
    """The conditions on a case's inputs (module docstring), from the oracle alone."""
    accum = oracle_render(name)[0]
    n_px = region(accum)[..., 0].size
    assert np.any(region(accum)[..., :3] != 0), f"{name}: a black image"
    if name in SHAPE_CASES:
        counts = mutant_counts(name)
        kinds = {m.split(":")[0] for m in counts}
        assert {"swap", "pow2"} <= kinds, f"{name}: no map the scene reads has a size these mutants change ({counts})"
        weak = {m: n for m, n in counts.items() if ":" not in m and n < MIN_MUTANT * n_px}
        assert not weak, f"{name}: mutants that change fewer than {MIN_MUTANT:.0%} of {n_px} pixels: {weak}"
    n_nan = int(nan_pixels(accum).sum())
    if name in NAN_CASES:
        assert MIN_NAN * n_px <= n_nan <= MAX_NAN * n_px, f"{name}: {n_nan} of {n_px} pixels hold a NaN"
        assert not np.isnan(region(accum)[..., 3]).any(), f"{name}: a NaN depth term"
    else:
        assert n_nan == 0, f"{name}: {n_nan} pixels hold a NaN in a case that is compared bit for bit"


# ---- device-resident meshes with missing attributes ----------------------------------------
# initMeshDevice takes None for normals, tangents or uvs and stores zeros.  Zero tangents skip the normal map (the
# face normal is used); zero normals under a normal map with real tangents make the normal 0 / 0 on every mesh hit,
# so that variant looks at the knot from farther away, where it covers under MAX_NAN of the image.
DEVICE_VARIANTS = {"no_normals": ("normals",), "no_tangents": ("tangents",), "no_uvs": ("uvs",),
                   "bare": ("normals", "tangents", "uvs")}
DEVICE_SCENES = ("C3", "C3B")
DEVICE_NAN_VARIANTS = ("no_normals",)
FAR_CAMERA_Z = 400.0


def device_mesh(variant=None) -> dict:
    """The indexed (24, 12) knot without the attributes the variant leaves out."""
    from vrenderer_pathtracer_amd import scenes
    drop = DEVICE_VARIANTS[variant] if variant else ()
    return {k: v for k, v in scenes.torus_knot(*KNOT).items() if k not in drop}


def device_scene(scene, variant=None) -> dict:
    """The odd-shaped maps of `scene`, no mesh: the test builds it on the device."""
    sc = dict(make_case(f"S_odd_{scene}"), mesh_flat=None, name=f"device {scene} {variant}")
    if variant in DEVICE_NAN_VARIANTS:
        sc["camera"] = dict(sc["camera"], origin=(0.0, 0.0, FAR_CAMERA_Z))
    return sc


def render_on(sc, flat):
    """(accum, rgba8, depth8) of the oracle on a scene with the mesh `flat`."""
    return _render(dict(sc, mesh_flat=flat))


def check_device_variant(scene, variant) -> int:
    """The NaN condition on a host build of the variant's mesh; returns the NaN pixel count."""
    from vrenderer_pathtracer_amd import build_flat
    accum = render_on(device_scene(scene, variant), build_flat(device_mesh(variant), max_leaf_tris=LEAF))[0]
    n_px, n_nan = region(accum)[..., 0].size, int(nan_pixels(accum).sum())
    if variant in DEVICE_NAN_VARIANTS:
        assert MIN_NAN * n_px <= n_nan <= MAX_NAN * n_px, f"{scene} {variant}: {n_nan} of {n_px} pixels hold a NaN"
        assert not np.isnan(region(accum)[..., 3]).any()
    else:
        assert n_nan == 0, f"{scene} {variant}: {n_nan} pixels hold a NaN"
    assert np.any(region(accum)[..., :3] != 0)
    return n_nan
