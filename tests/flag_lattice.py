"""The scene-flag lattice: every combination of the eight scene flags.

One recipe, shared by the generator (tests/golden/gen_ref_golden.py --flags,
which renders the 256 combinations with the reference compiled for the host
and stores digests in tests/golden/ref_flags.npz) and by
tests/test_flag_lattice.py (which renders them with the oracle and, over both
traversal modes and three launch kinds, with the HIP kernels).

A combination is the tuple (cornell, example, view_brdf, mesh, brdf, tex_d,
tex_n, tex_s) of 0/1.  Five of the flags follow an upload (mesh, BRDF table,
the three maps): the *upload set*; three are set per launch (Cornell box,
example sphere, BRDF view): the *toggles*.  The HDR map is always loaded, so
every combination without the Cornell box is a legal HDRI scene.

The last part restates, in Python, how the library turns a combination and
the strict-traversal switch into the launch's flag word
(vrhip_render.cpp build_params) and the flag word into a kernel
(vr_kernel.hip launch_scene and, for a render-service session, launch_service,
which repeats its three mesh comparisons; vr_kernel.hpp feature_class).  It is
a reading of those functions, used to name the kernel family in failure
messages and to check that the lattice reaches every dispatch target.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import ref_cases as rc
from ref_cases import input_digests                     # noqa: F401  (part of this module's interface)

W, H = 32, 32                     # 2 x 2 tiles: more than one tile row and column
TIMES = [12345, 13354]
FLAGS = ("cornell", "example", "view_brdf", "mesh", "brdf", "tex_d", "tex_n", "tex_s")
TOGGLES = FLAGS[:3]
UPLOADS = FLAGS[3:]
_TEX_KEYS = {"tex_d": "tex_diffuse", "tex_n": "tex_normal", "tex_s": "tex_specular"}


def combos():
    """The 256 combinations, in itertools.product order."""
    return list(itertools.product((0, 1), repeat=len(FLAGS)))


def name_of(combo) -> str:
    """cornell+mesh+tex_d; the combination with no flag set is `hdri`."""
    return "+".join(f for f, b in zip(FLAGS, combo) if b) or "hdri"


def toggles(combo):
    return tuple(combo[:3])


def upload_set(combo):
    return tuple(combo[3:])


def upload_name(uset) -> str:
    return "+".join(f for f, b in zip(UPLOADS, uset) if b) or "none"


def upload_sets(mesh="shallow"):
    """The 32 upload sets; with the deep mesh the 16 that load it."""
    sets = list(itertools.product((0, 1), repeat=len(UPLOADS)))
    return sets if mesh == "shallow" else [u for u in sets if u[0]]


def combos_of(uset):
    """The 8 combinations of an upload set, in combos() order."""
    return [t + tuple(uset) for t in itertools.product((0, 1), repeat=len(TOGGLES))]


@functools.lru_cache(maxsize=None)
def _inputs():
    from vrenderer_pathtracer_amd import scenes
    tex = scenes.procedural_textures(n=32)
    return dict(camera=scenes.default_camera(), hdr=scenes.procedural_hdr(w=64, h=32), brdf=scenes.synthetic_merl(),
                **{k: tex[k] for k in _TEX_KEYS.values()})


@functools.lru_cache(maxsize=None)
def mesh_of(kind):
    """shallow: the flat mesh stored in the sbvh fixture (no builder involved);
    deep: the one-triangle-per-leaf knot, deeper than 15 levels (24-entry stacks)."""
    if kind == "shallow":
        fx = rc.load_family("sbvh")
        return {k: np.array(fx[f"C2_sbvh/mesh_{k}"]) for k in ("bvh", "verts", "normals", "tangents", "uvs")}
    if kind == "deep":
        from vrenderer_pathtracer_amd import build_flat, scenes
        return build_flat(scenes.torus_knot(100, 50), max_leaf_tris=1)
    raise ValueError(kind)


def scene_of(combo, mesh="shallow") -> dict:
    """The scene dict pyoracle.render and scenes.load_into take."""
    cornell, example, view_brdf, has_mesh, has_brdf = combo[:5]
    inp = _inputs()
    sc = dict(camera=inp["camera"], fresnel_coef=0.1, fresnel_pow=3.0, width=W, height=H, time=TIMES[0],
              cornell=bool(cornell), example_sphere=bool(example), view_brdf=bool(view_brdf), hdr=inp["hdr"],
              name=name_of(combo))
    if has_mesh:
        sc["mesh_flat"] = mesh_of(mesh)
    if has_brdf:
        sc["brdf"] = inp["brdf"]
    for flag, key in _TEX_KEYS.items():
        if combo[FLAGS.index(flag)]:
            sc[key] = inp[key]
    return sc


def masked_depth(depth, saturated):
    """A depth image with the pixels zeroed on which it is not comparable with
    a host build of the reference: those whose saturating byte (the oracle's,
    the kernels') is zero, where the host build wraps."""
    return np.where(saturated[..., :1] != 0, depth, 0).astype(np.uint8)


# ---- the library's dispatch, restated ---------------------------------------------
# vr_params.hpp:33-41
F_CORNELL, F_EXAMPLE, F_VIEW_BRDF, F_MESH, F_BRDF, F_TEX_DIFF, F_TEX_NORM, F_TEX_SPEC, F_STRICT = (1 << i for i in range(9))
_BITS = dict(zip(FLAGS, (F_CORNELL, F_EXAMPLE, F_VIEW_BRDF, F_MESH, F_BRDF, F_TEX_DIFF, F_TEX_NORM, F_TEX_SPEC)))
_CLASS_GEOM = F_CORNELL | F_MESH
# launch_scene's equality tests (vr_kernel.hpp kFeat*)
EXACT = {F_CORNELL | F_MESH: "spec_c2", F_CORNELL | F_EXAMPLE: "spec_c1", F_MESH: "spec_c5",
         F_MESH | F_TEX_DIFF | F_TEX_NORM | F_TEX_SPEC: "spec_c3", F_EXAMPLE | F_VIEW_BRDF | F_BRDF: "spec_c4"}
CLASSES = ("cls_cornell_mesh", "cls_hdri_mesh", "cls_cornell_sphere", "cls_hdri_sphere")


def flag_word(combo, strict=False) -> int:
    """build_params: every flag as set, except that the mesh bit is dropped
    while the example sphere is on (the reference ignores the mesh then)."""
    f = sum(_BITS[n] for n, b in zip(FLAGS, combo) if b)
    if f & F_EXAMPLE:
        f &= ~F_MESH
    return f | (F_STRICT if strict else 0)


def dispatch(word) -> str:
    """launch_scene, launch_class and feature_class on a flag word."""
    if word in EXACT:
        return EXACT[word]
    if word & F_STRICT:
        return "generic_strict"
    geom = word & _CLASS_GEOM
    if geom & F_MESH:
        if word & F_EXAMPLE:
            return "generic_mesh_example"
        return "cls_cornell_mesh" if geom & F_CORNELL else "cls_hdri_mesh"
    return "cls_cornell_sphere" if geom & F_CORNELL else "cls_hdri_sphere"


def kernel_of(combo, strict=False) -> str:
    return dispatch(flag_word(combo, strict))
