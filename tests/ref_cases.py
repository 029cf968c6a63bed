"""The cases of the reference-rendered fixtures (tests/golden/ref_*.npz).

One recipe per case, shared by the generator (tests/golden/gen_ref_golden.py,
which renders them with the reference compiled for the host, oracle/ref/) and
by tests/test_reference_fixtures.py (which renders them with the oracle and
with the HIP kernels).  Only outputs are stored in the fixtures: a recipe
regenerates its inputs, and the SHA-256 of every input array is kept in the
fixture so that a change in a procedural input reports as input drift, not as
a parity failure.  The one stored input is the flat mesh of the two `sbvh`
cases, which only the reference's own builder can make.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = 64, 48
FEATURE_CLASSES = ["C2D", "C3D", "C2N", "C3B", "C1T", "C4D", "CB", "C3X"]     # test_gpu_classes without C5T

# the cases of tests/shading_cases.py that fit the fixture file's size cap: a shape set for each of spec_c3 and the four
# class kernels (two for spec_c3 and the HDRI sphere kernel), two uv, four attribute and two texel cases; the others
# are pinned to the oracle alone, like the X_ cases (tests/test_gpu_shading.py)
SHADING_CASES = ("S_odd_C3", "S_tall_C3B", "S_tall_C2N", "S_dot_C1T", "S_odd_C4D", "U_C3", "U_C2N", "D_tan0_C3B",
                 "D_nrm0_third_C3", "V_texels01_C3", "V_hdr_inf_C3", "S_tall_C3", "S_dot_C3X", "D_tan0_third_C2N")

# the launch scalars of tests/launch_scalar_cases.py on which the oracle's restatement (the uint32 wrap of the pixel
# seeds, the camera's operation order, pow at its edges) is checked against the reference itself: two times of 2^24
# and more on C2, three cameras and two Fresnel pairs on C3, and a single column of tiles
SCALAR_CASES = ("T_2p24p1_C2", "T_2p32m1_C2", "K_skewed_C3", "K_fov_10_C3", "K_up_C3", "F_0_0.5_C3", "F_1_64_C3",
                "I_16x64_C2")

# the comb of tests/stack_cases.py at the last depth of the 32-entry stack and of the 64-entry one, and its legged kind
STACK_CASES = (("C2", "comb", 30), ("C3", "comb", 30), ("C2", "comb", 62), ("C3", "comb", 62), ("C2", "legged", 62))

# name -> (family file, recipe, parameters)
CASES = {
    "C1": ("configs", "config", dict(cfg="C1", frames=3)),
    "C2": ("configs", "config", dict(cfg="C2")),
    "C3": ("configs", "config", dict(cfg="C3")),
    "C4": ("configs", "config", dict(cfg="C4")),
    "C2_100x70": ("configs", "config", dict(cfg="C2", width=100, height=70)),      # grid truncation
    **{n: ("classes", "class", dict(cls=n)) for n in FEATURE_CLASSES},
    "soup_C2_leaf3": ("soups", "soup", dict(cfg="C2", leaf=3)),
    "soup_C3_leaf5": ("soups", "soup", dict(cfg="C3", leaf=5)),
    "soup_C2_leaf16": ("soups", "soup", dict(cfg="C2", leaf=16)),
    "soup_C3_leaf40": ("soups", "soup", dict(cfg="C3", leaf=40)),
    "C2_deep": ("trees", "deep", dict(cfg="C2")),                                  # 24-entry-stack kernels
    "C3_deep": ("trees", "deep", dict(cfg="C3")),
    "C3_doubled": ("trees", "doubled", dict(cls="C3")),                            # equal-t ties, uvs outside [0,1]
    "C2D_doubled": ("trees", "doubled", dict(cls="C2D")),
    "C2_rotated": ("views", "rotated", dict(cfg="C2")),
    "C3_rotated": ("views", "rotated", dict(cfg="C3")),
    "C3_inside": ("views", "config", dict(cfg="C3", origin=(0.0, 0.0, 12.0), full_depth=True)),
    "C2_near": ("views", "config", dict(cfg="C2", origin=(0.0, 0.0, 20.0), full_depth=True)),
    "C2_sbvh": ("sbvh", "sbvh", dict(cfg="C2")),
    "C3_sbvh": ("sbvh", "sbvh", dict(cfg="C3")),
    # odd map shapes, wild uvs, zero attributes, extreme texels: recipes in tests/shading_cases.py
    **{n: ("shading", "shading", dict(case=n)) for n in SHADING_CASES},
    # time seeds, cameras, Fresnel pairs and an image shape: recipes in tests/launch_scalar_cases.py
    **{n: ("scalars", "scalars", dict(case=n)) for n in SCALAR_CASES},
    # trees that fill the 32- and the 64-entry stack to the last entry: recipes in tests/stack_cases.py
    **{f"{cfg}_{tree}{depth}": ("stacks", "stack", dict(cfg=cfg, tree=tree, depth=depth)) for cfg, tree, depth in STACK_CASES},
}
# cases in which no primary hit lies farther than the depth byte's range
# (150 units), so the depth image compares on every pixel
FULL_DEPTH = {"C4", "C3_inside", "C2_near"}
# cases in which the reference reads vHitData::m_normal before writing it
MAY_BE_UNDEFINED = {"C4D", "C3X", "S_odd_C4D", "S_dot_C3X"}
FAMILIES = sorted({v[0] for v in CASES.values()})


def times_of(name):
    if CASES[name][1] == "scalars":
        import launch_scalar_cases
        return launch_scalar_cases.ref_times(CASES[name][2]["case"])
    frames = CASES[name][2].get("frames", 2)
    return [12345 + 1009 * i for i in range(frames)]


def sliver_mesh() -> dict:
    """A cluster of small triangles crossed by long thin ones: the shape a
    spatial split exists for (a sliver's box spans the whole cluster)."""
    rng = np.random.default_rng(5)
    n_small, n_long = 360, 12
    c = rng.uniform(-25, 25, (n_small, 1, 3))
    small = c + rng.normal(0, 1.5, (n_small, 3, 3))
    a = rng.uniform(-30, 30, (n_long, 3))
    a[:, 0] = -38.0
    b = a + rng.normal(0, 6, (n_long, 3))
    b[:, 0] = 38.0
    long = np.stack([a, b, (a + b) / 2 + rng.normal(0, 0.6, (n_long, 3))], 1)
    P = np.concatenate([small, long]).reshape(-1, 3).astype(np.float32)
    n = len(P) // 3
    T = rng.normal(0, 1, (3 * n, 3))
    return dict(positions=P, normals=(T / np.linalg.norm(T, axis=1, keepdims=True)).astype(np.float32),
                tangents=np.tile([1, 0, 0], (3 * n, 1)).astype(np.float32),
                uvs=rng.uniform(0, 1, (3 * n, 2)).astype(np.float32),
                tris=np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))


def _rotated_camera(cam):
    o = np.array([30.0, 20.0, 130.0])
    d = -o / np.sqrt((o * o).sum())
    r = np.cross(d, [0.0, 1.0, 0.0])
    r = r / np.sqrt((r * r).sum())
    u = np.cross(r, d)
    f32 = lambda v: tuple(float(x) for x in v.astype(np.float32))
    return dict(cam, origin=f32(o), dir=f32(d), up=f32(u), right=f32(r), fov_scale=0.9)


def make_case(name, stored=None):
    """The scene dict of a case.  `stored`: the fixture's arrays (an NpzFile
    or dict) for the cases whose mesh is stored, None while generating."""
    from vrenderer_pathtracer_amd import build_flat, scenes
    fam, recipe, p = CASES[name]
    w, h = p.get("width", W), p.get("height", H)
    knot = (24, 12)
    if recipe == "config":
        sc = scenes.make_scene(p["cfg"], w, h, knot=knot)
        if "origin" in p:
            sc["camera"] = dict(sc["camera"], origin=p["origin"])
    elif recipe == "class":
        from test_gpu_classes import class_scene
        sc = class_scene(p["cls"], w, h)
        if sc.get("mesh_flat") is not None:
            sc["mesh_flat"] = scenes.knot_flat(*knot)
    elif recipe == "soup":
        from test_gpu_parity import _random_soup
        sc = scenes.make_scene(p["cfg"], w, h, knot=knot)
        leaf = p["leaf"]
        sc["mesh_flat"] = _random_soup(11 + leaf, 1500, leaf, cluster=20 if leaf > 8 else 1)
    elif recipe == "deep":
        sc = scenes.make_scene(p["cfg"], w, h, knot=knot)
        sc["mesh_flat"] = build_flat(scenes.torus_knot(100, 50), max_leaf_tris=1)
    elif recipe == "doubled":
        from test_gpu_classes import class_scene
        sc = class_scene(p["cls"], w, h) if p["cls"] != "C3" else scenes.make_scene("C3", w, h, knot=knot)
        m = scenes.torus_knot(*knot)
        m = dict(m, uvs=(m["uvs"] * np.float32(3) - np.float32(1)).astype(np.float32),
                 tris=np.concatenate([m["tris"], m["tris"]]))
        sc["mesh_flat"] = build_flat(m, max_leaf_tris=2)
    elif recipe == "rotated":
        sc = scenes.make_scene(p["cfg"], w, h, knot=knot)
        sc["camera"] = _rotated_camera(sc["camera"])
        sc.update(fresnel_coef=0.35, fresnel_pow=5.0)
    elif recipe == "sbvh":
        sc = scenes.make_scene(p["cfg"], w, h, knot=knot)
        sc["mesh_flat"] = None if stored is None else {k: np.array(stored[f"{name}/mesh_{k}"])
                                                       for k in ("bvh", "verts", "normals", "tangents", "uvs")}
    elif recipe == "shading":
        import shading_cases
        sc = shading_cases.make_case(p["case"])
    elif recipe == "scalars":
        import launch_scalar_cases
        sc = launch_scalar_cases.ref_scene(p["case"])
    elif recipe == "stack":
        import stack_cases
        sc = stack_cases.scene(stack_cases.tree(p["tree"], p["depth"]), p["cfg"], w, h)
    else:
        raise ValueError(recipe)
    sc["name"] = name
    return sc


def input_digests(sc) -> dict:
    """SHA-256 of every input of a scene: arrays as float32 bytes, the rest as JSON."""
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()
    out = {}
    for k in ("hdr", "tex_diffuse", "tex_normal", "tex_specular", "brdf"):
        if sc.get(k) is not None:
            out[k] = sha(sc[k])
    if sc.get("mesh_flat") is not None:
        for k in ("bvh", "verts", "normals", "tangents", "uvs"):
            out["mesh_" + k] = sha(sc["mesh_flat"][k])
    cam = {k: [float(np.float32(x)) for x in np.atleast_1d(v)] for k, v in sc["camera"].items()}
    scalars = dict(camera=cam, width=sc["width"], height=sc["height"], cornell=bool(sc.get("cornell")),
                   example_sphere=bool(sc.get("example_sphere")), view_brdf=bool(sc.get("view_brdf")),
                   fresnel_coef=float(np.float32(sc.get("fresnel_coef", 0.1))),
                   fresnel_pow=float(np.float32(sc.get("fresnel_pow", 3.0))))
    out["scalars"] = hashlib.sha256(json.dumps(scalars, sort_keys=True).encode()).hexdigest()
    return out


def load_family(fam):
    return np.load(os.path.join(GOLDEN, f"ref_{fam}.npz"))
