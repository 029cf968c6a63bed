"""What the shading cases (tests/shading_cases.py) pin, from the oracle and
tests/flag_lattice.py alone: no GPU, no reference.

A case with odd-shaped maps is worth its GPU time only if a kernel with a
wrong idea of a map's size would render it differently.  That is measured
here on the oracle: each S_ and U_ case is rendered with its maps' sizes
mangled (width and height exchanged, the first map's size given to the others,
every size rounded down to a power of two) and the mutant must change at least
1 % of the rendered pixels.  The X_ cases that make NaNs must make them on 1 %
to 5 % of the pixels: enough to pin the NaN paths, few enough that the rest of
the image still compares bit for bit.  And the cases together must reach the
kernels the shading code is compiled into.
"""
import numpy as np
import pytest

import flag_lattice as fl
import ref_cases as rc
import shading_cases as sh


def test_case_set_shape():
    assert (sh.W, sh.H) == (rc.W, rc.H) == (64, 48) and sh.TIMES == rc.times_of("S_odd_C3")
    assert set(rc.SHADING_CASES) <= set(sh.CASES) and not set(rc.SHADING_CASES) & set(sh.ORACLE_ONLY)
    assert set(sh.NAN_CASES) <= set(sh.ORACLE_ONLY)
    for name, s in sh.SHAPES.items():
        sizes = list(s["tex"]) + [s["hdr"]]
        assert len(set(s["tex"])) == 3, name
        for w, h in s["tex"]:                       # non-square and no pair of powers of two, or a single texel
            assert (w, h) == (1, 1) or (w != h and (w & (w - 1) or h & (h - 1))), (name, w, h)
        assert all(w * h <= 38 * 101 for w, h in sizes)
    assert (1, 1) in sh.SHAPES["odd"]["tex"]
    assert any(w == 1 and h > 1 for w, h in sh.SHAPES["tall"]["tex"]) and sh.SHAPES["tall"]["hdr"][0] == 1
    assert sh.SHAPES["dot"]["hdr"] == (1, 1)
    maps = sh.maps_of("odd")
    assert maps["tex_normal"][..., 2].min() >= 0.6
    assert all(maps[k].shape == (h, w, 4) for k, (w, h) in zip(sh.TEX_KEYS, sh.SHAPES["odd"]["tex"]))
    half = sh.maps_of("half", "nmap_half")["tex_normal"]
    assert int((half[..., :3] == 0.5).all(-1).sum()) == 1


def test_inputs_are_what_the_names_say(native):
    uv = sh.mesh_of("uv3")["uvs"]
    assert uv.min() < -0.9 and uv.max() > 1.8 and np.isfinite(uv).all()
    assert not sh.mesh_of("tan0")["tangents"].any()
    for kind, key in (("tan0_third", "tangents"), ("nrm0_third", "normals")):
        a, plain = sh.mesh_of(kind)[key], sh.mesh_of("plain")[key]
        zero = ~a[:, :3].any(-1) & plain[:, :3].any(-1)
        assert 0.2 < zero.sum() / plain[:, :3].any(-1).sum() < 0.5, kind
    huge = np.abs(sh.mesh_of("uv_huge")["uvs"])
    assert huge.max() * 6 > 2.0 ** 31 and np.isfinite(huge).all()        # dim * u saturates f2i from a side of 6 up
    bad = sh.mesh_of("uv_nonfinite")["uvs"]
    assert np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any()
    n = sh.mesh_of("nrm0_tris")["normals"]
    v = sh.mesh_of("nrm0_tris")["verts"]
    real = v[:, 0].view(np.uint32) != 0x80000000                          # not a leaf terminator slot
    assert 0.10 < (~n[real][:, :3].any(-1)).mean() < 0.15                 # one triangle in eight
    m = sh.maps_of("tall", "texels01")
    for key in ("tex_diffuse", "tex_specular", "hdr"):
        assert (m[key][..., :3] == 0).all(-1).any(), key
        assert (m[key][..., :3] == (65504 if key == "hdr" else 1)).all(-1).any(), key
    assert np.isposinf(sh.maps_of("odd", "hdr_inf")["hdr"][..., :3]).any()


@pytest.mark.parametrize("name", list(sh.CASES))
def test_case_conditions_hold_on_the_oracle(oracle, native, name):
    """The mutant condition (S_, U_), the NaN share (the NaN cases), no NaN at
    all (every other case), and no black image."""
    sh.check_case(name)
    if name in sh.SHAPE_CASES:
        print(f"{name}: pixels of {sh.W * sh.H} a mutant changes: {sh.mutant_counts(name)}")
    if name in sh.ORACLE_ONLY:
        print(f"{name}: NaN share {sh.nan_share(name):.4f}")


def test_every_map_of_every_set_is_pinned_on_its_own(oracle, native):
    """The three asserted mutants change all maps at once.  One map's own
    width and height exchanged must show too, in some case of its set -- not
    in every case: under the HDRI every example-sphere hit reads one texel,
    and a one-column map's address there is the same either way."""
    n_px = sh.W * sh.H
    for set_name in ("odd", "tall", "dot"):
        s = sh.SHAPES[set_name]
        best = {}
        for name in [n for n in sh.SHAPE_CASES if sh.CASES[n]["shapes"] == set_name]:
            for m, n in sh.mutant_counts(name).items():
                if m.startswith("swap:"):
                    best[m[5:]] = max(best.get(m[5:], 0), n)
        for key, (w, h) in zip(sh.MAP_KEYS, list(s["tex"]) + [s["hdr"]]):
            if w != h:
                assert best.get(key, 0) >= sh.MIN_MUTANT * n_px, (set_name, key, best)


def test_mutants_are_mutants():
    """A mutant keeps every texel buffer's leading bytes and changes a size."""
    sc = sh.make_case("S_odd_C3")
    ms = sh.mutants(sc)
    assert set(ms) == {"swap", "first", "pow2"} | {f"swap:{k}" for k in ("tex_diffuse", "tex_normal", "hdr")}
    for name, m in ms.items():
        changed = [k for k in sh.MAP_KEYS if m[k] is not sc[k]]
        assert changed, name
        for k in changed:
            a, b = np.asarray(sc[k]).reshape(-1), np.asarray(m[k]).reshape(-1)
            n = min(len(a), len(b))
            assert m[k].shape[:2] != sc[k].shape[:2] and a[:n].tobytes() == b[:n].tobytes(), (name, k)
    assert ms["swap"]["tex_diffuse"].shape == (38, 101, 4) and ms["pow2"]["hdr"].shape == (32, 16, 4)
    assert all(ms["first"][k].shape == (101, 38, 4) for k in sh.TEX_KEYS)
    # a scene that reads no second map has no `first` mutant; the BRDF view reads neither colour nor specular map
    assert "first" not in sh.mutants(sh.make_case("S_odd_C2D"))
    assert sh.maps_read(sh.make_case("S_odd_C3B")) == ("tex_normal", "hdr")


def test_cases_reach_the_kernels_shading_is_compiled_into():
    """From the cases' flags alone, through the restatement of build_params
    and launch_scene in tests/flag_lattice.py."""
    reached = {}
    for name in sh.CASES:
        for strict in (False, True):
            reached.setdefault(sh.kernel_of(name, strict), set()).add(name)
    for target in ("spec_c3",) + fl.CLASSES + ("generic_strict",):
        assert reached.get(target), f"no shading case reaches {target}"
    # every kind of case on the exact specialisation and on a class kernel; every scene in strict mode
    for kind in ("S_", "U_", "D_", "V_", "X_"):
        assert any(n.startswith(kind) for n in reached["spec_c3"]), kind
        assert any(n.startswith(kind) for t in fl.CLASSES for n in reached[t]), kind
    assert reached["generic_strict"] == set(sh.CASES)
    # Mesh + example sphere: the generic kernel has a branch for such a flag word, but build_params never forms one
    # (it drops the mesh bit while the example sphere is on; test_flag_lattice.py).  The C3X cases are those
    # combinations: rendered here, by the HDRI sphere kernel.
    raw = lambda c: sum(1 << i for i, b in enumerate(c) if b)           # noqa: E731
    both = [n for n in sh.CASES if sh.CASES[n]["scene"] == "C3X"]
    assert len(both) == 3 and "generic_mesh_example" not in reached
    assert {fl.dispatch(raw(sh.combo_of(sh.make_case(n)))) for n in both} == {"generic_mesh_example"}
    assert {sh.kernel_of(n) for n in both} == {"cls_hdri_sphere"}
    # the NaN cases: the exact specialisation and a class kernel
    assert {sh.kernel_of(n) for n in sh.NAN_CASES} >= {"spec_c3", "cls_hdri_mesh"}


@pytest.mark.parametrize("variant", list(sh.DEVICE_VARIANTS))
@pytest.mark.parametrize("scene", sh.DEVICE_SCENES)
def test_device_mesh_variants_on_a_host_build(oracle, native, scene, variant):
    """A mesh without normals, tangents or uvs (zeros on the device-mesh path),
    built on the host: which variant makes NaNs, and on how much of the image."""
    n = sh.check_device_variant(scene, variant)
    print(f"{scene} {variant}: NaN share {n / (sh.W * sh.H):.4f}")
    assert (n > 0) == (variant in sh.DEVICE_NAN_VARIANTS)
