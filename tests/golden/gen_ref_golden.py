"""Regenerate tests/golden/ref_*.npz from the reference compiled for the host.

Run by hand where a reference checkout exists (oracle/ref/README.md):

    python tests/golden/gen_ref_golden.py [--check] [case ...]

    python tests/golden/gen_ref_golden.py --flags [--check]

With --check nothing is written: the fresh arrays are compared with the
committed files, key by key.  --flags renders the 256 scene-flag combinations
of tests/flag_lattice.py instead of the cases and writes ref_flags.npz, which
holds digests, not images (oracle/ref/README.md has the layout).

Every case of tests/ref_cases.py is rendered by the `zero`-initialised
reference in both libm modes, by the `pattern`-initialised one (pixels that
differ read uninitialised memory: the `undefined` mask) and by the UBSan
build (float-cast-overflow; its reports are kept as file:line).  The
generator prints, per case: pixels compared, the `undefined` count, the UBSan
locations and the pixels differing from the oracle, and refuses to write a
fixture that breaks a condition below.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), TESTS]

import pyoracle as po                        # noqa: E402
import ref_cases as rc                       # noqa: E402

MAX_FILE = os.path.getsize(os.path.join(HERE, "golden_images.npz"))
MAX_UNDEFINED = 0.05
# the one conversion CUDA saturates and x86 wraps: the depth byte in render()
DEPTH_BYTE = re.compile(r"\bunsigned\s+char\s+depth\b")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sbvh_flat(builds, workdir):
    """The sliver mesh through the reference's SBVH builder, flattened by
    vRendererHIP::flattenSBVH over the stand-in tree of tests/stubs."""
    import pathlib
    from test_adapter import _build_driver, _read_flat, _write_mesh
    from vrenderer_pathtracer_amd import build as vbuild
    vbuild.build()
    mesh = rc.sliver_mesh()
    mp, tp, fp = (os.path.join(workdir, n) for n in ("mesh.bin", "tree.bin", "flat.bin"))
    _write_mesh(mp, mesh)
    subprocess.run([builds["sbvh_driver"], mp, tp], check=True, capture_output=True)
    raw = open(tp, "rb").read()
    n_nodes, n_refs = np.frombuffer(raw[:8], np.uint32)
    refs = np.frombuffer(raw[8 + 36 * int(n_nodes):], np.uint32)
    assert len(refs) == n_refs
    n_split = int((np.bincount(refs, minlength=len(mesh["tris"])) > 1).sum())
    exe = _build_driver(pathlib.Path(workdir))
    subprocess.run([exe, fp, mp, "--flatten", tp], check=True, capture_output=True)
    flat, _ = _read_flat(open(fp, "rb").read())
    return flat, dict(sbvh_nodes=int(n_nodes), sbvh_refs=int(n_refs), triangles=len(mesh["tris"]),
                      triangles_in_several_leaves=n_split)


def ubsan_locations(stderr, src_dir):
    """file:line of every UBSan report, and whether each is the depth byte."""
    locs, other = set(), []
    for line in stderr.splitlines():
        m = re.match(r"(.*?):(\d+):\d+: runtime error", line)
        if not m:
            continue
        path, ln = m.group(1), int(m.group(2))
        locs.add(f"{os.path.basename(path)}:{ln}")
        text = open(path, errors="replace").read().splitlines()[ln - 1]
        if not DEPTH_BYTE.search(text):
            other.append(f"{os.path.basename(path)}:{ln}")
    return sorted(locs), other


def generate(names, check=False):
    builds = po.build_reference()
    if builds is None:
        raise SystemExit("no reference checkout (set VRO_REFERENCE)")
    po.build()
    versions = po.ref_compiler_versions()
    fams = sorted({rc.CASES[n][0] for n in names})
    total_diff = 0
    for fam in fams:
        out = {}
        path = os.path.join(HERE, f"ref_{fam}.npz")
        fam_cases = [n for n in rc.CASES if rc.CASES[n][0] == fam]
        if not set(fam_cases) <= set(names):                 # partial regeneration keeps the other cases
            old = np.load(path)
            out.update({k: old[k] for k in old.files if k.split("/")[0] not in names})
        sbvh = None
        for name in [n for n in fam_cases if n in names]:
            with tempfile.TemporaryDirectory() as d:
                sc = rc.make_case(name)
                extra = {}
                if rc.CASES[name][1] == "sbvh":
                    if sbvh is None:
                        sbvh = sbvh_flat(builds, d)
                    sc["mesh_flat"], extra = sbvh
                    # no assertion on triangles_in_several_leaves: the reference builder duplicates
                    # no reference on any mesh tried (oracle/ref/README.md says why); the count is recorded
                    for k, a in sc["mesh_flat"].items():
                        out[f"{name}/mesh_{k}"] = a
                if rc.CASES[name][1] == "deep":
                    from vrenderer_pathtracer_amd import validate_flat
                    depth, _ = validate_flat(sc["mesh_flat"])
                    assert depth > 15, depth
                    extra["tree_depth"] = int(depth)
                if rc.CASES[name][1] == "stack":
                    from vrenderer_pathtracer_amd import validate_flat
                    depth, _ = validate_flat(sc["mesh_flat"])
                    assert depth == rc.CASES[name][2]["depth"], depth
                    extra["tree_depth"] = int(depth)
                    extra["max_stack"] = po.render(sc, frames=2, times=rc.times_of(name), libm=po.LIBM_PORTABLE,
                                                   count=True)[3]["max_stack"]
                    assert extra["max_stack"] == depth, extra        # the oracle's walk fills the stack the reference has
                times = rc.times_of(name)
                pa, pr, pd, _ = po.render_reference(builds["ref_portable_zero"], sc, times, d)
                ga, gr, _, _ = po.render_reference(builds["ref_glibc_zero"], sc, times, d)
                undefined = np.zeros(pa.shape[:2], bool)
                for libm, (za, zr, zd) in (("portable", (pa, pr, pd)), ("glibc", (ga, gr, None))):
                    qa, qr, qd, _ = po.render_reference(builds[f"ref_{libm}_pattern"], sc, times, d)
                    undefined |= (qa.view(np.uint32) != za.view(np.uint32)).any(-1) | (qr != zr).any(-1)
                    if zd is not None:
                        undefined |= (qd != zd).any(-1)
                ua, ur, ud, err = po.render_reference(builds["ref_portable_ubsan"], sc, times, d)
                assert np.array_equal(ua.view(np.uint32), pa.view(np.uint32)) and np.array_equal(ud, pd)
                locs, other = ubsan_locations(err, os.path.join(os.path.dirname(builds["ref_portable_zero"]), "src"))
            assert not other, f"{name}: UBSan reports outside the depth byte: {other}"
            n_undef = int(undefined.sum())
            if name in rc.MAY_BE_UNDEFINED:
                assert n_undef <= MAX_UNDEFINED * undefined.size, (name, n_undef)
            else:
                assert n_undef == 0, (name, n_undef)
            if name in rc.FULL_DEPTH:
                assert not locs, f"{name}: a full-depth case with UBSan reports {locs}"
            # against the oracle (reported; tests/test_reference_fixtures.py asserts it)
            h, w = (sc["height"] // 16) * 16, (sc["width"] // 16) * 16
            oa, orgba, od, _ = po.render(sc, frames=len(times), times=times, libm=po.LIBM_PORTABLE)
            oga, ogr, _, _ = po.render(sc, frames=len(times), times=times, libm=po.LIBM_GLIBC)
            ok = np.ones_like(undefined)             # the oracle defines what the reference leaves undefined as zero
            diff = ((oa.view(np.uint32) != pa.view(np.uint32)).any(-1) | (orgba != pr).any(-1) |
                    (oga.view(np.uint32) != ga.view(np.uint32)).any(-1) | (ogr != gr).any(-1)) & ok
            ddiff = (od != pd).any(-1) & ok & ((od[..., 0] != 0) | (name in rc.FULL_DEPTH))
            n_diff = int((diff | ddiff).sum())
            total_diff += n_diff
            print(f"{name:16s} pixels {h * w:5d}  undefined {n_undef:3d}  ubsan {locs}  differ from oracle {n_diff}"
                  + (f"  {extra}" if extra else ""))
            meta = dict(case=name, family=fam, recipe=rc.CASES[name][1], params=rc.CASES[name][2],
                        width=sc["width"], height=sc["height"], frames=len(times), times=times,
                        inputs=rc.input_digests(sc), ubsan=locs, compilers=versions, **extra)
            out[f"{name}/accum_portable"] = pa
            out[f"{name}/rgba_portable"] = pr
            out[f"{name}/depth_portable"] = pd
            out[f"{name}/accum_glibc_sha256"] = np.array(sha(ga))
            out[f"{name}/rgba_glibc_sha256"] = np.array(sha(gr))
            out[f"{name}/undefined"] = undefined
            out[f"{name}/meta"] = np.array(json.dumps(meta, sort_keys=True))
        if check:
            old = np.load(path)
            assert sorted(old.files) == sorted(out), f"{path}: keys differ"
            bad = [k for k in out if np.asarray(out[k]).tobytes() != old[k].tobytes() or np.asarray(out[k]).dtype != old[k].dtype]
            assert not bad, f"{path}: a fresh run differs in {bad}"
            print(f"  -> {os.path.relpath(path, REPO)} reproduced ({len(out)} arrays)")
            continue
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(f"  -> {os.path.relpath(path, REPO)}  {size} bytes")
        assert size <= MAX_FILE, f"{path} is larger than golden_images.npz ({MAX_FILE})"
    print("pixels differing from the oracle, all cases:", total_diff)


MIN_FLAG_PAIRS = 16          # of the 128 single-flag pairs of each flag, how many must differ
_ORACLE_LOCK = threading.Lock()   # the reference runs are processes; the oracle renders one scene at a time


def flags_point(builds, combo, workdir):
    """One lattice point through the five reference builds and both oracle modes."""
    import flag_lattice as fl
    name = fl.name_of(combo)
    sc = fl.scene_of(combo)
    times = fl.TIMES
    os.makedirs(workdir, exist_ok=True)
    pa, pr, pd, _ = po.render_reference(builds["ref_portable_zero"], sc, times, workdir)
    ga, gr, _, _ = po.render_reference(builds["ref_glibc_zero"], sc, times, workdir)
    undefined = np.zeros(pa.shape[:2], bool)
    for libm, (za, zr, zd) in (("portable", (pa, pr, pd)), ("glibc", (ga, gr, None))):
        qa, qr, qd, _ = po.render_reference(builds[f"ref_{libm}_pattern"], sc, times, workdir)
        undefined |= (qa.view(np.uint32) != za.view(np.uint32)).any(-1) | (qr != zr).any(-1)
        if zd is not None:
            undefined |= (qd != zd).any(-1)
    ua, ur, ud, err = po.render_reference(builds["ref_portable_ubsan"], sc, times, workdir)
    assert np.array_equal(ua.view(np.uint32), pa.view(np.uint32)) and np.array_equal(ud, pd), name
    locs, other = ubsan_locations(err, None)
    assert not other, f"{name}: UBSan reports outside the depth byte: {other}"
    with _ORACLE_LOCK:
        oa, orgba, od, _ = po.render(sc, frames=len(times), times=times, libm=po.LIBM_PORTABLE)
        oga, ogr, _, _ = po.render(sc, frames=len(times), times=times, libm=po.LIBM_GLIBC)
    diff = ((oa.view(np.uint32) != pa.view(np.uint32)).any(-1) | (orgba != pr).any(-1) |
            (oga.view(np.uint32) != ga.view(np.uint32)).any(-1) | (ogr != gr).any(-1) |
            ((od != pd).any(-1) & (od[..., 0] != 0)))
    assert np.any(pa[..., :3] != 0) and np.any(pr[..., :3] != 0), f"{name}: a black image"
    return dict(accum_portable=sha(pa), rgba_portable=sha(pr), depth_portable=sha(fl.masked_depth(pd, od)),
                accum_glibc=sha(ga), rgba_glibc=sha(gr), undefined=undefined, ubsan=locs,
                inputs=sha(json.dumps(rc.input_digests(sc), sort_keys=True).encode()),
                oracle=sha(oa), oracle_rgba=sha(orgba), differ=int(diff.sum()))


def generate_flags(check=False):
    """tests/golden/ref_flags.npz: per combination of tests/flag_lattice.py, digests
    of what the reference renders (256 float images do not fit the size cap)."""
    from concurrent.futures import ThreadPoolExecutor
    import flag_lattice as fl
    builds = po.build_reference()
    if builds is None:
        raise SystemExit("no reference checkout (set VRO_REFERENCE)")
    po.build()
    po.lib()
    combos = fl.combos()
    fl.scene_of(combos[-1])                          # the shared inputs, made once before the threads start
    with tempfile.TemporaryDirectory() as d:
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            pts = list(pool.map(lambda ic: flags_point(builds, ic[1], os.path.join(d, str(ic[0]))), enumerate(combos)))
    n_px = fl.W * fl.H
    counts = np.array([int(p["undefined"].sum()) for p in pts], np.int32)
    for combo, n in zip(combos, counts):
        c = dict(zip(fl.FLAGS, combo))
        may = not c["cornell"] and c["example"] and (c["tex_d"] or c["tex_n"] or c["tex_s"])
        assert n <= MAX_UNDEFINED * n_px, (fl.name_of(combo), int(n))
        assert may or n == 0, f"{fl.name_of(combo)}: {n} undefined pixels outside HDRI + example sphere + a map"
    index = {c: i for i, c in enumerate(combos)}
    pairs = {}                                       # per flag: (accumulations that differ, RGBA8 images that differ)
    for k, flag in enumerate(fl.FLAGS):
        off = [c for c in combos if not c[k]]
        pairs[flag] = tuple(sum(pts[index[c]][what] != pts[index[c[:k] + (1,) + c[k + 1:]]][what] for c in off)
                            for what in ("oracle", "oracle_rgba"))
        assert len(off) == 128 and min(pairs[flag]) >= MIN_FLAG_PAIRS, (flag, pairs[flag])
    masks, mask_index = [], []
    for p in pts:
        packed = np.packbits(p["undefined"].reshape(-1))
        for i, m in enumerate(masks):
            if np.array_equal(m, packed):
                break
        else:
            i = len(masks)
            masks.append(packed)
        mask_index.append(i)
    sc_all = fl.scene_of(combos[-1])
    arrays = {k: v for k, v in rc.input_digests(sc_all).items() if k != "scalars"}
    meta = dict(flags=list(fl.FLAGS), width=fl.W, height=fl.H, frames=len(fl.TIMES), times=fl.TIMES, inputs=arrays,
                ubsan=sorted({loc for p in pts for loc in p["ubsan"]}), compilers=po.ref_compiler_versions())
    out = {f"{k}_sha256": np.array([p[k] for p in pts]) for k in
           ("accum_portable", "rgba_portable", "depth_portable", "accum_glibc", "rgba_glibc", "inputs")}
    out["undefined_count"] = counts
    out["undefined_index"] = np.array(mask_index, np.int16)
    out["undefined_masks"] = np.stack(masks)
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    print(f"combinations {len(combos)}  distinct images {len({p['oracle'] for p in pts})} "
          f"(RGBA8 {len({p['oracle_rgba'] for p in pts})})  "
          f"undefined: max {int(counts.max())} of {n_px}, in {int((counts > 0).sum())} combinations, "
          f"{len(masks)} distinct masks  ubsan {meta['ubsan']}")
    print("single-flag pairs that differ, of 128 (accum, RGBA8):", pairs)
    print("pixels differing from the oracle, all combinations:", sum(p["differ"] for p in pts))
    path = os.path.join(HERE, "ref_flags.npz")
    if check:
        old = np.load(path)
        assert sorted(old.files) == sorted(out), f"{path}: keys differ"
        bad = [k for k in out if np.asarray(out[k]).tobytes() != old[k].tobytes() or np.asarray(out[k]).dtype != old[k].dtype]
        assert not bad, f"{path}: a fresh run differs in {bad}"
        size = os.path.getsize(path)
        assert size <= MAX_FILE, f"{path} is larger than golden_images.npz ({MAX_FILE})"
        print(f"  -> {os.path.relpath(path, REPO)} reproduced ({len(out)} arrays, {size} bytes)")
        return
    with tempfile.TemporaryDirectory() as d:
        fresh = os.path.join(d, "ref_flags.npz")
        np.savez_compressed(fresh, **out)
        size = os.path.getsize(fresh)
        assert size <= MAX_FILE, f"ref_flags.npz would be larger than golden_images.npz ({size} > {MAX_FILE})"
        shutil.move(fresh, path)
    print(f"  -> {os.path.relpath(path, REPO)}  {size} bytes")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a not in ("--check", "--flags")]
    if "--flags" in sys.argv[1:]:
        generate_flags(check="--check" in sys.argv[1:])
    else:
        generate(args or list(rc.CASES), check="--check" in sys.argv[1:])
