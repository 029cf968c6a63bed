#!/bin/bash
# VGPRs / spills / scratch of the production path-kernel instantiations in a
# build_variants log (kernel-resource-usage remarks):
#   bash scripts/kres.sh variants/<name>.log
# With a second argument `radiance`: every instantiation of the radiance query
# kernel (vr_radiance*.hip) beside render_kernel of the same feature set:
#   bash scripts/kres.sh variants/<name>.log radiance
# With `surface`: every instantiation of the surface query kernel
# (vr_surface*.hip) in the same table:
#   bash scripts/kres.sh variants/<name>.log surface
# With `shade`: every instantiation of the surface-record radiance kernel
# (vr_shade*.hip) in the same table:
#   bash scripts/kres.sh variants/<name>.log shade
# With `probe`: every instantiation of the probe kernel (vr_probe*.hip) beside
# ray_radiance_kernel of the same feature set and stack size, and the two
# small kernels of vr_probe.hip:
#   bash scripts/kres.sh variants/<name>.log probe
# With `denoise`: the denoiser's kernels (vr_denoise.hip):
#   bash scripts/kres.sh variants/<name>.log denoise
# With `atlas`: the atlas and surface-at kernels (vr_atlas.hip):
#   bash scripts/kres.sh variants/<name>.log atlas
python3 - "$1" "$2" <<'PY'
import re, sys
recs, cur = {}, None
for line in open(sys.argv[1]):
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = recs.setdefault(m.group(1), {})
        continue
    m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
    if m and cur is not None and m.group(1) not in cur:
        cur[m.group(1)] = int(m.group(2))
if len(sys.argv) > 2 and sys.argv[2] == "denoise":
    cols = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print(f"{'kernel':24s} {'VGPRs':>5s} {'vspill':>6s} {'sspill':>6s} {'scratch':>7s} {'LDS':>6s} {'waves':>5s}")
    for name, r in recs.items():
        m = re.search(r"denoise_(\w+?)_kernel", name)
        if m:
            print(f"{'denoise_' + m.group(1) + '_kernel':24s} " + " ".join(f"{r.get(c, 0):{w}d}" for c, w in zip(cols, (5, 6, 6, 7, 6, 5))))
    sys.exit(0)
if len(sys.argv) > 2 and sys.argv[2] == "atlas":
    cols = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print(f"{'kernel':28s} {'VGPRs':>5s} {'vspill':>6s} {'sspill':>6s} {'scratch':>7s} {'LDS':>6s} {'waves':>5s}")
    for name, r in recs.items():
        m = re.search(r"\d+(prim_inverse_kernel|atlas_\w+?_kernel|surface_fill_kernel)(ILb([01]))?", name)
        if m:
            lab = m.group(1) + ({"0": "<at>", "1": "<atlas>"}.get(m.group(3), ""))
            print(f"{lab:28s} " + " ".join(f"{r.get(c, 0):{w}d}" for c, w in zip(cols, (5, 6, 6, 7, 6, 5))))
    sys.exit(0)
if len(sys.argv) > 2 and sys.argv[2] == "probe":
    CLS, ALL = 1 << 30, 511
    sets = [("class Cornell+mesh", CLS + 253, (16, 24, 32, 64)), ("class HDRI+mesh", CLS + 252, (16, 24, 32, 64)),
            ("generic (strict)", ALL, (16, 24, 32, 64)), ("class Cornell spheres", CLS + 247, (16,)),
            ("class HDRI spheres", CLS + 246, (16,))]
    cols = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print(f"{'kernel':44s} {'VGPRs':>5s} {'vspill':>6s} {'sspill':>6s} {'scratch':>7s} {'LDS':>6s} {'waves':>5s}")
    def row(lab, name):
        r = recs.get(name)
        if r is None:
            print(f"{lab:44s} (not in this build)")
        else:
            print(f"{lab:44s} " + " ".join(f"{r.get(c, 0):{w}d}" for c, w in zip(cols, (5, 6, 6, 7, 6, 5))))
    for lab, feat, stacks in sets:
        for st in stacks:
            row(f"ray_radiance_kernel<{st}> {lab}", f"_ZN2vr19ray_radiance_kernelILi{st}ELj{feat}EEEvNS_12RenderParamsENS_11RayRadianceE")
            row(f"  probe_sh_kernel<{st}> {lab}", f"_ZN2vr15probe_sh_kernelILi{st}ELj{feat}EEEvNS_12RenderParamsENS_7ProbeSHE")
    row("probe_sum_kernel", "_ZN2vr16probe_sum_kernelEPKfjmPf")
    row("sh_irradiance_kernel", "_ZN2vr20sh_irradiance_kernelENS_12SHIrradianceE")
    sys.exit(0)
QUERIES = {"radiance": ("ray_radiance_kernel", "RayRadiance"), "surface": ("ray_surface_kernel", "RaySurface"),
           "shade": ("surface_shade_kernel", "SurfaceShade")}
if len(sys.argv) > 2 and sys.argv[2] in QUERIES:
    query = QUERIES[sys.argv[2]]
    CLS, ALL = 1 << 30, 511
    sets = [("class Cornell+mesh", CLS + 253, (16, 24, 32, 64)), ("class HDRI+mesh", CLS + 252, (16, 24, 32, 64)),
            ("generic (strict)", ALL, (16, 24, 32, 64)), ("class Cornell spheres", CLS + 247, (16,)),
            ("class HDRI spheres", CLS + 246, (16,))]
    cols = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print(f"{'kernel':44s} {'VGPRs':>5s} {'vspill':>6s} {'sspill':>6s} {'scratch':>7s} {'LDS':>6s} {'waves':>5s}")
    def row(lab, name):
        r = recs.get(name)
        if r is None:
            print(f"{lab:44s} (not in this build)")
        else:
            print(f"{lab:44s} " + " ".join(f"{r.get(c, 0):{w}d}" for c, w in zip(cols, (5, 6, 6, 7, 6, 5))))
    for lab, feat, stacks in sets:
        row(f"render_kernel<16> {lab}", f"_ZN2vr13render_kernelILi16ELb0ELj{feat}EEEvNS_12RenderParamsE")
        for st in stacks:
            row(f"  {query[0]}<{st}> {lab}",
                f"_ZN2vr{len(query[0])}{query[0]}ILi{st}ELj{feat}EEEvNS_12RenderParamsENS_{len(query[1])}{query[1]}E")
    sys.exit(0)
E, INL, SML, SVC, SPA = 2147483648, 8192, 16384, 32768, 65536
C2, C3, C5 = E + 9, E + 232, E + 8
CLS_C, CLS_H = (1 << 30) + 253, (1 << 30) + 252
rows = [("C2 whole frame", "render_wave_kernel", 16, C2, 256), ("C2 one frame", "render_wave_kernel", 16, C2 + INL + SML, 256),
        ("C2 service", "render_service_kernel", 16, C2 + SVC, 256),
        ("C2 small shard", "render_wave_kernel", 16, C2 + SML, 256),
        ("C3 whole frame", "render_wave_kernel", 16, C3, 768), ("C3 shard", "render_wave_kernel", 16, C3, 256),
        ("C3 small shard", "render_wave_kernel", 16, C3 + SML, 256),
        ("C3 one frame", "render_wave_kernel", 16, C3 + INL + SML, 256), ("C3 service", "render_service_kernel", 16, C3 + SVC, 256),
        ("C3 sparse frame", "render_wave_kernel", 16, C3 + SPA, 768), ("C3 sparse service", "render_service_kernel", 16, C3 + SVC + SPA, 256),
        ("C5 whole frame", "render_wave_kernel", 24, C5, 768), ("C5 shard", "render_wave_kernel", 24, C5, 256),
        ("C5 small shard", "render_wave_kernel", 24, C5 + SML, 256),
        ("C5 one frame", "render_wave_kernel", 24, C5 + INL + SML, 256), ("C5 service", "render_service_kernel", 24, C5 + SVC, 256),
        ("C5 sparse frame", "render_wave_kernel", 24, C5 + SPA, 768), ("C5 sparse service", "render_service_kernel", 24, C5 + SVC + SPA, 256),
        ("class Cornell+mesh", "render_wave_kernel", 16, CLS_C, 768), ("class HDRI+mesh", "render_wave_kernel", 16, CLS_H, 768)]
print(f"{'kernel':22s} {'VGPRs':>5s} {'spill':>5s} {'scratch':>7s} {'waves':>5s}")
for lab, k, st, feat, bt in rows:
    name = f"_ZN2vr{len(k)}{k}ILi{st}ELj{feat}ELi{bt}EEEvNS_12RenderParamsE"
    r = recs.get(name)
    if r is None:
        print(f"{lab:22s} (not in this build)")
        continue
    print(f"{lab:22s} {r.get('VGPRs', 0):5d} {r.get('VGPRs Spill', 0):5d} {r.get('ScratchSize [bytes/lane]', 0):7d} "
          f"{r.get('Occupancy [waves/SIMD]', 0):5d}")
PY
