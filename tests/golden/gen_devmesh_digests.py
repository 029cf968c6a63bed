#!/usr/bin/env python3
"""Writes tests/golden/devmesh_digests.json: SHA-256 digests of what the two
device builders and the refit produce for the cases of
tests/device_mesh_cases.py digest_cases (needs the GPU).

  python tests/golden/gen_devmesh_digests.py [--out FILE]

Recorded from the library before the builders and the refit came to share
their emission stage (vr_devmesh.hip); regenerate only for an intended change
of the trees, and say so.  tests/test_gpu_devmesh_digests.py compares."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import device_mesh_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "devmesh_digests.json"))
    a = ap.parse_args()
    renderers = cases.digest_renderers()
    out = {}
    for builder in cases.BUILDERS:
        for cid, (make, leaf) in cases.digest_cases().items():
            out[f"{builder}-{cid}"] = cases.case_digests(renderers, builder, make(), leaf)
    for r in renderers.values():
        r.cleanUp()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {a.out}")


if __name__ == "__main__":
    main()
