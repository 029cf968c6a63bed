"""The trees the device builders emit, the refit of each, and the renders on
them (which read the fp16 node rows and the triangle paths that no export
shows) equal the digests recorded in tests/golden/devmesh_digests.json."""
import json
import os

import pytest

import device_mesh_cases as cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "devmesh_digests.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def renderers(native):
    rs = cases.digest_renderers()
    yield rs
    for r in rs.values():
        r.cleanUp()


def test_every_recorded_case_is_compared():
    assert set(RECORDED) == {f"{b}-{c}" for b in cases.BUILDERS for c in cases.digest_cases()}


@pytest.mark.parametrize("cid", list(cases.digest_cases()))
@pytest.mark.parametrize("builder", cases.BUILDERS)
def test_trees_and_renders_equal_recorded_digests(renderers, builder, cid):
    make, leaf = cases.digest_cases()[cid]
    assert cases.case_digests(renderers, builder, make(), leaf) == RECORDED[f"{builder}-{cid}"]
