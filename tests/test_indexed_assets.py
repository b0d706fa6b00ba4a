"""Model.indexed_inputs(): the OBJ as an indexed mesh (one vertex record per distinct v/vt/vn triple of the faces, in
first-use order) for Renderer.upload_mesh_indexed.  Re-expanded it must be init_vertex_input's array (phong.rs:187-201,
Model.vertex_inputs) bit for bit -- normals normalised at fetch included."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "tests", "golden", "cube.obj")

# two quads as four faces whose shared triples come back in other corners, one triple used three times, one triple that
# differs from another in its normal only (a distinct vertex record), and an unnormalised normal
REUSE_OBJ = b"""v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 2 0.5 -1e-1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vn 0 0 3
vn 0.5 0.25 -2
f 1/1/1 2/2/1 3/3/1
f 3/3/1 4/4/1 1/1/1
f 2/2/1 5/3/2 3/3/1
f 3/3/2 2/2/1 1/1/1
f 5/3/2 3/3/2 2/2/2
"""


def _models():
    from f_renderer_amd.assets import Model
    return {"cube": Model(OBJ), "reuse": Model(data=REUSE_OBJ)}


@pytest.mark.parametrize("name", ["cube", "reuse"])
def test_indexed_inputs_expand_to_vertex_inputs(name):
    m = _models()[name]
    vertices, faces = m.indexed_inputs()
    assert vertices.dtype == np.float32 and faces.dtype == np.uint32
    assert vertices.shape == (vertices.shape[0], 8) and faces.shape == (m.faces_len(), 3)
    want = m.vertex_inputs()
    got = vertices[faces].reshape(m.faces_len(), 3, 8)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    triples = [t for f in m.faces for t in f]
    assert vertices.shape[0] == len(set(triples))
    assert vertices.shape[0] < 3 * m.faces_len()                      # something is shared
    # first-use order: vertex k is the k-th distinct triple met walking the faces
    order = list(dict.fromkeys(triples))
    np.testing.assert_array_equal(faces.reshape(-1), np.array([order.index(t) for t in triples], np.uint32))


def test_reuse_fixture_shares_in_other_corners():
    m = _models()["reuse"]
    vertices, faces = m.indexed_inputs()
    assert vertices.shape[0] == 7
    assert faces.tolist() == [[0, 1, 2], [2, 3, 0], [1, 4, 2], [5, 1, 0], [4, 5, 6]]
    assert not np.array_equal(vertices[2], vertices[5])              # same position and uv, another normal
    np.testing.assert_array_equal(vertices[0, 5:], np.array([0, 0, 1], np.float32))
