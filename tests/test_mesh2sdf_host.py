"""Host side of octfusion_amd/mesh2sdf.py that needs no device: the OBJ reader, normalize, shape names, the parser."""
import numpy as np
import pytest

from octfusion_amd import mesh2sdf as M

OBJ = """# a unit square as one quad, a pentagon, and two triangles with every token form
mtllib none.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0.5 0.5
vn 0 0 1
g plane
f 1/1/1 2/1/1 3/1/1 4/1/1
v 2 0.5 0
f 1 2 5 3 4
f -5//1 -4//1 -3//1
f 1/1 3/1 -2/1

s off
"""


def test_read_mesh(tmp_path):
    p = tmp_path / 'm.obj'
    p.write_text(OBJ)
    v, f = M.read_mesh(str(p))
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert v.shape == (5, 3) and np.array_equal(v[4], [2, 0.5, 0])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3],                    # the quad, fanned around its first vertex
                          [0, 1, 4], [0, 4, 2], [0, 2, 3],         # the pentagon
                          [0, 1, 2],                               # -5 -4 -3 of five vertices
                          [0, 2, 3]]                               # -2 of five vertices
    empty = tmp_path / 'e.obj'
    empty.write_text('v 0 0 0\n')
    v, f = M.read_mesh(str(empty))
    assert v.shape == (1, 3) and f.shape == (0, 3)


def test_normalize():
    rng = np.random.RandomState(0)
    v = rng.rand(50, 3) * [3.0, 1.0, 0.5] + [10.0, -2.0, 0.25]
    out, bbmin, bbmax = M.normalize(v)
    # tools/repair_mesh.py:143-147
    center = (v.min(0) + v.max(0)) * 0.5
    scale = 2.0 * 0.8 / (v.max(0) - v.min(0)).max()
    assert np.array_equal(out, (v - center) * scale)
    assert np.array_equal(bbmin, v.min(0)) and np.array_equal(bbmax, v.max(0))
    assert np.isclose(np.abs(out).max(), 0.8) and np.allclose(out.min(0) + out.max(0), 0)
    assert np.isclose(np.abs(M.normalize(v, 0.5)[0]).max(), 0.5)
    with pytest.raises(ValueError):
        M.normalize(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        M.normalize(np.zeros((0, 3)))


def test_shape_name_and_parser():
    assert M.shape_name('/data/ShapeNetCore.v1/02691156/abc123/model.obj') == '02691156/abc123'
    assert M.shape_name('meshes/chair.obj') == 'chair'
    assert M.shape_name('model.obj') == 'model'
    a = M.parser().parse_args(['--input', 'a.obj', 'b.obj', '--out', 'root'])
    assert a.input == ['a.obj', 'b.obj'] and a.size == 128 and a.level == 0.015 and a.points == 100000
    assert not a.pointcloud and not a.no_fix and a.seed == 0
    assert M.MESH_SCALE == 0.8 and M.SHAPE_SCALE == 0.5
