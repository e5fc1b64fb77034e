"""Golden vectors of the reference's voxel mesher (_voxel2mesh, models/networks/diffusion_networks/
ldm_diffusion_util.py:353-446; what export_octree runs on every generated octree) -> tests/golden/g_voxmesh.pt.

CPU only, through refenv.py.  Seeded grids: R = 2, 4, 8 random at fill 0.5, an R = 8 checkerboard and a sparse R = 16,
all binary 0 / 1 at the threshold voxel2mesh passes on (0.4), plus one R = 4 grid of float values (none equal to its
threshold).  Recorded per case: the grid, the threshold, the vertices as float32 (the float64 values are exact in it:
corner * 2 / R - 1) and the faces as int32, both in the reference's order.

    python tests/golden/make_voxmesh_golden.py
"""
import os

import numpy as np
import torch

import refenv

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'g_voxmesh.pt')


def grids():
    rng = np.random.default_rng(2025)
    out = []
    for R in (2, 4, 8):
        out.append(('random%d' % R, (rng.random((R, R, R)) < 0.5).astype(np.float32), 0.4))
    out.append(('checker8', (np.indices((8, 8, 8)).sum(0) % 2).astype(np.float32), 0.4))
    out.append(('sparse16', (rng.random((16, 16, 16)) < 0.01).astype(np.float32), 0.4))
    f = rng.normal(0.3, 1.0, (4, 4, 4)).astype(np.float32)
    thr = 0.25
    assert not (f == np.float32(thr)).any() and not (f.astype(np.float64) == thr).any()
    out.append(('float4', f, thr))
    return out


def main():
    refenv.setup()
    from models.networks.diffusion_networks.ldm_diffusion_util import _voxel2mesh
    g = {}
    for name, grid, thr in grids():
        verts, faces, _ = _voxel2mesh(grid, thr)
        v32 = verts.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), verts), name            # nothing lost in fp32
        g[name] = dict(grid=torch.from_numpy(grid), threshold=float(thr), verts=torch.from_numpy(v32),
                       faces=torch.from_numpy(faces.astype(np.int32)))
        print('%-10s R=%-3d quads=%d' % (name, grid.shape[0], len(faces) // 2))
    torch.save(g, OUT)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) < 256 * 1024


if __name__ == '__main__':
    main()
