"""The octree voxel mesh on the device (octfusion_amd.voxmesh.octree_mesh, csrc/ofx_voxmesh.hip), timed with HIP
events around the whole call (mask fill, count, the count readback, emit), warmed, on the bench's shell-6 octree at
B = 8 and on the shell-8 depth-8 octree at B = 1; welded and unwelded.

``--host`` instead times the reference's loop on this machine's CPU (no GPU needed): ``_voxel2mesh`` of the reference
tree on the depth-6 grid of one shell-6 shape, which is what export_octree runs per shape.

    python tools/voxmesh_probe.py --out profiles/mesh/voxmesh_probe.json
    python tools/voxmesh_probe.py --host
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from octfusion_amd import synthetic

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--host', action='store_true')
args = ap.parse_args()
torch.set_grad_enabled(False)


def shell6_grid():
    """The depth-6 grid of one shell-6 shape (all children of the occupied depth-5 cells), on the host."""
    s = synthetic.shell6_split(1)[0]
    occ5 = torch.zeros(32, 32, 32)
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                occ5[dx::2, dy::2, dz::2] = (s[4 * dx + 2 * dy + dz] > 0).float()
    return occ5.repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2).numpy()


if args.host:
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import refenv
    refenv.setup()
    from models.networks.diffusion_networks.ldm_diffusion_util import _voxel2mesh
    g = shell6_grid()
    t = time.perf_counter()
    v, f, _ = _voxel2mesh(g, 0.4)
    dt = time.perf_counter() - t
    print(json.dumps(dict(host_voxel2mesh_s=dt, R=64, occupied=int(g.sum()), quads=len(f) // 2)))
    sys.exit(0)

from octfusion_amd import _lib, voxmesh
from octfusion_amd.octree import split2octree_large, split2octree_small

dev = torch.device('cuda:0')
_lib.require_device()


def timed(fn, reps):
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return us, out


oc6 = split2octree_small(synthetic.shell6_split(8).to(dev), 6, 4)
one = split2octree_small(synthetic.shell6_split(1, jitter=False).to(dev), 6, 4)
x, y, z, _ = one.xyzb(6)
oc8 = split2octree_large(one, synthetic.shell8_split_large(x.cpu(), y.cpu(), z.cpu()).to(dev), 6)
rows = []
for name, oc, depth in (('shell6_B8', oc6, 6), ('shell8_B1', oc8, 8)):
    for weld in (True, False):
        for _ in range(3):
            voxmesh.octree_mesh(oc, depth, weld=weld)
        torch.cuda.synchronize()
        us, out = timed(lambda: voxmesh.octree_mesh(oc, depth, weld=weld), args.reps)
        V = sum(int(v.shape[0]) for v, _ in out)
        F = sum(int(f.shape[0]) for _, f in out)
        mask = oc.batch_size * (1 << (3 * depth)) // 8
        row = dict(octree=name, depth=depth, B=oc.batch_size, weld=weld, nodes=int(oc.nnum[depth]), verts=V, faces=F,
                   mask_bytes=mask, output_bytes=12 * (V + F), us_median=statistics.median(us), us_min=min(us))
        rows.append(row)
        print(json.dumps(row), flush=True)
res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
