"""Mesh simplification on the device (octfusion_amd.simplify.simplify, csrc/ofx_simplify.hip), timed with HIP events
next to marching cubes on the same lattices: one R = 256 sphere and a batch of 8, cells = 64 and 128.

Per workload: the whole call (cluster launches, the one readback of the kept counts, extraction), and the split of
the cluster launches over their five stages -- keys, vertex sort, incidence sort, solve, face pass.  The split comes
from ofx_simplify_cluster's `stages` argument: the first k stages are launched and timed for k = 1 .. 5 (no readback),
and a stage's time is the difference of two medians.  Also the face counts and, for one shape, the OBJ sizes before
and after.

    python tools/simplify_probe.py --out profiles/mesh/simplify_probe.json [--size 256 --reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

import mc_oracle as M
from octfusion_amd import _lib, mesh, simplify

STAGES = ('keys', 'vertex_sort', 'incidence_sort', 'solve', 'face_pass')

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--batches', default='1,8')
ap.add_argument('--cells', default='64,128')
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device('cuda:0')
_lib.require_device()
R = args.size
assert _lib.lib().ofx_simplify_stages() == len(STAGES)


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


def spread(us):
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us))


rows = []
field = torch.from_numpy(M.sphere(R, r=0.6)).to(dev)
for B in [int(b) for b in args.batches.split(',')]:
    x = field.unsqueeze(0).repeat(B, 1, 1, 1).contiguous()
    meshes = mesh.marching_cubes(x)
    nv = [int(v.shape[0]) for v, _ in meshes]
    nf = [int(f.shape[0]) for _, f in meshes]
    cat_v, cat_f = mesh._cat(meshes)
    for _ in range(2):
        mesh.marching_cubes(x)
    torch.cuda.synchronize()
    us_mc, _ = timed(lambda: mesh.marching_cubes(x), args.reps)
    for cells in [int(c) for c in args.cells.split(',')]:
        for _ in range(3):                                         # warm-up: code loading, allocator
            out = simplify.simplify(meshes, cells=cells)
        torch.cuda.synchronize()
        us_all, out = timed(lambda: simplify.simplify(meshes, cells=cells), args.reps)
        prefix = []
        for k in range(1, len(STAGES) + 1):
            run = lambda: simplify._simplify_group(cat_v, cat_f, nv, nf, 0, cells, None, 1e-3, stages=k)
            run()
            torch.cuda.synchronize()
            prefix.append(statistics.median(timed(run, args.reps)[0]))
        split = {name: prefix[k] - (prefix[k - 1] if k else 0.0) for k, name in enumerate(STAGES)}
        row = dict(B=B, R=R, cells=cells, V=sum(nv), F=sum(nf), out_V=sum(int(v.shape[0]) for v, _ in out),
                   out_F=sum(int(f.shape[0]) for _, f in out), simplify=spread(us_all), marching_cubes=spread(us_mc),
                   cluster_launches_median_us=prefix[-1], stage_median_us=split)
        if B == 1:
            with tempfile.TemporaryDirectory() as td:
                mesh.write_obj(os.path.join(td, 'full.obj'), *meshes[0])
                mesh.write_obj(os.path.join(td, 'simple.obj'), *out[0])
                row['obj_bytes_full'] = os.path.getsize(os.path.join(td, 'full.obj'))
                row['obj_bytes_simple'] = os.path.getsize(os.path.join(td, 'simple.obj'))
        rows.append(row)
        print(json.dumps(row), flush=True)
res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
