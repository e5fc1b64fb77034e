"""Mesh -> SDF lattice on the device (octfusion_amd.mesh2sdf, csrc/ofx_mesh2sdf.hip) at the real size, S = 128, batch
1 and 8, on two inputs: (i) icosphere(5), 20480 triangles, and (ii) the level-set mesh the repair itself extracts from
(i) (``compute(fix=True)``'s second pass: the triangle count of a real marching-cubes shell).

Timed with HIP events around each public call, after warm-up, median of --reps (every call ends in a host read, so
the events bracket finished work):
    unsigned   mesh_to_sdf(signed=False): bin + distance
    signed     mesh_to_sdf(signed=True):  bin + distance + sign      (sign = signed - unsigned)
    mc         mesh.marching_cubes(u, level, -1, 1)
    cc         mesh.largest_component
    compute    compute(fix=True) end to end (batch 1)
The split of a call into its kernels (ms_init / ms_bin<0> / ms_bin<1> / scan / ms_dist / ms_sign) comes from a kernel
trace taken in a run of its own (--trace-only runs each workload once so that the trace is short):
    rocprofv3 --kernel-trace --stats -d profiles/mesh2sdf/trace -- python tools/mesh2sdf_probe.py --trace-only
The work the culling leaves is counted by the kernel itself (ofx_mesh_sdf_set_counters, a separate untimed call):
bins searched, triangles staged and triangles evaluated per brick of 64 lattice points.

    python tools/mesh2sdf_probe.py --out profiles/mesh2sdf/mesh2sdf_probe.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import mesh2sdf_oracle as O
from octfusion_amd import _lib, mesh, mesh2sdf

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--size', type=int, default=128)
ap.add_argument('--level', type=float, default=0.015)
ap.add_argument('--batches', default='1,8')
ap.add_argument('--sub', type=int, default=5, help='icosphere subdivisions')
ap.add_argument('--trace-only', action='store_true', help='one untimed pass per workload (for a kernel trace)')
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')
S = args.size


def timed(fn, reps):
    for _ in range(2):
        out = fn()                                           # warm-up: code loading, allocator
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return out, statistics.median(us), min(us)


def counted(meshes):
    words = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.call('ofx_mesh_sdf_set_counters', _lib.ptr(words))
    try:
        mesh2sdf.mesh_to_sdf(meshes, S, signed=False)
        torch.cuda.synchronize()
    finally:
        _lib.call('ofx_mesh_sdf_set_counters', None)
    return [int(w) for w in words.cpu()[:3]]


V, F = O.icosphere(args.sub, (0.0, 0.0, 0.0), 0.8)
ico = (torch.from_numpy(V.astype(np.float32)).to(dev), torch.from_numpy(F).to(dev))
u0 = mesh2sdf.mesh_to_sdf([ico], S, signed=False)
shell = mesh.largest_component(mesh.marching_cubes(u0, args.level, bbmin=-1, bbmax=1))[0]
inputs = {'icosphere(%d)' % args.sub: ico, 'level-set shell': shell}

rows = []
for name, m in inputs.items():
    for B in [int(b) for b in args.batches.split(',')]:
        meshes = [m] * B
        if args.trace_only:
            u = mesh2sdf.mesh_to_sdf(meshes, S, signed=True)
            torch.cuda.synchronize()
            continue
        u, t_u, m_u = timed(lambda: mesh2sdf.mesh_to_sdf(meshes, S, signed=False), args.reps)
        _, t_s, m_s = timed(lambda: mesh2sdf.mesh_to_sdf(meshes, S, signed=True), args.reps)
        mc, t_mc, _ = timed(lambda: mesh.marching_cubes(u, args.level, bbmin=-1, bbmax=1), args.reps)
        _, t_cc, _ = timed(lambda: mesh.largest_component(mc), args.reps)
        bins, staged, evaluated = counted(meshes)
        bricks = B * ((S + 3) // 4) ** 3
        nf = int(m[1].shape[0])
        row = dict(input=name, B=B, S=S, faces=nf, unsigned_us=t_u, unsigned_us_min=m_u, signed_us=t_s,
                   signed_us_min=m_s, sign_us=t_s - t_u, mc_us=t_mc, cc_us=t_cc,
                   mc_faces=sum(int(f.shape[0]) for _, f in mc), bricks=bricks, bins_searched=bins,
                   triangles_staged=staged, triangles_evaluated=evaluated, pairs_evaluated=64 * evaluated,
                   pairs_brute_force=B * S ** 3 * nf, staged_per_brick=staged / bricks,
                   evaluated_per_brick=evaluated / bricks)
        rows.append(row)
        print(json.dumps(row), flush=True)
if not args.trace_only:
    _, t_c, m_c = timed(lambda: mesh2sdf.compute(ico[0], ico[1], S, fix=True, level=args.level), args.reps)
    row = dict(input='compute(fix=True) on icosphere(%d)' % args.sub, B=1, S=S, compute_us=t_c, compute_us_min=m_c)
    rows.append(row)
    print(json.dumps(row), flush=True)
res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, level=args.level, rows=rows)
if args.out and not args.trace_only:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
