"""Winding numbers on the device (octfusion_amd.mesh_query.winding_number, csrc/ofx_winding.hip) on the level-set
shell of tools/mesh2sdf_probe.py (the marching-cubes shell at 0.015 around icosphere(5), about 10^5 triangles):

    lattice  the --lattice^3 (128) lattice points of mesh_to_sdf, made on the device
    random   --points (10^6) points uniform in [-1, 1]^3

each exact (beta = 0) and with the far field at beta 2 and 3 on grids of 8^3 and 16^3 bins (16 is what the automatic
rule gives this shell).  Timed with HIP events around the public call, after a warm-up, median of --reps (every call
ends in a host read, so the events bracket finished work).  The work the far field leaves is counted by the kernel
itself (ofx_mesh_winding_set_counters, a separate untimed call): bins that were far for a whole wave, triangles
staged, (query, triangle) pairs summed against brute force (points x triangles), dipoles taken.  The far field's
largest difference from the exact values and the occupancies it flips are measured on the same points.

    python tools/winding_probe.py --out profiles/winding/winding_probe.json
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
from octfusion_amd import _lib, mesh, mesh2sdf, mesh_query

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--points', type=int, default=1000000)
ap.add_argument('--lattice', type=int, default=128, help='lattice the shell is extracted from and queried on')
ap.add_argument('--level', type=float, default=0.015)
ap.add_argument('--sub', type=int, default=5, help='icosphere subdivisions')
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')


def timed(fn, reps):
    out = fn()                                               # warm-up: code loading, allocator
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


def counted(fn):
    words = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.call('ofx_mesh_winding_set_counters', _lib.ptr(words))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.call('ofx_mesh_winding_set_counters', None)
    return [int(w) for w in words.cpu()]


V, F = O.icosphere(args.sub, (0.0, 0.0, 0.0), 0.8)
ico = (torch.from_numpy(V.astype(np.float32)).to(dev), torch.from_numpy(F).to(dev))
u0 = mesh2sdf.mesh_to_sdf([ico], args.lattice, signed=False)
shell = mesh.largest_component(mesh.marching_cubes(u0, args.level, bbmin=-1, bbmax=1))[0]
shell = (shell[0].contiguous(), shell[1].to(torch.int32).contiguous())
nf = int(shell[1].shape[0])

S = args.lattice
ax = ((2.0 * torch.arange(S, dtype=torch.float64, device=dev)) / S - 1.0).float()
lattice = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), dim=-1).reshape(-1, 3).contiguous()
gen = torch.Generator(device=dev).manual_seed(0)
cloud = (torch.rand(args.points, 3, device=dev, generator=gen) * 2.0 - 1.0).contiguous()

rows = []
for what, pts in (('%d^3 lattice points' % S, lattice), ('%d random points' % args.points, cloud)):
    n = int(pts.shape[0])
    exact = None
    for bins, beta in ((0, 0.0), (8, 2.0), (8, 3.0), (16, 2.0), (16, 3.0)):
        def fn():
            return mesh_query.winding_number([shell], [pts], beta=beta, bins=bins)[0]
        w, t, m = timed(fn, args.reps)
        far_bins, staged, pairs, dipoles = counted(fn)
        waves = -(-n // 64)
        row = dict(workload=what, mode='exact' if beta == 0 else 'far', bins=bins, beta=beta, points=n, faces=nf,
                   us=t, us_min=m, ns_per_point=1e3 * t / n, pairs_summed=pairs, pairs_brute_force=n * nf,
                   pairs_share=pairs / (n * nf), triangles_staged_per_wave=staged / waves,
                   far_bins_per_wave=far_bins / waves, dipoles_per_point=dipoles / n,
                   pairs_per_s=pairs / (t * 1e-6), inside=int((w > 0.5).sum()))
        if beta == 0:
            exact = w
        else:
            row.update(max_error=float((w.double() - exact.double()).abs().max()),
                       occupancy_flips=int(((w > 0.5) != (exact > 0.5)).sum()),
                       speedup=[r for r in rows if r['workload'] == what and r['mode'] == 'exact'][0]['us'] / t)
        rows.append(row)
        print(json.dumps(row), flush=True)

res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, level=args.level, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
