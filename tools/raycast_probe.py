"""Ray casts on the device (octfusion_amd.raycast, csrc/ofx_raycast.hip) on the level-set shell of
tools/mesh2sdf_probe.py (the marching-cubes shell at 0.015 around icosphere(5), about 10^5 triangles):

    views    ray_images of the shell from the 20 FID views at --size (299) squared pixels: camera rays in 8 x 8 tiles,
             not sorted; and the cast alone (ray_cast(coherent=True) on the same rays, without the normal maps)
    random   ray_cast of --rays (10^6) rays from random points of the bounding sphere towards random points of the
             ball of half its radius: incoherent, sorted by the entry
    scan     virtual_scan from the 20 views at 128 squared

Timed with HIP events around each public call, after warm-up, median of --reps (every call ends in a host read, so the
events bracket finished work).  The work the culling leaves is counted by the kernel itself
(ofx_ray_cast_set_counters, a separate untimed call): bins visited, triangles staged and (ray, triangle) pairs
evaluated, against brute force (rays x triangles).

The split of a call into its kernels comes from a kernel trace taken in a run of its own (--trace-only casts the view
rays once so that the trace is short):
    rocprofv3 --kernel-trace --stats -d profiles/raycast/trace -- python tools/raycast_probe.py --trace-only

    python tools/raycast_probe.py --out profiles/raycast/raycast_probe.json
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
from octfusion_amd import _lib, mesh, mesh2sdf, raycast, render

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--rays', type=int, default=1000000)
ap.add_argument('--size', type=int, default=299, help='pixels per side of a view')
ap.add_argument('--lattice', type=int, default=128, help='lattice the shell is extracted from')
ap.add_argument('--level', type=float, default=0.015)
ap.add_argument('--sub', type=int, default=5, help='icosphere subdivisions')
ap.add_argument('--trace-only', action='store_true', help='one untimed cast of the view rays (for a kernel trace)')
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')


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


def counted(fn):
    words = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.call('ofx_ray_cast_set_counters', _lib.ptr(words))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.call('ofx_ray_cast_set_counters', None)
    return [int(w) for w in words.cpu()[:3]]


V, F = O.icosphere(args.sub, (0.0, 0.0, 0.0), 0.8)
ico = (torch.from_numpy(V.astype(np.float32)).to(dev), torch.from_numpy(F).to(dev))
u0 = mesh2sdf.mesh_to_sdf([ico], args.lattice, signed=False)
shell = mesh.largest_component(mesh.marching_cubes(u0, args.level, bbmin=-1, bbmax=1))[0]
shell = (shell[0].contiguous(), shell[1].to(torch.int32).contiguous())
nf = int(shell[1].shape[0])
unit = (raycast._unit_frame(shell[0]), shell[1])              # what ray_images casts against
poses = render.fid_poses()
view_org, view_dir, _, _ = raycast._view_rays(poses, args.size)

if args.trace_only:
    raycast.ray_cast([unit], [view_org], [view_dir], coherent=True)
    torch.cuda.synchronize()
    sys.exit(0)

rows = []


def record(row, fn_counted, n):
    bins, staged, pairs = counted(fn_counted)
    waves = -(-n // 64)
    row.update(rays=n, faces=nf, waves=waves, bins_visited=bins, triangles_staged=staged, pairs_evaluated=pairs,
               pairs_brute_force=n * nf, bins_per_wave=bins / waves, staged_per_wave=staged / waves,
               pairs_per_ray=pairs / n, rays_per_s=n / (row['us'] * 1e-6), ns_per_ray=1e3 * row['us'] / n)
    rows.append(row)
    print(json.dumps(row), flush=True)


n_view = int(view_org.shape[0])
img, t, m = timed(lambda: raycast.ray_images([shell], size=args.size), args.reps)
record(dict(workload='ray_images, 20 views at %d^2' % args.size, us=t, us_min=m,
            hits=int((img['face'] >= 0).sum())), lambda: raycast.ray_images([shell], size=args.size), n_view)
for bins in (0, 8):
    out, t, m = timed(lambda: raycast.ray_cast([unit], [view_org], [view_dir], coherent=True, bins=bins), args.reps)
    record(dict(workload='ray_cast of the same rays, coherent, bins=%d' % bins, us=t, us_min=m,
                hits=int((out[0][1] >= 0).sum())),
           lambda: raycast.ray_cast([unit], [view_org], [view_dir], coherent=True, bins=bins), n_view)
out, t, m = timed(lambda: raycast.ray_cast([unit], [view_org], [view_dir]), args.reps)
record(dict(workload='ray_cast of the same rays, sorted by the entry', us=t, us_min=m,
            hits=int((out[0][1] >= 0).sum())), lambda: raycast.ray_cast([unit], [view_org], [view_dir]), n_view)

gen = torch.Generator(device=dev).manual_seed(0)
centre = (shell[0].min(0).values + shell[0].max(0).values) * 0.5
radius = (shell[0] - centre).norm(dim=1).max()
a = torch.randn(args.rays, 3, device=dev, generator=gen)
org = (centre + radius * a / a.norm(dim=1, keepdim=True)).contiguous()
b = torch.randn(args.rays, 3, device=dev, generator=gen)
b = b / b.norm(dim=1, keepdim=True) * torch.rand(args.rays, 1, device=dev, generator=gen).pow(1.0 / 3.0)
dirs = (centre + 0.5 * radius * b - org).contiguous()
out, t, m = timed(lambda: raycast.ray_cast([shell], [org], [dirs]), args.reps)
record(dict(workload='ray_cast, random rays from the bounding sphere', us=t, us_min=m,
            hits=int((out[0][1] >= 0).sum())), lambda: raycast.ray_cast([shell], [org], [dirs]), args.rays)

scan, t, m = timed(lambda: raycast.virtual_scan([shell], poses, size=128), args.reps)
record(dict(workload='virtual_scan, 20 views at 128^2', us=t, us_min=m, points=int(scan[0][0].shape[0])),
       lambda: raycast.virtual_scan([shell], poses, size=128), 20 * 128 * 128)

res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, level=args.level, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
