"""Point -> mesh queries on the device (octfusion_amd.mesh_query, csrc/ofx_meshquery.hip) on the level-set shell of
tools/mesh2sdf_probe.py (the marching-cubes shell at 0.015 around icosphere(5), about 10^5 triangles):

    queries     closest_point of --queries points, half uniform in the shell's bounding box, half surface samples
                jittered by N(0, 0.01); unsigned and signed, with and without the closest point
    mesh_error  mesh_error(shell, simplify(shell, cells=64), 100000): both directions, one call
    lattice     for orientation, mesh_to_sdf(S=128, signed=False) on the same mesh in the same session

Timed with HIP events around each public call, after warm-up, median of --reps (every call ends in a host read, so the
events bracket finished work).  The work the culling leaves is counted by the kernel itself
(ofx_mesh_query_set_counters, a separate untimed call): bins searched, triangles staged and triangles evaluated per
wave of 64 queries, against brute force (queries x triangles).

The split of a call into its kernels (tb_init / tb_bound / tb_bin<1, 2> / scan / tb_key / sort / mq_dist / mq_sign) comes from a
kernel trace taken in a run of its own (--trace-only runs the signed 'both' query once so that the trace is short):
    rocprofv3 --kernel-trace --stats -d profiles/meshquery/trace -- python tools/meshquery_probe.py --trace-only

    python tools/meshquery_probe.py --out profiles/meshquery/meshquery_probe.json
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
from octfusion_amd import _lib, mesh, mesh2sdf, mesh_query, metrics, simplify

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--queries', type=int, default=1000000)
ap.add_argument('--samples', type=int, default=100000, help='mesh_error samples per side')
ap.add_argument('--size', type=int, default=128, help='lattice of the shell and of the orientation figure')
ap.add_argument('--level', type=float, default=0.015)
ap.add_argument('--sub', type=int, default=5, help='icosphere subdivisions')
ap.add_argument('--trace-only', action='store_true', help='one untimed signed query of both sets (for a kernel trace)')
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
    _lib.call('ofx_mesh_query_set_counters', _lib.ptr(words))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.call('ofx_mesh_query_set_counters', None)
    return [int(w) for w in words.cpu()[:3]]


V, F = O.icosphere(args.sub, (0.0, 0.0, 0.0), 0.8)
ico = (torch.from_numpy(V.astype(np.float32)).to(dev), torch.from_numpy(F).to(dev))
u0 = mesh2sdf.mesh_to_sdf([ico], args.size, signed=False)
shell = mesh.largest_component(mesh.marching_cubes(u0, args.level, bbmin=-1, bbmax=1))[0]
nf = int(shell[1].shape[0])
lo, hi = shell[0].min(0).values, shell[0].max(0).values
gen = torch.Generator(device=dev).manual_seed(0)
half = args.queries // 2
uniform = lo + (hi - lo) * torch.rand(half, 3, device=dev, generator=gen)
near = metrics.sample_surface([shell], n=args.queries - half, seed=0, normalize=False)[0]
near = near + 0.01 * torch.randn(near.shape, device=dev, generator=gen)
sets = {'uniform in the box': uniform.contiguous(), 'surface + N(0, 0.01)': near.contiguous(),
        'both': torch.cat([uniform, near]).contiguous()}

if args.trace_only:
    mesh_query.closest_point([shell], [sets['both']], signed=True)
    torch.cuda.synchronize()
    sys.exit(0)

rows = []
for name, q in sets.items():
    n = int(q.shape[0])
    for signed, want_point in ((False, True), (False, False), (True, True)):
        _, t, m = timed(lambda: mesh_query.closest_point([shell], [q], signed=signed, want_point=want_point),
                        args.reps)
        row = dict(workload='queries', queries=name, n=n, faces=nf, signed=signed, point=want_point, us=t, us_min=m,
                   queries_per_s=n / (t * 1e-6), ns_per_query=1e3 * t / n)
        if not signed and want_point:
            bins, staged, evaluated = counted(lambda: mesh_query.closest_point([shell], [q]))
            waves = -(-n // 64)
            row.update(waves=waves, bins_searched=bins, triangles_staged=staged, triangles_evaluated=evaluated,
                       pairs_evaluated=64 * evaluated, pairs_brute_force=n * nf,
                       staged_per_wave=staged / waves, evaluated_per_wave=evaluated / waves)
        rows.append(row)
        print(json.dumps(row), flush=True)

small = simplify.simplify([shell], cells=64)[0]
err, t, m = timed(lambda: mesh_query.mesh_error(shell, small, args.samples), args.reps)
bins, staged, evaluated = counted(lambda: mesh_query.mesh_error(shell, small, args.samples))
row = dict(workload='mesh_error', faces_a=nf, faces_b=int(small[1].shape[0]), samples=args.samples, us=t, us_min=m,
           result=err, triangles_evaluated=evaluated, pairs_evaluated=64 * evaluated,
           pairs_brute_force=args.samples * (nf + int(small[1].shape[0])))
rows.append(row)
print(json.dumps(row), flush=True)

_, t, m = timed(lambda: mesh2sdf.mesh_to_sdf([shell], args.size, signed=False), args.reps)
row = dict(workload='lattice', S=args.size, points=args.size ** 3, faces=nf, us=t, us_min=m,
           ns_per_point=1e3 * t / args.size ** 3)
rows.append(row)
print(json.dumps(row), flush=True)

res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, level=args.level, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
