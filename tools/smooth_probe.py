"""Mesh smoothing on the device (octfusion_amd.mesh_smooth, csrc/ofx_meshsmooth.hip) on generate-sized meshes: the
marching-cubes mesh of a rippled sphere on a 128^3 and a 256^3 lattice (--lattices).

Per mesh, with HIP events around the calls and a synchronisation, after a warm-up, the median of --reps:
  * the adjacency build (ofx_mesh_adjacency without the corner lists, buffers allocated outside the window);
  * one half-step, uniform and cotangent weights: (ofx_mesh_smooth with --steps Laplacian iterations - the same call
    with 0 iterations) / --steps, so the set-up the two calls share drops out; that set-up is reported too;
  * the bytes a half-step must move at least -- the state read and written once (48 V), the rules (4 V), the row
    offsets (8 V), the neighbour indices (4 per entry) and, for cotangent weights, the weights (8 per entry) -- the rate
    that makes, its share of 8 TB/s, and beside it the bytes the gather asks the caches for (24 per entry);
  * ``smooth(iterations=10)`` as a user calls it (Taubin: 20 half-steps), allocation and the host read included.

    python tools/smooth_probe.py --out profiles/smooth/smooth_probe.json
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

from octfusion_amd import _lib, mesh, mesh_check, mesh_smooth
from octfusion_amd._lib import call, ptr, stream

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--steps', type=int, default=100, help='half-steps in the timed call')
ap.add_argument('--lattices', type=int, nargs='+', default=[128, 256])
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')
PEAK = 8.0e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return statistics.median(us), min(us), max(us)


def rippled_sphere(R):
    g = (torch.arange(R, device=dev, dtype=torch.float32) * (1.8 / R) - 0.9)
    x, y, z = torch.meshgrid(g, g, g, indexing='ij')
    return (torch.sqrt(x * x + y * y + z * z) - 0.6 + 0.02 * torch.sin(9 * x) * torch.sin(7 * y) * torch.sin(8 * z))[None]


rows = []
for R in args.lattices:
    m = mesh.marching_cubes(rippled_sphere(R).contiguous())[0]
    m = (m[0].contiguous(), m[1].to(torch.int32).contiguous())
    g = mesh_check._gather([m], 'probe')
    V, F = g['nv'][0], g['nf'][0]
    margs = mesh_check._mesh_args(g)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    row_off = torch.empty(V + 1, dtype=torch.int64, device=dev)
    nbr = torch.empty(6 * F, dtype=torch.int32, device=dev)
    vflags = torch.empty(V, dtype=torch.int32, device=dev)
    ws = mesh_check._ws(g, 'ofx_mesh_adjacency_ws_bytes', 'probe')
    t_adj = timed(lambda: call('ofx_mesh_adjacency', *margs, V, F, ptr(row_off), ptr(nbr), ptr(vflags), None, None,
                               ptr(ws), ptr(status), stream()), args.reps)
    entries = int(row_off[-1])
    degree = (row_off[1:] - row_off[:-1])
    row = dict(lattice=R, vertices=V, faces=F, entries=entries, mean_degree=entries / V, max_degree=int(degree.max()),
               adjacency_us=t_adj[0], adjacency_us_min_max=t_adj[1:])
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    for name, wmode in (('uniform', 0), ('cot', 1)):
        ws = mesh_check._ws(g, 'ofx_mesh_smooth_ws_bytes', 'probe', wmode)

        def run(iters):
            call('ofx_mesh_smooth', *margs, V, F, wmode, 0, 0.5, 0.0, iters, ptr(out), None, ptr(ws), ptr(status),
                 stream())
        t0 = timed(lambda: run(0), args.reps)
        t1 = timed(lambda: run(args.steps), args.reps)
        step = (t1[0] - t0[0]) / args.steps
        need = 48 * V + 4 * V + 8 * V + (4 + 8 * wmode) * entries
        row[name] = dict(setup_us=t0[0], setup_us_min_max=t0[1:], call_us=t1[0], call_us_min_max=t1[1:],
                         half_step_us=step, bytes_needed=need, gather_bytes=24 * entries,
                         needed_GBps=need / step * 1e-3, share_of_8TBps=need / (step * 1e-6) / PEAK)
    torch.cuda.synchronize()
    wall = []
    for _ in range(args.reps + 1):
        t = time.perf_counter()
        mesh_smooth.smooth([m], iterations=10)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t))
    row['smooth_10_taubin_ms'] = statistics.median(wall[1:])
    rows.append(row)
    print(json.dumps(row), flush=True)

res = dict(device=torch.cuda.get_device_name(0), host=os.uname().nodename, reps=args.reps, steps=args.steps, rows=rows)
print(json.dumps(dict(device=res['device'], host=res['host'])))
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
