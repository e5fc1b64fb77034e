"""The mesh checker on the device (octfusion_amd.mesh_check, csrc/ofx_meshcheck.hip) on a generate-sized mesh: the
marching-cubes shell at --level around icosphere(5) on a --lattice^3 (256) lattice, a few 10^5 triangles, and the same
mesh simplified to --cells cells (vertex clustering leaves non-manifold edges and folded faces behind).

Per mesh: the time of weld (both calls and the host read between them), of the topology call and of the
self-intersection call at the automatic grid, each with HIP events around the call and a synchronisation, after a
warm-up, median of --reps; the three counters of the pair search (ofx_mesh_selfx_set_counters, a separate untimed
call) beside F (F - 1) / 2; and the search's time for every bins in 1 .. 16, against what the automatic rule picks.

    python tools/meshcheck_probe.py --out profiles/meshcheck/meshcheck_probe.json
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
from octfusion_amd import _lib, mesh, mesh2sdf, mesh_check, simplify

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--lattice', type=int, default=256)
ap.add_argument('--level', type=float, default=0.015)
ap.add_argument('--sub', type=int, default=5, help='icosphere subdivisions')
ap.add_argument('--cells', type=int, default=64, help='cells of the simplified mesh')
ap.add_argument('--sweep-reps', type=int, default=2)
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')


def timed(fn, reps):
    out = fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return out, statistics.median(us)


def counted(fn):
    words = torch.zeros(3, dtype=torch.int64, device=dev)
    _lib.call('ofx_mesh_selfx_set_counters', _lib.ptr(words))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.call('ofx_mesh_selfx_set_counters', None)
    return [int(w) for w in words.cpu()]


def auto_bins(F):
    g = 1
    while g < 16 and 256 * g * g < F:
        g += 1
    return g


V, F = O.icosphere(args.sub, (0.0, 0.0, 0.0), 0.8)
ico = (torch.from_numpy(V.astype(np.float32)).to(dev), torch.from_numpy(F).to(dev))
u0 = mesh2sdf.mesh_to_sdf([ico], args.lattice, signed=False)
shell = mesh.largest_component(mesh.marching_cubes(u0, args.level, bbmin=-1, bbmax=1))[0]
shell = (shell[0].contiguous(), shell[1].to(torch.int32).contiguous())
del u0
small = simplify.simplify([shell], cells=args.cells)[0]
small = (small[0].contiguous(), small[1].to(torch.int32).contiguous())

rows = []
for what, m in (('marching cubes %d^3' % args.lattice, shell), ('simplified, %d cells' % args.cells, small)):
    g = mesh_check._gather([m], 'probe')
    nf, nv = g['nf'][0], g['nv'][0]
    report = mesh_check.check([m])[0]
    _, t_weld = timed(lambda: mesh_check._weld(g, 'probe'), args.reps)
    _, t_topo = timed(lambda: mesh_check._topology(g, 'probe', True), args.reps)
    _, t_selfx = timed(lambda: mesh_check._selfx(g, 0, 'probe'), args.reps)
    visited, staged, judged = counted(lambda: mesh_check._selfx(g, 0, 'probe'))
    waves = -(-nf // 64)
    sweep = {}
    for bins in range(1, 17):
        sweep[bins] = timed(lambda: mesh_check._selfx(g, bins, 'probe'), args.sweep_reps)[1]
    best = min(sweep, key=sweep.get)
    row = dict(mesh=what, vertices=nv, faces=nf, report=report, weld_us=t_weld, topology_us=t_topo,
               selfx_us=t_selfx, auto_bins=auto_bins(nf), bins_visited_per_wave=visited / waves,
               triangles_staged_per_wave=staged / waves, pairs_judged=judged, pairs_all=nf * (nf - 1) // 2,
               judged_share=judged / 2 / (nf * (nf - 1) // 2), staged_share=staged / (waves * nf),
               selfx_us_by_bins=sweep, best_bins=best, best_us=sweep[best], auto_over_best=sweep[auto_bins(nf)] / sweep[best])
    rows.append(row)
    print(json.dumps(row), flush=True)

res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, level=args.level, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
