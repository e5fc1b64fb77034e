"""The largest-component clean on the device (octfusion_amd.mesh.largest_component, csrc/ofx_mesh_cc.hip), timed
with HIP events from the label launch to the end of the extraction (the kept-count readback included), next to
marching cubes alone on the same batch and to the host path it replaces: device -> host copy of one shape's mesh
plus the numpy / scipy oracle (tests/cc_oracle.py).

Algorithmic bytes of one clean: the face passes read 12 F each (check, hook, flag, keep, extract), the label passes
move 4 V each, the extraction reads 12 V + 12 F and writes the kept bytes.

Workloads: B = 8, R = 256 on a sphere, a torus and ``noisy(256, 4)`` (1.2 M components per shape).

    python tools/clean_probe.py --out profiles/mesh/clean_probe.json [--fields sphere --batch 8 --size 256]
    rocprofv3 --kernel-trace --stats -- python tools/clean_probe.py --once --fields noisy     # the per-kernel split
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import cc_oracle as C
import mc_oracle as M
from octfusion_amd import _lib, mesh

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--fields', default='sphere,torus,noisy')
ap.add_argument('--once', action='store_true', help='one warm-up and one clean per field, no host path (for a trace)')
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device('cuda:0')
_lib.require_device()
R, B = args.size, args.batch


def field(kind):
    f = {'sphere': lambda: M.sphere(R, r=0.6), 'torus': lambda: M.torus(R), 'noisy': lambda: C.noisy(R, 4)}[kind]()
    return torch.from_numpy(f).to(dev).unsqueeze(0).repeat(B, 1, 1, 1).contiguous()


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


rows = []
for kind in args.fields.split(','):
    x = field(kind)
    meshes = mesh.marching_cubes(x)
    stats = {}
    out = mesh.largest_component(meshes, stats=stats)            # warm-up: code loading, allocator
    torch.cuda.synchronize()
    if args.once:
        out = mesh.largest_component(meshes)
        torch.cuda.synchronize()
        continue
    for _ in range(2):
        mesh.largest_component(meshes)
        mesh.marching_cubes(x)
    torch.cuda.synchronize()
    us_cc, out = timed(lambda: mesh.largest_component(meshes), args.reps)
    us_mc, _ = timed(lambda: mesh.marching_cubes(x), args.reps)
    us_both, _ = timed(lambda: mesh.marching_cubes(x, clean=True), args.reps)
    V = sum(int(v.shape[0]) for v, _ in meshes)
    F = sum(int(f.shape[0]) for _, f in meshes)
    KV = sum(int(v.shape[0]) for v, _ in out)
    KF = sum(int(f.shape[0]) for _, f in out)
    # host path, one shape: copy, components, table, selection, extraction
    torch.cuda.synchronize()
    t = time.perf_counter()
    hv, hf = meshes[0][0].cpu().numpy(), meshes[0][1].cpu().numpy()
    copy_s = time.perf_counter() - t
    wv, wf, comps = C.clean(hv, hf)
    host_s = time.perf_counter() - t
    assert comps == stats['components'][0] and np.array_equal(wf, out[0][1].cpu().numpy())
    nbytes = 5 * 12 * F + 6 * 4 * V + 12 * V + 12 * KV + 12 * KF
    med = statistics.median(us_cc)
    row = dict(field=kind, B=B, R=R, V=V, F=F, kept_V=KV, kept_F=KF, components_per_shape=stats['components'][0],
               clean_us_median=med, clean_us_min=min(us_cc), mc_us_median=statistics.median(us_mc),
               mc_clean_us_median=statistics.median(us_both), algorithmic_MB=nbytes / 1e6,
               TBps=nbytes / med / 1e6, host_copy_s_per_shape=copy_s, host_clean_s_per_shape=host_s,
               speedup_vs_host=host_s * B / (med * 1e-6))
    rows.append(row)
    print(json.dumps(row), flush=True)
res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows)
if args.out and not args.once:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
