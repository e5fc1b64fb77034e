"""Marching cubes on the device (octfusion_amd.mesh.marching_cubes, csrc/ofx_mesh.hip), timed with HIP events from
the count launch to the end of the emit pass (the count readback included), against the algorithmic bytes
B * 4 R^3 (the lattice, read once) + 12 V + 12 F and the 8 TB/s HBM roof; the numpy oracle (tests/mc_oracle.py) on the
same lattice is the host baseline (one shape, seconds).

Workloads: B in {1, 8} x R in {128, 256} on a sphere, a torus and the SDF of generated shapes (snet_uncond with
synthetic weights, bench shell-6 split codes, 2 DDIM steps; shapes differ per batch element).

    python tools/mesh_probe.py --out profiles/mesh/mesh_probe.json [--sizes 256 --batches 8 --fields sphere]
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

import mc_oracle as M
from octfusion_amd import _lib, configs, generate as G, mesh, synthetic
from octfusion_amd.pipeline import CascadeSampler

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--sizes', default='128,256')
ap.add_argument('--batches', default='1,8')
ap.add_argument('--fields', default='sphere,torus,generated')
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device('cuda:0')
_lib.require_device()

generated = {}


def gen_lattices(R):
    if R not in generated:
        cfg = configs.CONFIGS['snet_uncond']
        net, vae, _ = G.prepare('snet_uncond', 0, dev)
        cs = CascadeSampler(net, cfg, vae)
        out = cs.sample(8, ddim_steps=2, seed=0, shape_indices=list(range(8)),
                        split_small=synthetic.shell6_split(8, jitter=True).to(dev), sdf_resolution=R)
        generated[R] = out['sdfs'].contiguous()
    return generated[R]


def field(kind, R, B):
    if kind == 'generated':
        return gen_lattices(R)[:B].contiguous()
    f = M.sphere(R, r=0.6) if kind == 'sphere' else M.torus(R)
    return torch.from_numpy(f).to(dev).unsqueeze(0).repeat(B, 1, 1, 1).contiguous()


rows = []
for R in [int(r) for r in args.sizes.split(',')]:
    for kind in args.fields.split(','):
        for B in [int(b) for b in args.batches.split(',')]:
            x = field(kind, R, B)
            for _ in range(3):
                out = mesh.marching_cubes(x)                 # warm-up: code loading, allocator
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = mesh.marching_cubes(x)
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1))
            V = sum(int(v.shape[0]) for v, _ in out)
            F = sum(int(f.shape[0]) for _, f in out)
            nbytes = B * 4 * R ** 3 + 12 * V + 12 * F
            med = statistics.median(us)
            t = time.perf_counter()
            wv, wf = M.marching_cubes(x[0].cpu().numpy())
            cpu_s = time.perf_counter() - t
            assert (len(wv), len(wf)) == tuple(out[0][0].shape[:1]) + tuple(out[0][1].shape[:1])
            row = dict(field=kind, B=B, R=R, us_median=med, us_min=min(us), V=V, F=F, algorithmic_MB=nbytes / 1e6,
                       TBps=nbytes / med / 1e6, frac_of_8TBps=nbytes / med / 1e6 / 8.0,
                       oracle_cpu_s_per_shape=cpu_s, speedup_vs_oracle=cpu_s * B / (med * 1e-6))
            rows.append(row)
            print(json.dumps(row), flush=True)
res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
