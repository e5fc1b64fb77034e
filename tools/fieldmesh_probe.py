"""Field meshing (octfusion_amd.mesh.field_mesh, csrc/ofx_fieldmesh.hip) next to the dense path (mpu.calc_sdf +
mesh.marching_cubes) on one decoded field: the jittered shell-6 batch of three shapes that tests/test_gpu_generate.py
uses, through a narrow net and a randomly initialised GraphVAE (depth_out 8).

Per lattice size: wall time per call over windows of about a quarter of a second of back-to-back calls (host clock,
ending in a device synchronise; the calls read counts back, so events alone would miss the host part), peak device
memory above what was allocated before the call, the
active-brick fraction, and the vertex / face counts.  The two paths alternate inside one process.

    python tools/fieldmesh_probe.py --out profiles/mesh/fieldmesh_probe.json [--reps 5] [--margin 1]
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

from octfusion_amd import _lib, configs, graph_unet_union as U, mesh, mpu, pipeline, synthetic
from octfusion_amd.graph_vae import GraphVAE

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--margin', type=int, default=1)
ap.add_argument('--field-sizes', default='256,512,1024,2048')
ap.add_argument('--dense-sizes', default='256,512')
ap.add_argument('--shapes', type=int, default=3)
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')
B = args.shapes

cfg = dict(configs.SNET_UNCOND, model_channels=[32, 32])
net = U.UNet3DModel(**{k: v for k, v in dict(cfg, stage_flag='hr').items() if k != 'df_type'})
net.load_state_dict(synthetic.random_state_dict(net))
vae = GraphVAE(depth=8, channel_in=4, nout=4, full_depth=4, depth_stop=6, depth_out=8, resblk_type='basic',
               resblk_num=2, code_channel=16, embed_dim=3)
vae.load_state_dict(synthetic.random_state_dict(vae))
cs = pipeline.CascadeSampler(net.to(dev).eval(), cfg, vae.to(dev).eval())
out = cs.sample(B, ddim_steps=2, seed=3, split_small=synthetic.shell6_split(B, jitter=True).to(dev))
field = out['decoded']['neural_mpu']
nodes = [int(v) for v in field.octree.nnum]


def run(fn, reps, window=0.25):
    """(seconds per call of `reps` timed windows, peak bytes above the baseline, last result) after two warm-up calls.
    A window holds as many back-to-back calls as it takes to last about `window` seconds (every call ends in its own
    host readback, so they do not overlap), sized from the second warm-up call."""
    res = fn()
    del res
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    calls = max(1, int(round(window / max(time.perf_counter() - t0, 1e-6))))
    del res
    secs, peak = [], 0
    for i in range(reps):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        for _ in range(calls):
            res = fn()
            if _ + 1 < calls:
                del res
        torch.cuda.synchronize()
        secs.append((time.perf_counter() - t0) / calls)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        if i + 1 < reps:
            del res
    return secs, peak, res, calls


def spread(secs):
    return dict(median_ms=1e3 * statistics.median(secs), min_ms=1e3 * min(secs), max_ms=1e3 * max(secs))


def dense(R):
    return mesh.marching_cubes(mpu.calc_sdf(field, B, size=R, bbmin=-0.9, bbmax=0.9))


rows = []
fsizes = [int(s) for s in args.field_sizes.split(',')]
dsizes = [int(s) for s in args.dense_sizes.split(',')]
for R in sorted(set(fsizes) | set(dsizes)):
    row = dict(size=R, shapes=B, margin=args.margin)
    if R in fsizes:
        st = {}
        secs, peak, res, calls = run(lambda: mesh.field_mesh(field, R, margin=args.margin, stats=st), args.reps)
        row['field_mesh'] = dict(spread(secs), calls_per_window=calls, peak_bytes=int(peak), bricks=st['bricks'],
                                 seeds=st['seeds'],
                                 leaks=st['leaks'], total_bricks=st['total_bricks'],
                                 active_fraction=sum(st['bricks']) / sum(st['total_bricks']),
                                 vertices=[int(v.shape[0]) for v, _ in res], faces=[int(f.shape[0]) for _, f in res])
        del res
    if R in dsizes:
        secs, peak, res, calls = run(lambda: dense(R), args.reps)
        row['dense'] = dict(spread(secs), calls_per_window=calls, peak_bytes=int(peak),
                            vertices=[int(v.shape[0]) for v, _ in res],
                            faces=[int(f.shape[0]) for _, f in res])
        del res
    rows.append(row)
    print(json.dumps(row), flush=True)

rec = dict(probe='fieldmesh', device=torch.cuda.get_device_name(0), octree_nodes_per_depth=nodes, reps=args.reps,
           rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(rec, fh, indent=1)
