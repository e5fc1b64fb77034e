"""Time octfusion_amd.render on the device: 8 marching-cubes meshes from 256^3 lattices x 20 views x
299^2, and a low-polygon mesh of large triangles as raw dataset meshes have them.

    python tools/render_probe.py [--out DIR] [--runs 12] [--lattice 256] [--samples 1|4|16]

Device events around `render` after two warm calls, the median of --runs; then one more call with every entry point
between its own events (_lib.PROFILE).  Bytes are the algorithm's compulsory traffic from the shapes, not a counter:
  project  per view: read verts 12 B, write sxy + depth 16 B, per vertex
  raster   per view: read a face 12 B and its three projected vertices 3 x 16 B, per face; fill the keys 8 B per sample
  shade    read the keys 8 B per sample, write 3 B, per pixel; a covered pixel also reads a face 12 B and three vertices
           36 B (once: further faces of a multisampled pixel are not counted)
Prints one JSON line and, with --out, writes it to DIR/render_probe.json.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octfusion_amd import _lib, mesh, render  # noqa: E402

HBM_PEAK = 8.0e12


def lattices(n, R, dev):
    """n smooth SDF-like fields [R, R, R]: spheres, tori and blends of blobs with different centres."""
    g = torch.arange(R, device=dev, dtype=torch.float32) * (1.8 / R) - 0.9
    x, y, z = torch.meshgrid(g, g, g, indexing='ij')
    out = []
    rng = np.random.default_rng(0)
    for k in range(n):
        if k % 3 == 0:
            f = torch.sqrt(x * x + y * y + z * z) - (0.5 + 0.03 * k)
        elif k % 3 == 1:
            q = torch.sqrt(x * x + y * y) - 0.5
            f = torch.sqrt(q * q + z * z) - (0.15 + 0.01 * k)
        else:
            f = torch.full_like(x, 0.35)
            for _ in range(6):
                c = rng.uniform(-0.5, 0.5, 3)
                s = rng.uniform(0.1, 0.3)
                f = f - torch.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
        out.append(f)
    return torch.stack(out).contiguous()


def low_poly(k=6):
    """A box of 12 k^2 triangles: at 299^2 each covers hundreds of pixels."""
    t = np.linspace(-0.5, 0.5, k + 1)
    vs, fs = [], []
    for axis in range(3):
        for side in (-0.5, 0.5):
            base = len(vs)
            for a in t:
                for b in t:
                    p = [a, b]
                    p.insert(axis, side)
                    vs.append(p)
            for i in range(k):
                for j in range(k):
                    q = base + i * (k + 1) + j
                    fs += [(q, q + 1, q + k + 2), (q, q + k + 2, q + k + 1)]
    return np.asarray(vs, np.float32), np.asarray(fs, np.int32)


def timed(fn, runs):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stages(fn):
    _lib.PROFILE = prof = []
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.PROFILE = None
    out = {}
    for name, e0, e1, _ in prof:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def traffic(meshes, views, size, covered, samples=1):
    nv = sum(int(v.shape[0]) for v, _ in meshes)
    nf = sum(int(f.shape[0]) for _, f in meshes)
    px = len(meshes) * views * size * size
    return {'project': views * nv * 28, 'raster': views * nf * 60 + px * 8 * samples,
            'shade': px * (8 * samples + 3) + covered * 48}


def measure(meshes, size, runs, **kw):
    ms = timed(lambda: render.render(meshes, size=size, **kw), runs)
    st = stages(lambda: render.render(meshes, size=size, **kw))
    _, buf = render.render(meshes, size=size, buffers=True, **kw)
    samples = kw.get('samples', 1)
    hit = buf['ids'] >= 0
    covered = int((hit.any(-1) if samples > 1 else hit).sum())
    by = traffic(meshes, 20, size, covered, samples)
    med = statistics.median(ms)
    return {'meshes': len(meshes), 'vertices': sum(int(v.shape[0]) for v, _ in meshes),
            'faces': sum(int(f.shape[0]) for _, f in meshes), 'size': size, 'samples': samples,
            'runs_ms': [round(m, 3) for m in ms],
            'median_ms': med, 'min_ms': min(ms), 'max_ms': max(ms), 'stage_ms': st, 'bytes': by,
            'bytes_total': sum(by.values()), 'hbm_fraction': sum(by.values()) / (med * 1e-3) / HBM_PEAK,
            'covered_pixels': covered, 'dropped': int(buf['dropped'].sum())}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--runs', type=int, default=12)
    ap.add_argument('--lattice', type=int, default=256)
    ap.add_argument('--shapes', type=int, default=8)
    ap.add_argument('--samples', type=int, default=1, choices=render.SAMPLES, help='samples per pixel')
    args = ap.parse_args(argv)
    _lib.require_device()
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {}
    meshes = mesh.marching_cubes(lattices(args.shapes, args.lattice, dev))
    kw = {'samples': args.samples} if args.samples > 1 else {}
    res['marching_cubes_%d' % args.lattice] = measure(meshes, 299, args.runs, **kw)
    v, f = low_poly()
    lp = [(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))] * args.shapes
    res['low_poly'] = measure(lp, 299, args.runs, **kw)
    res['low_poly_all_threads'] = measure(lp, 299, args.runs, big_px=2 ** 40, **kw)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'render_probe.json'), 'w') as fh:
            fh.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
