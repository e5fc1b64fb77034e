"""Probe of the reconstruction path: per-phase seconds of one reconstruct call at the ShapeNet VAE
config (batch 8, resolution 256, seeded random weights, eight synthetic meshes as --from-mesh inputs), the split of the
VAE forward into graphs / encode / decode, the oriented sampler next to the unoriented one at the same shape, and
nn_matrix with one pair of large clouds.  Host clocks around device synchronises; HIP events for the kernels.

    python tools/reconstruct_probe.py [OUT_DIR]      # OUT_DIR/reconstruct_probe.json (default profiles/reconstruct)
"""
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octfusion_amd import _lib, metrics, reconstruct as R                     # noqa: E402
from octfusion_amd.dual_octree import DualOctree                              # noqa: E402
from octfusion_amd.octree import Points, build_octree_batch                   # noqa: E402


def _grid_faces(idx, nu, nv):
    f = []
    for i in range(nu):
        for j in range(nv):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return f


def uv_mesh(kind, nu=96, nv=64, k=0):
    """A closed torus (2 nu nv faces) or UV sphere; k varies the radius so the eight shapes differ."""
    u = np.linspace(0, 2 * math.pi, nu, endpoint=False)
    if kind == 'torus':
        w = np.linspace(0, 2 * math.pi, nv, endpoint=False)
        U, W = np.meshgrid(u, w, indexing='ij')
        big, small = 0.5 + 0.02 * k, 0.18
        ring = big + small * np.cos(W)
        v = np.stack([ring * np.cos(U), ring * np.sin(U), small * np.sin(W)], -1)
        return v.reshape(-1, 3).astype(np.float32), np.asarray(
            _grid_faces(lambda i, j: (i % nu) * nv + (j % nv), nu, nv), np.int32)
    w = np.linspace(0, math.pi, nv + 1)[1:-1]
    U, W = np.meshgrid(u, w, indexing='ij')
    rad = 0.5 + 0.03 * k
    v = np.stack([rad * np.sin(W) * np.cos(U), rad * np.sin(W) * np.sin(U), rad * np.cos(W)], -1).reshape(-1, 3)
    m = nv - 1
    top, bot = len(v), len(v) + 1
    v = np.concatenate([v, [[0, 0, rad], [0, 0, -rad]]])
    idx = lambda i, j: (i % nu) * m + j                                        # noqa: E731
    f = []
    for i in range(nu):
        f.append([top, idx(i, 0), idx(i + 1, 0)])
        f.append([bot, idx(i + 1, m - 1), idx(i, m - 1)])
        for j in range(m - 1):
            f += [[idx(i, j), idx(i, j + 1), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i + 1, j)]]
    return v.astype(np.float32), np.asarray(f, np.int32)


def sync_clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def event_seconds(fn, iters):
    """Mean seconds of fn over `iters` back-to-back calls, between two HIP events, after one warm call."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def probe_driver(res, vae, inputs, dev, out):
    """The whole call twice: the first warms every shape, the second is the record."""
    cfg = R.recon_config('snet_uncond')
    for rep in ('warm', 'timed'):
        t = {}
        o = R.reconstruct(vae, cfg, inputs, dev, sdf_resolution=256, batch=8, seed=0, timings=t,
                          out_dir=os.path.join(out, 'recon') if rep == 'timed' else None)
        res['reconstruct_' + rep] = t
        res['shapes_' + rep] = o['shapes']
        print(rep, json.dumps(t), flush=True)


def probe_forward_split(res, vae, clouds):
    """graphs / encode / decode of GraphVAE.forward, through the composition the tests pin as bit-equal."""
    for rep in range(2):
        t0 = sync_clock()
        oc = build_octree_batch(clouds, 8, 4)
        t1 = sync_clock()
        doc = DualOctree(oc)
        data = doc.get_input_feature()
        doc.csr(8)
        t2 = sync_clock()
        code, _, _ = vae.encode(data, doc)
        t3 = sync_clock()
        dec = vae.decode_code(code, doc, update_octree=True)
        t4 = sync_clock()
        res['split_%d' % rep] = {'octree': t1 - t0, 'graphs_in': t2 - t1, 'encode': t3 - t2,
                                 'decode_incl_out_graphs': t4 - t3, 'nnum_in': [int(x) for x in oc.nnum],
                                 'nnum_out': [int(x) for x in dec['octree_out'].nnum]}
        print('split', json.dumps(res['split_%d' % rep]), flush=True)


def probe_sampler(res, vf, dev):
    """Oriented next to unoriented at the same shape, alternating, three rounds: the Python call, then the two entry
    points alone through the C ABI."""
    for n_pts in (2048, R.POINTS):
        rows = []
        for _ in range(3):
            a = event_seconds(lambda: metrics.sample_surface(vf, n=n_pts, seed=0, normalize=True), 20)
            b = event_seconds(lambda: metrics.sample_surface(vf, n=n_pts, seed=0, normalize=True, normals=True), 20)
            rows.append((a, b))
        res['sampler_b8_n%d' % n_pts] = {'unoriented_s': [r[0] for r in rows], 'oriented_s': [r[1] for r in rows],
                                          'note': 'whole sample_surface call: host packing, range-check sync'}
        print('sampler', n_pts, rows, flush=True)
    B = len(vf)
    nv = [int(v.shape[0]) for v, _ in vf]
    nf = [int(f.shape[0]) for _, f in vf]
    T = sum(nf)
    offs = torch.tensor(np.concatenate([np.cumsum([0] + nv[:-1]), nv, np.cumsum([0] + nf[:-1]), nf]),
                        dtype=torch.int64).to(dev)
    V = torch.cat([v for v, _ in vf]).contiguous()
    F = torch.cat([f for _, f in vf]).contiguous()
    ws = torch.empty(_lib.lib().ofx_surface_sample_ws_bytes(B, T), dtype=torch.uint8, device=dev)
    for n_pts in (2048, R.POINTS):
        o = torch.empty(B, n_pts, 3, device=dev)
        nn = torch.empty_like(o)
        args = (V.data_ptr(), F.data_ptr(), offs.data_ptr(), None, B, T, n_pts, 0, 1, ws.data_ptr(), o.data_ptr())
        rows = []
        for _ in range(3):
            a = event_seconds(lambda: _lib.call('ofx_surface_sample', *args, _lib.stream()), 200)
            b = event_seconds(lambda: _lib.call('ofx_surface_sample_oriented', *args, nn.data_ptr(), _lib.stream()),
                              200)
            rows.append((a, b))
        res['sampler_abi_b8_n%d' % n_pts] = {'unoriented_s': [r[0] for r in rows], 'oriented_s': [r[1] for r in rows],
                                              'faces': T}
        print('sampler abi', n_pts, rows, flush=True)


def probe_nn_single_pair(res, p):
    for n_pts in (2048, 16384, R.POINTS):
        A = p[0:1, :n_pts].contiguous()
        B = p[1:2, :n_pts].contiguous()
        res['nn_matrix_1x1_n%d' % n_pts] = [event_seconds(lambda: metrics.nn_matrix(A, B), 2) for _ in range(2)]
        print('nn_matrix', n_pts, res['nn_matrix_1x1_n%d' % n_pts], flush=True)


def main(out):
    torch.set_grad_enabled(False)
    _lib.require_device()
    dev = torch.device('cuda', 0)
    os.makedirs(out, exist_ok=True)
    inputs = []
    for k in range(8):
        v, f = uv_mesh('torus' if k % 2 else 'sphere', k=k)
        inputs.append({'name': 's%d' % k, 'kind': 'mesh', 'path': 's%d' % k, 'verts': v, 'faces': f})
    vae = R.build_vae('snet_uncond').to(dev).eval()
    res = {}
    probe_driver(res, vae, inputs, dev, out)
    vf = [(torch.from_numpy(i['verts']).to(dev), torch.from_numpy(i['faces']).to(dev)) for i in inputs]
    p, n = metrics.sample_surface(vf, n=R.POINTS, seed=0, normalize=True, normals=True)
    probe_forward_split(res, vae, [Points(p[j] * 0.9, n[j]) for j in range(8)])
    probe_sampler(res, vf, dev)
    probe_nn_single_pair(res, p)
    with open(os.path.join(out, 'reconstruct_probe.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
    print('done')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'profiles/reconstruct')
