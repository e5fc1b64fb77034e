"""Normal estimation (csrc/ofx_normals.hip) at the driver's cloud size: kNN, PCA and orientation timed stage by stage
with HIP events around calls that end in a synchronise, after a warm-up call of every shape, for one cloud and for eight
clouds of n points (default 100 000) sampled from marching-cubes meshes of analytic fields (tori, spheres, a rounded
box) with their face normals -- so the share of wrong signs and the unoriented angle error are measured as well.

  * knn at k = 16 and k = 64, automatic grid; beside it recon_metrics.nearest of the same cloud against itself, the
    existing exact 1-NN sweep over n^2 pairs, as the yardstick.
  * pca, orient (the automatic G, 8 steps, 3 rounds).
  * --recon: reconstruct() through the config's GraphVAE with seeded random weights, once from the true normals and once
    with estimate_normals=True, and recon_metrics.surface_scores of one mesh against the other.

    python tools/normals_probe.py --out profiles/normals/normals_probe.json [--n 100000] [--reps 5] [--recon]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from octfusion_amd import _lib, mesh, metrics, normals, recon_metrics

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--n', type=int, default=100000, help='points per cloud')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--recon', action='store_true')
ap.add_argument('--config', default='snet_uncond')
ap.add_argument('--sdf-resolution', type=int, default=128)
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')
n = args.n


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, out


def best(fn):
    fn()
    torch.cuda.synchronize()
    ts = [timed(fn)[0] for _ in range(args.reps)]
    return dict(seconds=ts, seconds_min=min(ts))


# ---- eight meshes of analytic fields on a 128^3 lattice
R = 128
ax = torch.arange(R, device=dev, dtype=torch.float32) * (1.8 / R) - 0.9
x, y, z = torch.meshgrid(ax, ax, ax, indexing='ij')
torus = lambda a, b: ((x * x + y * y).sqrt() - a).pow(2).add(z * z).sqrt() - b             # noqa: E731
ball = lambda r, cx: ((x - cx).pow(2) + y * y + z * z).sqrt() - r                          # noqa: E731
rbox = lambda hx, hy, hz: torch.stack([x.abs() - hx, y.abs() - hy, z.abs() - hz]).clamp(min=0).pow(2).sum(0).sqrt() - 0.08  # noqa: E731
fields = [torus(0.55, 0.2), ball(0.7, 0.0), torch.minimum(ball(0.3, -0.4), ball(0.3, 0.4)), rbox(0.6, 0.4, 0.2),
          torus(0.5, 0.12), ball(0.5, 0.1), rbox(0.3, 0.6, 0.3), torus(0.6, 0.25)]
meshes = mesh.marching_cubes(torch.stack(fields), scale=1.0)
pts, nrm = metrics.sample_surface(meshes, n=n, seed=0, normalize=False, normals=True)
clouds = [pts[j].contiguous() for j in range(len(meshes))]
rows = {}

for label, group in (('one', clouds[:1]), ('eight', clouds)):
    B = normals._Batch(group)
    r = {'clouds': len(group), 'n': n}
    for k in (16, 64):
        r['knn_k%d' % k] = best(lambda: normals._knn(B, k, 0))
    idx, d2 = normals._knn(B, 16, 0)
    r['knn_cells'] = _lib.lib().ofx_knn_cells(n)
    r['nn_search_self'] = best(lambda: recon_metrics.nearest(group, group))
    r['knn_k16_over_nn_search'] = r['knn_k16']['seconds_min'] / r['nn_search_self']['seconds_min']
    un = torch.empty(B.total, 3, device=dev)
    var = torch.empty(B.total, device=dev)
    deg = torch.zeros(B.batch, dtype=torch.int32, device=dev)
    r['pca'] = best(lambda: _lib.call('ofx_pca_normals', B.p.data_ptr(), B.off.data_ptr(), idx.data_ptr(), B.batch,
                                      B.total, B.max_n, 16, un.data_ptr(), var.data_ptr(), deg.data_ptr(),
                                      _lib.stream()))
    lo, e, G, _ = normals._cubes(B, d2, 16, None)
    g_dev = torch.tensor(G, dtype=torch.int32).to(dev)
    ws = torch.empty(_lib.lib().ofx_orient_normals_ws_bytes(B.batch, B.total, max(G)), dtype=torch.uint8, device=dev)
    out = torch.empty_like(un)
    counts = torch.zeros(B.batch, 4, dtype=torch.int32, device=dev)
    r['orient'] = best(lambda: _lib.call('ofx_orient_normals', B.p.data_ptr(), un.data_ptr(), B.off.data_ptr(),
                                         idx.data_ptr(), B.batch, B.total, B.max_n, 16, lo.data_ptr(), e.data_ptr(),
                                         g_dev.data_ptr(), max(G), 8, 3, ws.data_ptr(), out.data_ptr(), None,
                                         counts.data_ptr(), _lib.stream()))
    r['G'] = G
    r['counts'] = counts.tolist()
    r['estimate_normals_call'] = best(lambda: normals.estimate_normals(group))
    true = torch.cat([nrm[j] for j in range(len(group))])
    dots = (out.double() * true.double()).sum(1)
    ang = torch.rad2deg(torch.acos(dots.abs().clamp(max=1.0)))
    r['wrong_sign_share'] = [float((d < 0).double().mean()) for d in dots.split(B.sizes)]
    r['unoriented_angle_deg'] = dict(median=float(ang.median()), p99=float(ang.quantile(0.99)), max=float(ang.max()))
    rows[label] = r
    print(json.dumps({label: r}), flush=True)

if args.recon:
    from octfusion_amd import reconstruct as RC
    vae = RC.build_vae(args.config).to(dev).eval()
    cfg = RC.recon_config(args.config)
    ps = cfg['point_scale']
    rec = {}
    for j in (0, 2, 3):
        c, s = RC._frame(meshes[j][0])
        p = ((clouds[j] - c) * (s * 0.9)).cpu().numpy() * np.float32(ps)
        res = []
        for true_normals in (True, False):
            item = {'name': 'shape%d' % j, 'kind': 'points', 'path': 'shape%d' % j, 'points': p,
                    'normals': nrm[j].cpu().numpy() if true_normals else None}
            res.append(RC.reconstruct(vae, cfg, [item], dev, sdf_resolution=args.sdf_resolution, chamfer_points=0,
                                      estimate_normals=not true_normals))
        a, b = res[0]['meshes']['shape%d' % j], res[1]['meshes']['shape%d' % j]
        row = {'faces_true': int(a[1].shape[0]), 'faces_estimated': int(b[1].shape[0]),
               'normals': res[1]['shapes']['shape%d' % j].get('normals')}
        if a[1].shape[0] and b[1].shape[0]:
            sc = recon_metrics.surface_scores(a, b, n=n)
            row.update(chamfer_l1=sc['chamfer_l1'], normal_consistency=sc['normal_consistency'], fscore=sc['fscore'])
        rec['shape%d' % j] = row
        print(json.dumps({'shape%d' % j: row}), flush=True)
    rows['reconstruct_estimated_vs_true_normals'] = rec

res = dict(device=torch.cuda.get_device_name(0), rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
