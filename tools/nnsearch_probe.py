"""The nearest-neighbour search (csrc/ofx_nnsearch.hip) at one pair of large clouds, beside metrics.nn_matrix on the same
pair, and recon_metrics.surface_scores at its default sample count -- timed with HIP events around calls that end in a
synchronise, after a warm-up call of every shape, the two searches alternating in one process.

  * nearest: one pair of n x n points (default 100 000): the automatic geometry cuts the target cloud into slices, so
    ceil(n / 2048) * slices blocks share the n^2 point pairs; 3 packed issues per two pairs for the distance plus a
    compare and two selects per pair for (minimum, index) = 4.5 issue slots per pair against the VALU issue roof
    (256 CUs x 4 SIMDs x 16 lanes / clock at 2.4 GHz).
  * nn_matrix: the same n^2 pairs in one block of 256 threads on one CU.
  * the mean of nearest's dist2 against nn_matrix's entry (the same distances; nn_matrix sums them in fp32).
  * surface_scores of two marching-cubes spheres at n samples per side: two samplings, one search call over both
    directions, the float64 reductions and the host read.

    python tools/nnsearch_probe.py --out profiles/nnsearch/nnsearch_probe.json [--n 100000] [--reps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from octfusion_amd import _lib, mesh, metrics, recon_metrics

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--n', type=int, default=100000, help='points per cloud')
ap.add_argument('--reps', type=int, default=5, help='timed calls of each search, alternating')
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')
CLOCK, ROOF_LANES = 2.4e9, 256 * 4 * 16
n = args.n


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, out


g = torch.Generator(device=dev).manual_seed(0)
A = (torch.rand(1, n, 3, device=dev, generator=g) - 0.5).contiguous()
B = (torch.rand(1, n, 3, device=dev, generator=g) - 0.5).contiguous()
search = lambda: recon_metrics.nearest(A, B)                        # noqa: E731
matrix = lambda: metrics.nn_matrix(A, B)                            # noqa: E731
(d2, ix), D = search(), matrix()                                    # warm-up of both shapes
torch.cuda.synchronize()
t_search, t_matrix = [], []
for _ in range(args.reps):
    t_search.append(timed(search)[0])
    t_matrix.append(timed(matrix)[0])
pairs = float(n) ** 2
splits = _lib.lib().ofx_nn_search_splits(1, n, n)
rows = {'nearest': dict(n=n, slices=splits, blocks=-(-n // _lib.lib().ofx_nn_search_qpass()) * splits,
                        seconds=t_search, seconds_min=min(t_search), point_pairs=pairs,
                        roof_seconds_4p5_issues=pairs * 4.5 / (ROOF_LANES * CLOCK),
                        frac_of_roof_4p5_issues=pairs * 4.5 / (ROOF_LANES * CLOCK) / min(t_search)),
        'nn_matrix': dict(n=n, blocks=1, seconds=t_matrix, seconds_min=min(t_matrix)),
        'speedup_min_over_min': min(t_matrix) / min(t_search),
        'mean_dist2': dict(nearest_float64=float(d2.double().mean()), nn_matrix_float32=float(D[0, 0]))}
print(json.dumps(rows), flush=True)

# ---- surface_scores at the default sample count: two spheres of a 128^3 lattice
R = 128
ax = torch.arange(R, device=dev, dtype=torch.float32) * (1.8 / R) - 0.9
x, y, z = torch.meshgrid(ax, ax, ax, indexing='ij')
rad = (x * x + y * y + z * z).sqrt()
meshes = mesh.marching_cubes(torch.stack([rad - 0.5, rad - 0.52]), scale=0.5)
score = lambda: recon_metrics.surface_scores(meshes[0], meshes[1], n=n)     # noqa: E731
s = score()
t_scores = [timed(score)[0] for _ in range(args.reps)]
rows['surface_scores'] = dict(n=n, seconds=t_scores, seconds_min=min(t_scores), chamfer_l1=s['chamfer_l1'],
                              fscore=s['fscore'], normal_consistency=s['normal_consistency'])
print(json.dumps(rows['surface_scores']), flush=True)
res = dict(device=torch.cuda.get_device_name(0), clock_assumed_hz=CLOCK, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
