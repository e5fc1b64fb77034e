"""Reconstruction driver: an existing shape in, the GraphVAE's reconstruction of it out, with a Chamfer score.

Mirror of the reference's ``OctFusionVAEModel.inference`` (models/octfusion_model_vae.py:189-205: autoencoder.forward(
octree_in, evaluate=True) -> get_sdfs -> export_mesh -> input.ply) and of ``calc_chamfer``
(utils/util_dualoctree.py:152-168), on the device from the point cloud to the mesh:

    oriented points -> Points.clip -> build_octree_batch -> GraphVAE.forward(evaluate=True) -> mpu.calc_sdf ->
    mesh.marching_cubes -> <out>/<name>/0.obj, <out>/<name>/input.ply, <out>/metrics.json

* Inputs are directories holding the reference's ``pointcloud.npz`` (keys ``points``, ``normals``;
  datasets/dualoctree_snet.py:36-47: points / point_scale, then clip to the open cube), or, with ``--from-mesh``, OBJ
  files -- also the ones ``generate.py --mesh`` writes -- sampled with their face normals on the device
  (metrics.sample_surface(normals=True)) after the max-extent normalisation to [-1, 1] and a factor ``--fit``.
* The SDF is read at the decoder's finest depth (``--mpu-depth``, default depth_out) -- see DESIGN.md 4.9: the
  reference's inference reads depth_stop through forward's wrapper, which ``--mpu-depth <depth_stop>`` reproduces.
* The score is calc_chamfer's pair: n surface samples of each side, not normalised, the two directed mean squared
  nearest-neighbour distances x 1e5.  The samples are the project's (counter hash), not trimesh's with seed 101.
* A shape whose reconstruction is empty gets no OBJ and ``null`` scores, with a warning; the rest go on.
* ``--metrics`` adds the reconstruction table of the occupancy-network line of work to every shape (Chamfer-L1 / -L2,
  completeness, accuracy, normal consistency, F-score at ``--thresholds``) and ``--occupancy`` the volumetric IoU
  against the ``points.npz`` beside a point-cloud input: octfusion_amd.recon_metrics, DESIGN.md 4.15.  Without them
  metrics.json is what it was.
* ``--estimate-normals`` takes clouds that carry no normals -- a ``pointcloud.npz`` without the ``normals`` key, a bare
  ``.npy`` / ``.npz`` (key ``points``) or a ``.ply`` -- and estimates them on the device before the ``Points`` are
  built (octfusion_amd.normals); such a shape's record gains ``normals`` (k, the grid size and the
  orientation counts).  An input that has normals takes exactly the path it takes without the flag.

    python -m octfusion_amd.reconstruct --config snet_uncond --vae vae.pth --input data/02691156/1a04e3 --out recon
    python -m octfusion_amd.reconstruct --config snet_uncond --vae vae.pth --from-mesh --input samples/0.obj --out recon
"""
import argparse
import json
import os
import time
import warnings

import numpy as np
import torch

from . import configs, mesh, metrics, mpu, normals, recon_metrics
from .metrics import sample_surface          # reconstruct() has an argument called metrics
from .octree import Points, build_octree_batch

CHAMFER_SCALE = 1.0e5           # utils/util_dualoctree.py:153
# --points / --chamfer-points default: a choice (the reference has no call site of calc_chamfer and ships its clouds
# ready-made); about one point per depth-8 surface cell
POINTS = 100000


def recon_config(name):
    """What the driver needs of a config name of octfusion_amd.configs: the VAE's octree depths and point_scale."""
    kw = configs.vae_params(name)
    return {'name': name, 'depth': kw['depth'], 'full_depth': kw['full_depth'], 'point_scale': mesh.mesh_scale(name)}


def shape_name(path):
    """The output folder of an input, as inference derives it (octfusion_model_vae.py:193-197): the base name up to its
    last '.'; for a ``pointcloud.npz`` file, its directory's."""
    path = os.path.normpath(path)
    if os.path.basename(path) == 'pointcloud.npz':
        path = os.path.dirname(path)
    name = os.path.basename(path)
    pos = name.rfind('.')
    if pos != -1:
        name = name[:pos]
    if not name:
        raise ValueError('reconstruct: %s leaves no name once its suffix is removed' % path)
    return name


def _read_raw(path):
    """(points, normals or None) of an input of --estimate-normals: a directory with pointcloud.npz, that file, or a
    bare .npy / .npz / .ply cloud."""
    low = path.lower()
    if os.path.isdir(path) or os.path.basename(path) == 'pointcloud.npz':
        low = path = path if os.path.basename(path) == 'pointcloud.npz' else os.path.join(path, 'pointcloud.npz')
    nrm = None
    if low.endswith('.npz'):
        with np.load(path) as z:
            pts = np.asarray(z['points'], np.float32)
            if 'normals' in z.files:
                nrm = np.asarray(z['normals'], np.float32)
    elif low.endswith('.ply'):
        pts, nrm = mesh.read_ply(path)
    else:
        pts = normals.read_cloud(path)
    if pts.ndim != 2 or pts.shape[1] != 3 or (nrm is not None and nrm.shape != pts.shape):
        raise ValueError('reconstruct: %s: points %s, normals %s' % (path, pts.shape, None if nrm is None else nrm.shape))
    return pts, nrm


def read_inputs(paths, from_mesh=False, estimate_normals=False):
    """[{name, kind, path, points + normals | verts + faces}] (numpy, file units) of the input paths; kind 'points' for
    a directory with pointcloud.npz (or the file itself), 'mesh' for an OBJ with from_mesh.  estimate_normals: a point
    input may also be a bare .npy / .npz / .ply file, and may lack normals (``normals`` is then None)."""
    out, seen = [], set()
    for p in paths:
        name = shape_name(p)
        if name in seen:
            raise ValueError('reconstruct: two inputs are named %r' % name)
        seen.add(name)
        if from_mesh:
            if not p.lower().endswith('.obj'):
                raise ValueError('reconstruct: --from-mesh takes .obj files, got %s' % p)
            v, f = mesh.read_obj(p)
            if len(f) == 0:
                raise ValueError('reconstruct: %s has no faces' % p)
            out.append({'name': name, 'kind': 'mesh', 'path': p, 'verts': v, 'faces': f})
        elif estimate_normals:
            pts, nrm = _read_raw(p)
            out.append({'name': name, 'kind': 'points', 'path': p, 'points': pts, 'normals': nrm})
        else:
            f = p if os.path.basename(p) == 'pointcloud.npz' else os.path.join(p, 'pointcloud.npz')
            with np.load(f) as z:
                pts, nrm = np.asarray(z['points'], np.float32), np.asarray(z['normals'], np.float32)
            if pts.ndim != 2 or pts.shape[1] != 3 or nrm.shape != pts.shape:
                raise ValueError('reconstruct: %s: points %s, normals %s' % (f, pts.shape, nrm.shape))
            out.append({'name': name, 'kind': 'points', 'path': p, 'points': pts, 'normals': nrm})
    return out


def _cloud(side, n, seed):
    """[1, m, 3]: n surface samples of a (verts, faces) mesh in its own frame, or a given [m, 3] cloud."""
    if torch.is_tensor(side):
        return side.reshape(1, -1, 3)
    return metrics.sample_surface([side], n=n, seed=seed, normalize=False)


def chamfer(mesh_a, mesh_b, n, seed=0):
    """calc_chamfer(gt, pred, point_num) (utils/util_dualoctree.py:152-168): (chamfer_a, chamfer_b) = the mean squared
    distance from the samples of b to their nearest sample of a, and from those of a to b, x 1e5.  Each side is a
    ``(verts, faces)`` mesh, of which n surface points are drawn without normalising, or an [m, 3] cloud taken as it
    is.  Both sides draw with the same seed and shape id, so a mesh against itself scores exactly (0, 0) -- and the
    two sample sets share their triangle and barycentric random numbers, so for two similar meshes the samples are
    correlated and the score lies slightly below what independent draws (the reference's) give.  Two launches of
    nn_matrix with one cloud on each side; at one pair nn_matrix runs on a single block, over n^2 point pairs per
    direction.  One host read."""
    A, B = _cloud(mesh_a, n, seed), _cloud(mesh_b, n, seed)
    d = torch.cat([metrics.nn_matrix(B, A).reshape(1), metrics.nn_matrix(A, B).reshape(1)]).double() * CHAMFER_SCALE
    ca, cb = d.tolist()
    return ca, cb


def _frame(verts):
    """(centre [3], scale) of the sampler's normalisation: (v - centre) * scale fills the [-1, 1] max-extent cube."""
    lo, hi = verts.min(0).values, verts.max(0).values
    ext = float((hi - lo).max())
    return (lo + hi) * 0.5, (2.0 / ext if ext > 0 else 1.0)


def _input_dir(path):
    """The directory of a point-cloud input: the path itself, or the one holding the ``pointcloud.npz`` it names."""
    return os.path.dirname(path) if os.path.basename(os.path.normpath(path)) == 'pointcloud.npz' else path


def _lap(timings, name, t0, device):
    if timings is None:
        return t0
    if device.type == 'cuda':
        torch.cuda.synchronize(device)
    t1 = time.perf_counter()
    timings[name] = timings.get(name, 0.0) + t1 - t0
    return t1


@torch.no_grad()
def reconstruct(vae, cfg, inputs, device, sdf_resolution=256, sdf_scale=0.9, level=0.0, clean=False, batch=8, seed=0,
                points=POINTS, chamfer_points=POINTS, fit=None, mpu_depth=None, out_dir=None, timings=None,
                metrics=False, thresholds=recon_metrics.THRESHOLDS, occupancy=False, field_mesh=False, mesh_margin=1,
                estimate_normals=False, normal_k=16, exact=False):
    """Reconstruct every shape of ``inputs`` (read_inputs) through ``vae``, ``batch`` shapes per call.  cfg:
    recon_config(name), or a dict with depth, full_depth, point_scale.  points: samples per mesh input; fit: factor
    on the normalised mesh samples (default sdf_scale); mpu_depth: depth the SDF is read at (default depth_out);
    chamfer_points: samples per side of the score (0: no score).  The posterior noise comes from torch's generator,
    seeded with ``seed`` once at the start.  Writes <out_dir>/<name>/0.obj, <name>/input.ply and metrics.json when
    out_dir is given.  Returns the metrics dict; ``result['meshes'][name]`` holds the device meshes.
    metrics: each shape's record gains ``scores`` = recon_metrics.surface_scores(gt, reconstruction) at ``thresholds``
    (file units), with chamfer_points samples per mesh side (POINTS when chamfer_points is 0, so that
    ``metrics=True, chamfer_points=0`` scores at 100 000 points without the single-block Chamfer launches); the gt side
    is the input mesh in the output frame or, for a point-cloud input, the oriented input cloud x point_scale cut to
    that count by the Chamfer score's stride rule; ``null`` for an empty reconstruction.  exact: a mesh input is scored
    with ``surface_scores(exact=True)``, samples against the other side's triangles (a point-cloud input has no
    triangles and is scored as before).  occupancy: a point-cloud
    input whose directory holds ``points.npz`` gains ``iou``, ``iou_intersection``, ``iou_union`` =
    recon_metrics.occupancy_iou of the batch's ``neural_mpu`` field against that file; any other input gets ``null``
    and a warning; ``result['fields'][name]`` = (field, batch index).
    field_mesh: mesh the field in octree-guided bricks (mesh.field_mesh: sdf_resolution up to 2048, a band of
    mesh_margin finest octree cells around the finest nodes, no dense lattice); each shape's record gains ``mesh_stats``
    (seeds, bricks, leaks, total_bricks).
    estimate_normals: a point input whose ``normals`` is None gets them from normals.estimate_normals(k=normal_k) on the
    device, all such clouds of a group in one call; its record gains ``normals`` = {k, G, undecided_after_march,
    flipped_by_vote, undecided, degenerate}.  Without it such an input is an error."""
    device = torch.device(device)
    ps = float(cfg['point_scale'])
    fit = float(sdf_scale if fit is None else fit)
    d_mpu = vae.depth_out if mpu_depth is None else int(mpu_depth)
    torch.manual_seed(seed)
    shapes, meshes, fields = {}, {}, {}
    score_points = chamfer_points if chamfer_points else POINTS
    for g0 in range(0, len(inputs), batch):
        group = inputs[g0:g0 + batch]
        t0 = time.perf_counter()
        # ---- oriented clouds in the encoder's frame, [-1, 1]^3
        clouds, gts = [None] * len(group), [None] * len(group)
        mesh_pos = [k for k, it in enumerate(group) if it['kind'] == 'mesh']
        if mesh_pos:
            vf = [(torch.from_numpy(group[k]['verts']).to(device), torch.from_numpy(group[k]['faces']).to(device))
                  for k in mesh_pos]
            p, n = sample_surface(vf, n=points, seed=seed, normalize=True, ids=[g0 + k for k in mesh_pos],
                                  normals=True)
            for j, k in enumerate(mesh_pos):
                clouds[k] = Points(p[j] * fit, n[j])
                c, s = _frame(vf[j][0])
                gts[k] = ((vf[j][0] - c) * (s * fit * ps), vf[j][1])        # the input mesh in the output frame
        raw_pos = [k for k, it in enumerate(group) if it['kind'] == 'points' and it['normals'] is None]
        if raw_pos and not estimate_normals:
            raise ValueError('reconstruct: %s has no normals (estimate_normals is off)' % group[raw_pos[0]]['path'])
        est, nstats = {}, {}
        if raw_pos:
            got = normals.estimate_normals([torch.from_numpy(group[k]['points']).to(device) / ps for k in raw_pos],
                                           k=normal_k, stats=nstats)
            est = dict(zip(raw_pos, got))
            nstats = {k: dict({'k': int(normal_k), 'G': nstats['G'][j]}, **{c: nstats[c][j] for c in normals.COUNTS})
                      for j, k in enumerate(raw_pos)}
        for k, it in enumerate(group):
            if it['kind'] == 'points':
                clouds[k] = Points(torch.from_numpy(it['points']).to(device) / ps,
                                   est[k] if k in est else torch.from_numpy(it['normals']).to(device))
        for k, c in enumerate(clouds):
            c.clip(-1.0, 1.0)
            if c.points.shape[0] == 0:
                raise ValueError('reconstruct: %s has no point inside the cube' % group[k]['path'])
        t0 = _lap(timings, 'sample', t0, device)
        # ---- encode, decode (growing the octree), SDF lattice, mesh
        octree_in = build_octree_batch(clouds, cfg['depth'], cfg['full_depth'])
        t0 = _lap(timings, 'octree', t0, device)
        out = vae.forward(octree_in, evaluate=True, mpu_depth=d_mpu)
        t0 = _lap(timings, 'vae_forward', t0, device)
        fstats = {}
        if field_mesh:
            recon = mesh.field_mesh(out['neural_mpu'], sdf_resolution, level=level, bbmin=-sdf_scale, bbmax=sdf_scale,
                                    scale=ps, margin=mesh_margin, clean=clean, stats=fstats)
            fstats.pop('components', None)
        else:
            sdfs = mpu.calc_sdf(out['neural_mpu'], len(group), size=sdf_resolution, bbmin=-sdf_scale, bbmax=sdf_scale)
            t0 = _lap(timings, 'sdf', t0, device)
            recon = mesh.marching_cubes(sdfs, level=level, bbmin=-sdf_scale, bbmax=sdf_scale, scale=ps, clean=clean)
        t0 = _lap(timings, 'mesh', t0, device)
        # ---- score and files
        for k, it in enumerate(group):
            name, (v, f) = it['name'], recon[k]
            rec = {'gt': it['kind'], 'input_points': int(clouds[k].points.shape[0]), 'vertices': int(v.shape[0]),
                   'faces': int(f.shape[0]), 'chamfer_a': None, 'chamfer_b': None, 'obj': None}
            if field_mesh:
                rec['mesh_stats'] = {key: int(val[k]) for key, val in fstats.items()}
            if k in nstats:
                rec['normals'] = nstats[k]
            if f.shape[0] == 0:
                warnings.warn('reconstruct: %s: marching cubes found no surface, no mesh written' % name)
            elif chamfer_points:
                gt = gts[k]
                if gt is None:                    # point-cloud input: the points the encoder saw, in file units
                    pts = clouds[k].points
                    if pts.shape[0] > chamfer_points:
                        pts = pts[torch.arange(chamfer_points, device=device) * pts.shape[0] // chamfer_points]
                    gt = pts * ps
                rec['chamfer_a'], rec['chamfer_b'] = chamfer(gt, (v, f), chamfer_points, seed)
            shapes[name] = rec
            meshes[name] = (v, f)
        t0 = _lap(timings, 'chamfer', t0, device)
        if metrics:
            for k, it in enumerate(group):
                (v, f), gt = recon[k], gts[k]
                if gt is None:                        # the oriented cloud the encoder saw, in file units
                    pts, nrm = clouds[k].points, clouds[k].normals
                    if pts.shape[0] > score_points:
                        sel = torch.arange(score_points, device=device) * pts.shape[0] // score_points
                        pts, nrm = pts[sel], nrm[sel]
                    gt = (pts * ps, nrm)
                shapes[it['name']]['scores'] = None if f.shape[0] == 0 else recon_metrics.surface_scores(
                    gt, (v, f), n=score_points, seed=seed, thresholds=thresholds,
                    exact=bool(exact) and gts[k] is not None)
            t0 = _lap(timings, 'scores', t0, device)
        if occupancy:
            for k, it in enumerate(group):
                rec = shapes[it['name']]
                rec['iou'] = rec['iou_intersection'] = rec['iou_union'] = None
                fields[it['name']] = (out['neural_mpu'], k)
                occu = os.path.join(_input_dir(it['path']), 'points.npz') if it['kind'] == 'points' else None
                if occu is None or not os.path.exists(occu):
                    warnings.warn('reconstruct: %s: no points.npz beside the input, no IoU' % it['name'])
                    continue
                with np.load(occu) as z:
                    rec['iou'], rec['iou_intersection'], rec['iou_union'] = recon_metrics.occupancy_iou(
                        out['neural_mpu'], z['points'], z['occupancies'], ps, level=level, batch_index=k)
            t0 = _lap(timings, 'iou', t0, device)
        if out_dir is not None:
            for k, it in enumerate(group):
                d = os.path.join(out_dir, it['name'])
                os.makedirs(d, exist_ok=True)
                if shapes[it['name']]['faces']:
                    mesh.write_obj(os.path.join(d, '0.obj'), *recon[k])
                    shapes[it['name']]['obj'] = os.path.join(it['name'], '0.obj')
                mesh.write_ply(os.path.join(d, 'input.ply'), clouds[k].points, clouds[k].normals)
            t0 = _lap(timings, 'write', t0, device)
    res = {'config': cfg.get('name'), 'point_scale': ps, 'sdf_resolution': sdf_resolution, 'sdf_scale': sdf_scale,
           'mpu_depth': d_mpu, 'fit': fit, 'seed': seed, 'chamfer_points': chamfer_points,
           'chamfer_scale': CHAMFER_SCALE, 'shapes': shapes}
    if field_mesh:
        res.update(field_mesh=True, mesh_margin=mesh_margin)
    if timings is not None:
        res['phase_seconds'] = dict(timings)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, 'metrics.json'), 'w') as fh:
            json.dump(res, fh, indent=1)
    res['meshes'] = meshes
    if occupancy:
        res['fields'] = fields
    return res


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.reconstruct', description=__doc__.split('\n\n')[0])
    ap.add_argument('--config', default='snet_uncond', choices=sorted(configs.CONFIGS))
    ap.add_argument('--vae', default=None, help='GraphVAE checkpoint (seeded random weights when absent)')
    ap.add_argument('--allow-pickle', action='store_true',
                    help='read the checkpoint file with the full unpickler (only for files you trust)')
    ap.add_argument('--input', nargs='+', required=True, metavar='PATH',
                    help='directories holding pointcloud.npz (keys points, normals); with --from-mesh, .obj files')
    ap.add_argument('--out', required=True, metavar='DIR',
                    help='writes DIR/<name>/0.obj, DIR/<name>/input.ply and DIR/metrics.json')
    ap.add_argument('--from-mesh', action='store_true',
                    help='inputs are OBJ meshes: sampled with face normals on the device after mapping each to the '
                         '[-1, 1] max-extent cube')
    ap.add_argument('--points', type=int, default=POINTS, help='with --from-mesh: surface samples per mesh')
    ap.add_argument('--fit', type=float, default=None,
                    help='with --from-mesh: factor on the normalised samples.  Default: sdf_scale (0.9), the box the '
                         'meshes are extracted in -- a choice of this driver, not a value of the reference, which '
                         'only reads ready-made clouds')
    ap.add_argument('--sdf-resolution', type=int, default=256)
    ap.add_argument('--clean', action='store_true', help='keep only the largest connected component of every mesh')
    ap.add_argument('--field-mesh', action='store_true',
                    help='mesh the field in octree-guided 8^3-cell bricks instead of sweeping the lattice '
                         '(mesh.field_mesh): --sdf-resolution may go up to 2048 and every shape of metrics.json gains '
                         'mesh_stats.  Surface sheets inside coarse leaves, outside the band, are not meshed')
    ap.add_argument('--mesh-margin', type=int, default=1, metavar='M',
                    help='with --field-mesh: width of the band around the finest octree nodes, in finest-level cells')
    ap.add_argument('--batch', type=int, default=8, help='shapes per call')
    ap.add_argument('--seed', type=int, default=0, help='seeds the surface sampler and the posterior noise')
    ap.add_argument('--mpu-depth', type=int, default=None,
                    help='octree depth the SDF is read at (default: depth_out, what decode_code reads; the '
                         'reference\'s inference reads depth_stop)')
    ap.add_argument('--chamfer-points', type=int, default=POINTS,
                    help='surface samples per side of the Chamfer score (default: the --points default, a choice: '
                         'the reference never calls calc_chamfer); 0: no score.  The score of one shape is two '
                         'launches over N^2 point pairs, each on a single block of the device (DESIGN.md 4.9): '
                         'the default is slow, 2048 is cheap; --metrics --chamfer-points 0 is the fast way to a '
                         'Chamfer number at 100 000 points')
    ap.add_argument('--metrics', action='store_true',
                    help='add the reconstruction table to every shape (recon_metrics.surface_scores): Chamfer-L1/L2, '
                         'completeness, accuracy, normal consistency, precision / recall / F-score, with '
                         '--chamfer-points samples per side (%d when that is 0)' % POINTS)
    ap.add_argument('--thresholds', type=float, nargs='+', default=list(recon_metrics.THRESHOLDS), metavar='T',
                    help='with --metrics: the F-score distance thresholds, in file units')
    ap.add_argument('--exact', action='store_true',
                    help='with --metrics: score a mesh input against the triangles of the other side instead of its '
                         'samples (recon_metrics.surface_scores(exact=True), octfusion_amd.mesh_query)')
    ap.add_argument('--estimate-normals', action='store_true',
                    help='accept clouds without normals (pointcloud.npz without the key, bare .npy / .npz / .ply) and '
                         'estimate oriented normals on the device (octfusion_amd.normals)')
    ap.add_argument('--normal-k', type=int, default=16, metavar='K',
                    help='with --estimate-normals: neighbours per point (1..%d)' % normals.MAX_K)
    ap.add_argument('--occupancy', action='store_true',
                    help='add the volumetric IoU against the points.npz beside a pointcloud.npz input '
                         '(recon_metrics.occupancy_iou)')
    return ap


def parse_args(argv=None):
    args = parser().parse_args(argv)
    if args.points < 1 or args.batch < 1 or args.chamfer_points < 0 or args.sdf_resolution < 2:
        raise ValueError('--points, --batch >= 1, --chamfer-points >= 0 and --sdf-resolution >= 2 are required')
    if any(not t > 0 for t in args.thresholds):
        raise ValueError('--thresholds must be positive')
    if args.field_mesh and (args.sdf_resolution > mesh.FIELD_MAX_SIZE or args.mesh_margin < 0):
        raise ValueError('--field-mesh needs --sdf-resolution <= %d and --mesh-margin >= 0' % mesh.FIELD_MAX_SIZE)
    if not 1 <= args.normal_k <= normals.MAX_K:
        raise ValueError('--normal-k must be in [1, %d]' % normals.MAX_K)
    if args.estimate_normals and args.from_mesh:
        raise ValueError('--estimate-normals is for point inputs; --from-mesh samples face normals')
    return args


def build_vae(config, vae_ckpt=None, allow_pickle=False):
    """The config's GraphVAE on the CPU: the checkpoint's weights, or seeded random ones (as generate.py)."""
    from . import checkpoint, synthetic
    from .graph_vae import GraphVAE
    vae = GraphVAE(**configs.vae_params(config))
    if vae_ckpt:
        checkpoint.load_vae(vae_ckpt, vae, allow_pickle=allow_pickle)
    else:
        vae.load_state_dict(synthetic.random_state_dict(vae))
    return vae


def main(argv=None):
    args = parse_args(argv)
    inputs = read_inputs(args.input, args.from_mesh, args.estimate_normals)
    from . import _lib
    _lib.require_device()
    device = torch.device('cuda', torch.cuda.current_device())
    vae = build_vae(args.config, args.vae, args.allow_pickle).to(device).eval()
    timings = {}
    res = reconstruct(vae, recon_config(args.config), inputs, device, sdf_resolution=args.sdf_resolution,
                      clean=args.clean, batch=args.batch, seed=args.seed, points=args.points,
                      chamfer_points=args.chamfer_points, fit=args.fit, mpu_depth=args.mpu_depth, out_dir=args.out,
                      timings=timings, metrics=args.metrics, thresholds=tuple(args.thresholds),
                      occupancy=args.occupancy, field_mesh=args.field_mesh, mesh_margin=args.mesh_margin,
                      estimate_normals=args.estimate_normals, normal_k=args.normal_k, exact=args.exact)
    res.pop('meshes')
    res.pop('fields', None)
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
