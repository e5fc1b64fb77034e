"""Generate-style driver: independent shapes sharded over the ranks of one node, end to end.

Mirror of the reference's generation loop (train.py:166-185 -> OctFusionModel.sample,
octfusion_model_union.py:354-401): lr DDIM loop -> octree -> hr DDIM loop (-> feature loop for the 3-stage model) ->
GraphVAE.decode_code -> NeuralMPU SDF on the resolution^3 lattice (get_sdfs, :425-433) -> with ``--mesh``, marching
cubes on the device and ``<out>/<index>.obj`` (export_mesh, :435-468, which runs skimage + trimesh on the host;
mesh.py lists the differences).

* The sampling nets hold the EMA weights, as the reference's generate does (train.py:181 ``ema=True``;
  ``self.ema_df`` and ``unet_lr=self.ema_df.unet_lr``, octfusion_model_union.py:319,391).
* Rank r of W produces the shapes with ``result_index = i * W + r`` (dist.shard_indices), ``--batch`` of them per
  call: shapes are independent, so they are batched -- and every shape of a batch still gets exactly the noise the
  reference's one-shape-per-call loop would draw for its result index (CascadeSampler.sample(shape_indices=)).
* Rank 0 owns the weights (checkpoints, or seeded random weights when none are given) and broadcasts U-Net AND VAE
  once over RCCL (dist.broadcast_module_); nothing is communicated per step.

    python -m octfusion_amd.generate --config snet_uncond --shapes 8 --steps 200 [--ckpt df.pth --vae vae.pth]
    python -m octfusion_amd.generate --config snet_uncond --shapes 8 --mesh --out samples     # + samples/<i>.obj
    python -m octfusion_amd.generate --config snet_uncond --shapes 8 --mesh --points 2048 --out samples  # + <i>.npy
    python -m octfusion_amd.generate --config snet_uncond --shapes 8 --mesh --clean --out samples   # largest component
    python -m octfusion_amd.generate --config snet_uncond --shapes 8 --mesh --views --out samples   # + fid_images/
    python -m octfusion_amd.generate --config snet_uncond --shapes 8 --mesh --simplify 64 --out samples  # small .obj
    python -m octfusion_amd.generate --config snet_uncond --shapes 8 --no-vae --octree-mesh --out samples
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m octfusion_amd.generate --config snet_cond --shapes 32 --category 2
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from . import checkpoint, configs, dist, synthetic
from .graph_unet_union import UNet3DModel
from .pipeline import CascadeSampler


def build_models(config, ckpt=None, vae_ckpt=None, with_vae=True, rank=0, allow_pickle=False):
    """(net with EMA weights, vae or None) on the CPU; only rank 0 reads files / draws the synthetic weights."""
    cfg = configs.CONFIGS[config]
    stage = cfg['unet_type'][-1]
    net = UNet3DModel(**configs.unet_params(config, stage))
    vae = None
    if with_vae:
        from .graph_vae import GraphVAE
        vae = GraphVAE(**configs.vae_params(config))
    if rank == 0:
        if ckpt:
            # `net` plays both roles of load_ckpt: the df_* weights are loaded first and then overwritten by ema_df_*,
            # so a file whose two sets differ leaves the EMA set in the sampling net
            checkpoint.load_ckpt(ckpt, net, ema_df=net, allow_pickle=allow_pickle)
        else:
            net.load_state_dict(synthetic.random_state_dict(net))
        if vae is not None:
            if vae_ckpt:
                checkpoint.load_vae(vae_ckpt, vae, allow_pickle=allow_pickle)
            else:
                vae.load_state_dict(synthetic.random_state_dict(vae))
    return net, vae


def plan(n_shapes, rank, world, shapes_per_call):
    """The groups of result indices rank `rank` generates, in order: its share {i : i mod world == rank}
    (train.py:168) cut into calls of `shapes_per_call`."""
    mine = dist.shard_indices(n_shapes, rank, world)
    return [mine[g0:g0 + shapes_per_call] for g0 in range(0, len(mine), shapes_per_call)]


def prepare(config, rank, device, ckpt=None, vae_ckpt=None, with_vae=True, allow_pickle=False):
    """(net, vae, bytes broadcast): models on `device` with rank 0's weights on every rank -- ONE flat broadcast per
    model, U-Net and VAE."""
    net, vae = build_models(config, ckpt, vae_ckpt, with_vae=with_vae, rank=rank, allow_pickle=allow_pickle)
    net = net.to(device).eval()
    nbytes = dist.broadcast_module_(net, src=0)
    if vae is not None:
        vae = vae.to(device).eval()
        nbytes += dist.broadcast_module_(vae, src=0)
    return net, vae, nbytes


def generate(net, cfg, n_shapes, rank, world, seed=0, ddim_steps=200, label=None, vae=None, out_dir=None,
             shapes_per_call=1, use_graph=None, sdf_resolution=None, timings=None, mesh=False, mesh_level=0.0,
             mesh_scale=1.0, points=None, mesh_clean=False, octree_mesh=False, views=False, view_size=299,
             view_samples=1, mesh_simplify=None, field_mesh=False, mesh_margin=1, mesh_smooth=None,
             smooth_normals=False):
    """Yields (result indices, output dict, seconds) for every group of shapes this rank owns.  mesh: also
    out['meshes'] (needs the VAE and sdf_resolution), written as <out_dir>/<index>.obj.  points (needs mesh): also
    out['points'] = {position in the group: [points, 3] cloud} of every non-empty mesh, sampled on the device after the
    unit-cube normalisation (metrics.sample_surface keyed by the result index), written as <out_dir>/<index>.npy.
    mesh_clean (needs mesh): the meshes, files and clouds are those of each shape's largest component, and
    out['mesh_components'] holds the component counts before cleaning.  octree_mesh: also out['octree_meshes'] (and
    out['octree_meshes_large'] for a 3-stage config), written as <out_dir>/octree/<index>.obj (octree_large/).
    views (needs mesh): also out['views'] = {position in the group: uint8 [20, view_size, view_size, 3]}, every
    non-empty mesh (the cleaned one under mesh_clean) seen from the 20 FID views (render.render, view_samples samples
    per pixel), written as
    <out_dir>/fid_images/view_<j>/<index>.png -- the layout of the reference's generate_synth_image.py.
    mesh_simplify=N (needs mesh): also out['simple_meshes'], every mesh (the cleaned one under mesh_clean) simplified
    by vertex clustering with N cells along its longest side (simplify.simplify), and <out_dir>/<index>.obj is that
    mesh; out['meshes'], the clouds and the views stay those of the full mesh.
    field_mesh (needs mesh): the meshes come from mesh.field_mesh (octree-guided bricks, sdf_resolution up to 2048,
    mesh_margin finest octree cells around the finest nodes) instead of the dense sweep: out['mesh_stats'] holds the
    per-shape seeds / bricks / leaks / total_bricks, and there is no out['sdfs'], hence no sdf.pt.
    mesh_smooth=K (needs mesh): out['meshes'] are the meshes (the cleaned ones under mesh_clean) after K Taubin
    iterations (mesh_smooth.smooth), before any simplification; clouds, views and files are the smoothed mesh's.
    smooth_normals (needs mesh_smooth): also out['normals'], the angle-weighted vertex normals of every written
    mesh (None for an empty one), written as vn lines."""
    if mesh_smooth is not None and not mesh:
        raise ValueError('mesh_smooth needs mesh')
    if smooth_normals and mesh_smooth is None:
        raise ValueError('smooth_normals needs mesh_smooth')
    if field_mesh and not mesh:
        raise ValueError('field_mesh needs mesh')
    if mesh_clean and not mesh:
        raise ValueError('mesh_clean needs mesh')
    if views and not mesh:
        raise ValueError('views needs mesh')
    if mesh_simplify is not None and not mesh:
        raise ValueError('mesh_simplify needs mesh')
    cs = CascadeSampler(net, cfg, vae)
    dev = cs.device
    for idxs in plan(n_shapes, rank, world, shapes_per_call):
        lab = None
        if label is not None:
            lab = torch.full((len(idxs),), int(label), dtype=torch.long, device=dev)
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = cs.sample(len(idxs), ddim_steps=ddim_steps, label=lab, seed=seed, shape_indices=idxs,
                        use_graph=use_graph, sdf_resolution=sdf_resolution if vae is not None else None,
                        timings=timings, mesh=mesh, mesh_level=mesh_level, mesh_scale=mesh_scale,
                        **({'mesh_clean': True} if mesh_clean else {}),
                        **({'field_mesh': True, 'mesh_margin': mesh_margin} if field_mesh else {}),
                        **({'mesh_smooth': mesh_smooth} if mesh_smooth is not None else {}),
                        **({'octree_mesh': True} if octree_mesh else {}))
        if dev.type == 'cuda':
            torch.cuda.synchronize()
            from . import ops
            ops.raise_on_sync_error(dev)         # (the DDIM loops check per stage; this covers the VAE decode)
        dt = time.perf_counter() - t0
        if points:
            out['points'] = sample_points(out['meshes'], idxs, points, seed)
        if views:
            out['views'] = render_views(out['meshes'], view_size, view_samples)
        if mesh_simplify is not None:
            from . import simplify
            out['simple_meshes'] = simplify.simplify(out['meshes'], cells=mesh_simplify)
        if smooth_normals:
            out['normals'] = written_normals(out.get('simple_meshes', out['meshes']))
        if out_dir is not None:
            write_outputs(out_dir, idxs, out, cfg)
        yield idxs, out, dt


def sample_points(meshes, idxs, points, seed):
    """{position: cloud} of the non-empty meshes of one group, as generate_pointclouds.py samples its OBJ files
    (metrics/generate_pointclouds.py:33-37), without the OBJ round trip."""
    from . import metrics
    keep = [b for b, (_, f) in enumerate(meshes) if f.shape[0] > 0]
    if not keep:
        return {}
    pts = metrics.sample_surface([meshes[b] for b in keep], n=points, seed=seed, ids=[idxs[b] for b in keep])
    return {b: pts[j] for j, b in enumerate(keep)}


def render_views(meshes, size=299, samples=1):
    """{position: [20, size, size, 3] uint8} of the non-empty meshes of one group: generate_image_for_fid
    (utils/render_utils.py:14-23) without the OBJ round trip."""
    from . import render
    keep = [b for b, (_, f) in enumerate(meshes) if f.shape[0] > 0]
    if not keep:
        return {}
    images = render.render([meshes[b] for b in keep], size=size, samples=samples)
    return {b: images[j] for j, b in enumerate(keep)}


def written_normals(meshes):
    """Per mesh the angle-weighted vertex normals (mesh_smooth.vertex_normals), None for a mesh without faces."""
    from . import mesh_smooth
    keep = [b for b, (_, f) in enumerate(meshes) if f.shape[0] > 0]
    res = [None] * len(meshes)
    if keep:
        for b, n in zip(keep, mesh_smooth.vertex_normals([meshes[b] for b in keep])):
            res[b] = n
    return res


def write_outputs(out_dir, idxs, out, cfg):
    """Per shape: <index>/split_small.pth (+ split_large.pth) in the reference's sample-file format
    (tools/gen_split.py:50-54), <index>/sdf.pt when the SDF lattice was computed, and <index>.obj (export_mesh's
    file name, octfusion_model_union.py:466) when the meshes were -- the simplified mesh when there is one; an empty
    mesh is skipped with a warning -- and
    <index>.npy, its [points, 3] surface samples, when they were.  With the octree meshes: octree/<index>.obj
    (export_octree's file name, :376,420) and, for the large depth, octree_large/<index>.obj -- the reference writes
    both depths to octree/<index>.obj, so its depth-8 file replaces the depth-6 one
    (octfusion_model_union_3t.py:172,191).  With the views: fid_images/view_<j>/<index>.png."""
    from .octree import octree2split_large, octree2split_small
    small = octree2split_small(out['octree_small'], cfg['full_depth'])
    large = bid = None
    if 'octree_large' in out:
        # depth-8 cascade (3-stage model): the stage-2 sample format, one [nnum6 of the shape, 8] tensor per shape
        # (gen_split.py:50-54 writes it from a one-shape octree; here the batch is sliced by the depth-6 batch ids)
        sd = cfg['input_depth'][1]
        large = octree2split_large(out['octree_large'], sd)
        bid = out['octree_large'].batch_id(sd)
    for b, i in enumerate(idxs):
        d = os.path.join(out_dir, str(i))
        os.makedirs(d, exist_ok=True)
        torch.save(small[b].cpu(), os.path.join(d, 'split_small.pth'))
        if large is not None:
            torch.save(large[bid == b].cpu(), os.path.join(d, 'split_large.pth'))
        if 'sdfs' in out:
            torch.save(out['sdfs'][b].cpu(), os.path.join(d, 'sdf.pt'))
        if 'meshes' in out:
            from . import mesh
            mesh.write_obj(os.path.join(out_dir, '%d.obj' % i), *out.get('simple_meshes', out['meshes'])[b],
                           **({'normals': out['normals'][b]} if 'normals' in out else {}))
        for key, sub in (('octree_meshes', 'octree'), ('octree_meshes_large', 'octree_large')):
            if key in out:
                from . import mesh
                mesh.write_obj(os.path.join(out_dir, sub, '%d.obj' % i), *out[key][b])
        if b in out.get('points', {}):
            np.save(os.path.join(out_dir, '%d.npy' % i), out['points'][b].cpu().numpy())
        if b in out.get('views', {}):
            from . import render
            render.write_fid_images(os.path.join(out_dir, 'fid_images'), [i], out['views'][b][None])


def run(args, rank, local_rank, world, device):
    cfg = configs.CONFIGS[args.config]
    net, vae, nbytes = prepare(args.config, rank, device, args.ckpt, args.vae, with_vae=not args.no_vae,
                               allow_pickle=getattr(args, 'allow_pickle', False))
    label = args.category if cfg.get('num_classes') else None
    if cfg.get('num_classes') and label is None:
        label = 0
    mesh = getattr(args, 'mesh', False)
    if mesh:
        from .mesh import mesh_scale
    if mesh and (args.no_vae or not args.sdf_resolution):
        raise ValueError('--mesh needs the VAE and --sdf-resolution')
    points = getattr(args, 'points', None)
    if points is not None and (not mesh or points < 1):
        raise ValueError('--points needs --mesh and a positive count')
    clean = getattr(args, 'clean', False)
    if clean and not mesh:
        raise ValueError('--clean needs --mesh')
    simple = getattr(args, 'simplify', None)
    if simple is not None and not mesh:
        raise ValueError('--simplify needs --mesh')
    field = getattr(args, 'field_mesh', False)
    if field:
        from .mesh import FIELD_MAX_SIZE
        if not mesh:
            raise ValueError('--field-mesh needs --mesh')
        if not 2 <= args.sdf_resolution <= FIELD_MAX_SIZE or getattr(args, 'mesh_margin', 1) < 0:
            raise ValueError('--field-mesh needs 2 <= --sdf-resolution <= %d and --mesh-margin >= 0' % FIELD_MAX_SIZE)
    per_rank = len(dist.shard_indices(args.shapes, rank, world))
    batch = args.batch or max(1, min(8, per_rank))
    timings = {}
    done = []
    mesh_counts = {}
    mesh_comps = {}
    mesh_stats = {}
    simple_counts = {}
    checks = {}
    check = getattr(args, 'check', False)
    if check and not (mesh and args.out):
        raise ValueError('--check needs --mesh and --out')
    kw = dict(mesh=True, mesh_level=args.mesh_level, mesh_scale=mesh_scale(args.config), points=points) if mesh else {}
    if clean:
        kw['mesh_clean'] = True
    if simple is not None:
        kw['mesh_simplify'] = simple
    if field:
        kw['field_mesh'] = True
        kw['mesh_margin'] = getattr(args, 'mesh_margin', 1)
    smooth = getattr(args, 'smooth', None)
    if smooth is not None:
        if not mesh or not 0 <= smooth <= 10000:
            raise ValueError('--smooth needs --mesh and 0 <= K <= 10000')
        kw['mesh_smooth'] = smooth
    if getattr(args, 'smooth_normals', False):
        if smooth is None:
            raise ValueError('--smooth-normals needs --smooth')
        kw['smooth_normals'] = True
    if getattr(args, 'views', False):
        if not mesh or not args.out:
            raise ValueError('--views needs --mesh and --out')
        kw['views'] = True
        kw['view_size'] = getattr(args, 'view_size', 299)
        kw['view_samples'] = getattr(args, 'view_samples', 1)
    if getattr(args, 'octree_mesh', False):
        if not args.out:
            raise ValueError('--octree-mesh needs --out')
        kw['octree_mesh'] = True
    for idxs, out, dt in generate(net, cfg, args.shapes, rank, world, args.seed, args.steps, label, vae, args.out, batch,
                                  sdf_resolution=args.sdf_resolution, timings=timings, **kw):
        done.append((idxs, dt))
        for i, (v, f) in zip(idxs, out.get('meshes', ())):
            mesh_counts[i] = (int(v.shape[0]), int(f.shape[0]))
        for i, k in zip(idxs, out.get('mesh_components', ())):
            mesh_comps[i] = int(k)
        for i, (v, f) in zip(idxs, out.get('simple_meshes', ())):
            simple_counts[i] = (int(v.shape[0]), int(f.shape[0]))
        if check:
            from . import mesh_check
            written = out.get('simple_meshes', out['meshes'])
            for r in mesh_check.reports([('%d.obj' % i, m) for i, m in zip(idxs, written)]):
                checks[r['name']] = r
        for b, i in enumerate(idxs if 'mesh_stats' in out else ()):
            mesh_stats[i] = {k: int(v[b]) for k, v in out['mesh_stats'].items()}
    total = sum(dt for _, dt in done)
    tmax = dist.max_over_ranks(total, device)
    res = {'config': args.config, 'shapes': args.shapes, 'world': world, 'steps_per_stage': args.steps,
           'shapes_per_call': batch, 'weight_broadcast_bytes': nbytes, 'seconds_max_over_ranks': tmax,
           'seconds_per_shape': tmax * world / args.shapes if args.shapes else None,
           'shapes_per_s': args.shapes / tmax if tmax > 0 else None, 'rank0_indices': [i for g, _ in done for i in g],
           'rank0_phase_seconds': timings, 'sdf_resolution': args.sdf_resolution if vae is not None else None}
    if mesh:
        res['rank0_mesh_vertices'] = [mesh_counts[i][0] for i in res['rank0_indices']]
        res['rank0_mesh_faces'] = [mesh_counts[i][1] for i in res['rank0_indices']]
    if clean:
        res['rank0_mesh_components'] = [mesh_comps[i] for i in res['rank0_indices']]
    if field:
        res['mesh_margin'] = kw['mesh_margin']
        for k in ('seeds', 'bricks', 'leaks', 'total_bricks'):
            res['rank0_mesh_' + k] = [mesh_stats[i][k] for i in res['rank0_indices']]
    if simple is not None:
        res['rank0_simple_vertices'] = [simple_counts[i][0] for i in res['rank0_indices']]
        res['rank0_simple_faces'] = [simple_counts[i][1] for i in res['rank0_indices']]
    if check:
        res['rank0_mesh_check'] = [checks['%d.obj' % i] for i in res['rank0_indices']]
        if rank == 0:
            with open(os.path.join(args.out, 'mesh_check.json'), 'w') as fh:
                json.dump(res['rank0_mesh_check'], fh, indent=1)
    return res


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='snet_uncond', choices=sorted(configs.CONFIGS))
    ap.add_argument('--shapes', type=int, default=8)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=None, help='shapes per sample() call (default: min(8, shapes per rank))')
    ap.add_argument('--category', type=int, default=None, help='class label for the conditional config')
    ap.add_argument('--ckpt', default=None, help='df_*.pth (the EMA weights are used, as the reference does)')
    ap.add_argument('--vae', default=None, help='GraphVAE checkpoint (seeded random weights when absent)')
    ap.add_argument('--no-vae', action='store_true', help='stop after the last DDIM stage (no decode, no SDF)')
    ap.add_argument('--allow-pickle', action='store_true',
                    help='read the checkpoint files with the full unpickler (only for files you trust)')
    ap.add_argument('--sdf-resolution', type=int, default=256)
    ap.add_argument('--out', default=None)
    ap.add_argument('--mesh', action='store_true',
                    help='marching cubes on the device; writes <out>/<index>.obj (needs the VAE and --sdf-resolution)')
    ap.add_argument('--mesh-level', type=float, default=0.0, help='iso level of --mesh (the reference uses 0)')
    ap.add_argument('--points', type=int, default=None,
                    help='with --mesh: also write <out>/<index>.npy, that many surface points per shape after the '
                         'unit-cube normalisation (the input of python -m octfusion_amd.evaluate)')
    ap.add_argument('--clean', action='store_true',
                    help='with --mesh: keep only the largest connected component of every mesh (the reference\'s '
                         'export_mesh clean=True); the .obj, the --points cloud and the vertex / face counts are the '
                         'cleaned mesh\'s, and the result line gains rank0_mesh_components (counts before cleaning)')
    ap.add_argument('--field-mesh', action='store_true',
                    help='with --mesh: mesh the decoded field in octree-guided 8^3-cell bricks instead of sweeping the '
                         'lattice (mesh.field_mesh): --sdf-resolution may go up to 2048, no sdf.pt is written, and the '
                         'result line gains rank0_mesh_seeds / _bricks / _leaks / _total_bricks.  Surface sheets '
                         'inside coarse leaves, outside the band, are not meshed')
    ap.add_argument('--mesh-margin', type=int, default=1, metavar='M',
                    help='with --field-mesh: width of the band around the finest octree nodes, in finest-level cells')
    ap.add_argument('--simplify', type=int, default=None, metavar='N',
                    help='with --mesh: write <out>/<index>.obj simplified by vertex clustering on the device, N cells '
                         '(1 .. 1024) along the longest side of every mesh (the cleaned one under --clean); --points and '
                         '--views keep the full mesh, and the result line gains rank0_simple_vertices / _faces')
    ap.add_argument('--smooth', type=int, default=None, metavar='K',
                    help='with --mesh: K Taubin iterations (mesh_smooth.smooth: lambda 0.5, mu -0.53, uniform weights) '
                         'on every mesh, after --clean and before --simplify; the .obj, the clouds, the views and '
                         '--check are the smoothed mesh\'s')
    ap.add_argument('--smooth-normals', action='store_true',
                    help='with --smooth: write the angle-weighted vertex normals of every mesh as vn lines')
    ap.add_argument('--check', action='store_true',
                    help='with --mesh: check every written mesh on the device (mesh_check.check: closed, manifold, '
                         'oriented, self-intersections, ...) and write the reports of rank 0 to <out>/mesh_check.json; '
                         'the result line gains rank0_mesh_check; needs --out')
    ap.add_argument('--octree-mesh', action='store_true',
                    help='write the generated octree itself as a mesh of cubes, <out>/octree/<index>.obj (the '
                         'reference\'s export_octree) and, for a three-stage config, <out>/octree_large/<index>.obj; '
                         'needs --out, works with --no-vae')
    ap.add_argument('--views', action='store_true',
                    help='with --mesh: render every mesh (the cleaned one under --clean) from the 20 FID views on the '
                         'device and write <out>/fid_images/view_<j>/<index>.png, the image set of the reference\'s '
                         'generate_synth_image.py; needs --out')
    ap.add_argument('--view-size', type=int, default=299, help='image size of --views (Inception v3: 299)')
    ap.add_argument('--view-samples', type=int, default=1, choices=(1, 4, 16),
                    help='samples per pixel of --views (render.render samples=; 4 is recommended for FID image sets)')
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    if args.clean and not args.mesh:
        raise ValueError('--clean needs --mesh')
    if args.simplify is not None and not args.mesh:
        raise ValueError('--simplify needs --mesh')
    if args.field_mesh and not args.mesh:
        raise ValueError('--field-mesh needs --mesh')
    if args.smooth is not None and not args.mesh:
        raise ValueError('--smooth needs --mesh')
    if args.smooth_normals and args.smooth is None:
        raise ValueError('--smooth-normals needs --smooth')
    if args.views and not (args.mesh and args.out):
        raise ValueError('--views needs --mesh and --out')
    if args.octree_mesh and not args.out:
        raise ValueError('--octree-mesh needs --out')
    if args.check and not (args.mesh and args.out):
        raise ValueError('--check needs --mesh and --out')
    rank, local_rank, world = dist.init()
    from . import _lib
    _lib.require_device()
    torch.cuda.set_device(local_rank)
    res = run(args, rank, local_rank, world, torch.device('cuda', local_rank))
    if rank == 0:
        print(json.dumps(res))
    dist.barrier()
    return res


if __name__ == '__main__':
    main()
