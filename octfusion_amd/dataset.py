"""Training data of the GraphVAE from SDF lattices, on the device (csrc/ofx_sdfdata.hip), and the reference's dataset
folder read back into the arguments of ``vae_training.vae_stage_step``.

Replaces, from the lattice on (turning a mesh into a lattice -- the reference's mesh2sdf call -- is not here):
  * tools/repair_mesh.py: sample_sdf (:260-338 -> ``<name>/sdf.npz``), sample_occu (:341-378 -> ``<name>/points.npz``),
    generate_test_points (:381-413 -> ``test.input/<name>.ply``);
  * datasets/dualoctree_snet.py: ReadFile, TransformShape; datasets/utils.py: collate_func (``collate``);
  * models/octfusion_model_vae.py: batch_to_cuda + set_input (:135-160, ``to_device_batch``).

Differences a caller can observe:
  * the samplers draw from the project's counter hash of (seed, shape id, sample, axis), not from torch's / numpy's
    global generators: the files are a pure function of the lattice, the octree and the seed, bitwise reproducible, but
    not the reference's samples;
  * TransformShape takes a ``seed`` and chooses its random indices on the device (torch's device generator); what it
    returns already lives on the device;
  * to_device_batch builds the batch's input octree in one build (build_octree_batch) instead of one per shape + merge.

    python -m octfusion_amd.dataset --sdf-dir data/sdf --dataset-dir data/dataset [--names all.txt] [--occu]
        [--test-points]
"""
import argparse
import os
import zlib

import numpy as np
import torch

from . import _lib, mesh
from ._lib import call, ptr, stream
from .octree import Octree, Points, build_octree_batch

SHAPE_SCALE = 0.5          # tools/repair_mesh.py:36: the dataset's points live in [-0.5, 0.5]
U64 = 2 ** 64 - 1


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _lattice(sdf):
    """[S, S, S] fp32 contiguous on the device."""
    _lib.require_device()
    if not torch.is_tensor(sdf):
        sdf = torch.from_numpy(np.ascontiguousarray(sdf, np.float32))
    if sdf.dim() != 3 or not (sdf.shape[0] == sdf.shape[1] == sdf.shape[2]) or sdf.shape[0] < 2:
        raise ValueError('SDF lattice must be [S, S, S] with S >= 2, got %s' % (tuple(sdf.shape),))
    dev = sdf.device if sdf.device.type == 'cuda' else _device()
    return sdf.to(device=dev, dtype=torch.float32).contiguous()


def _uniforms(u, rows, dtype, dev, what):
    if u is None:
        return None
    if not torch.is_tensor(u):
        u = torch.from_numpy(np.ascontiguousarray(u))
    if u.numel() != rows * 3:
        raise ValueError('%s: u must hold [%d, 3] uniforms, got %s' % (what, rows, tuple(u.shape)))
    return u.to(device=dev, dtype=dtype).reshape(rows, 3).contiguous()


def sample_nodes(sdf, xyz, depth_off, depth_start, k=4, seed=0, shape_id=0, shape_scale=SHAPE_SCALE, u=None):
    """ofx_sdf_sample_nodes on explicit node coordinates: xyz [N, 3] int32 of consecutive depths from depth_start,
    depth-major; depth_off: where each depth begins (len = depths + 1).  See sample_sdf."""
    sdf = _lattice(sdf)
    dev = sdf.device
    S, k = int(sdf.shape[0]), int(k)
    if k < 1:
        raise ValueError('sample_sdf: k must be >= 1')
    xyz = torch.as_tensor(xyz).to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    N = int(xyz.shape[0])
    off = [int(o) for o in depth_off]
    if len(off) < 2 or off[0] != 0 or off[-1] != N or any(a > b for a, b in zip(off, off[1:])):
        raise ValueError('sample_sdf: depth_off %r does not partition %d nodes' % (off, N))
    offs = torch.tensor(off, dtype=torch.int64).to(dev)
    u = _uniforms(u, N * k, torch.float32, dev, 'sample_sdf')
    points = torch.empty(N * k, 3, dtype=torch.float16, device=dev)
    grad = torch.empty(N * k, 3, dtype=torch.float16, device=dev)
    val = torch.empty(N * k, dtype=torch.float16, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.lib().ofx_sdf_sample_ws_bytes(N, k), dtype=torch.uint8, device=dev)
    call('ofx_sdf_sample_nodes', ptr(sdf), S, ptr(xyz), N, ptr(offs), len(off) - 1, int(depth_start), k,
         int(seed) & U64, int(shape_id), ptr(u), float(shape_scale), ptr(ws), ptr(points), ptr(grad), ptr(val),
         ptr(count), stream())
    n = int(count.item())                                  # the one host read
    return {'points': points[:n], 'grad': grad[:n], 'sdf': val[:n]}


def sample_sdf(sdf, octree, full_depth, depth, k=4, seed=0, shape_id=0, shape_scale=SHAPE_SCALE, u=None):
    """The reference's sample_sdf (tools/repair_mesh.py:293-334) for one shape: k random points in every node of
    ``octree`` at depths full_depth..depth, scaled onto the lattice ``sdf`` [S, S, S]; samples with a coordinate
    >= S - 1 are dropped; value and normalised gradient are interpolated from the eight surrounding lattice values.
    Returns dict(points [n, 3], grad [n, 3], sdf [n]): fp16 device tensors, points in [-shape_scale, shape_scale], in
    the reference's order (depth, node, sample).  u: optional [N*k, 3] fp32 uniforms in [0, 1) replacing the draw from
    ofx_metrics_hash(seed, shape_id, i*k + j, axis).  One host read (the kept count)."""
    if octree.batch_size != 1:
        raise ValueError('sample_sdf: one shape per octree, got batch size %d' % octree.batch_size)
    xyz, off = [], [0]
    for d in range(full_depth, depth + 1):
        x, y, z, _ = octree.xyzb(d)
        xyz.append(torch.stack([x, y, z], dim=1).to(torch.int32))
        off.append(off[-1] + int(x.shape[0]))
    return sample_nodes(sdf, torch.cat(xyz), off, full_depth, k, seed, shape_id, shape_scale, u)


def sample_occu(sdf, n=100000, seed=0, shape_id=0, shape_scale=SHAPE_SCALE, u=None):
    """The reference's sample_occu (tools/repair_mesh.py:358-375): n uniform points in [0, (S-1)/S)^3 of the lattice
    cube, their trilinear SDF value in fp64, occupancy = value < 0.  Returns dict(points [n, 3] fp16 in
    [-shape_scale, shape_scale), occupancies [ceil(n/8)] uint8 packed as numpy.packbits) on the device.  u: optional
    [n, 3] fp64 uniforms replacing (ofx_metrics_hash(seed, shape_id, i, axis) >> 11) * 2^-53."""
    sdf = _lattice(sdf)
    dev = sdf.device
    n = int(n)
    if n < 0:
        raise ValueError('sample_occu: n must be >= 0')
    u = _uniforms(u, n, torch.float64, dev, 'sample_occu')
    points = torch.empty(n, 3, dtype=torch.float16, device=dev)
    bits = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
    call('ofx_sdf_sample_occu', ptr(sdf), int(sdf.shape[0]), n, int(seed) & U64, int(shape_id), ptr(u),
         float(shape_scale), ptr(points), ptr(bits), stream())
    return {'points': points, 'occupancies': bits}


def _generator(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    return g


def noisy_points(points, n=3000, std=0.005, seed=0):
    """The reference's generate_test_points (tools/repair_mesh.py:397-402): n points chosen with replacement from
    ``points`` [m, 3] plus N(0, std^2) noise -> [n, 3] fp32 on the device (torch's device generator, seeded)."""
    _lib.require_device()
    if not torch.is_tensor(points):
        points = torch.from_numpy(np.asarray(points, np.float32))
    dev = points.device if points.device.type == 'cuda' else _device()
    points = points.to(device=dev, dtype=torch.float32).reshape(-1, 3)
    if points.shape[0] == 0:
        raise ValueError('noisy_points: no points to choose from')
    g = _generator(dev, seed)
    idx = torch.randint(points.shape[0], (int(n),), generator=g, device=dev)
    return points[idx] + std * torch.randn(int(n), 3, generator=g, device=dev)


# ---------------------------------------------------------------------------------------------------- files
def _np(t, dtype):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.dtype != dtype:
        raise ValueError('expected %s, got %s' % (np.dtype(dtype), a.dtype))
    return a


def write_sdf_npz(path, samples):
    """``sdf.npz`` as the reference writes it (tools/repair_mesh.py:338): points [n, 3], grad [n, 3], sdf [n], fp16."""
    np.savez(path, points=_np(samples['points'], np.float16).reshape(-1, 3),
             grad=_np(samples['grad'], np.float16).reshape(-1, 3), sdf=_np(samples['sdf'], np.float16).reshape(-1))


def write_occu_npz(path, samples):
    """``points.npz`` (tools/repair_mesh.py:378): points [n, 3] fp16, occupancies [ceil(n/8)] uint8."""
    np.savez(path, points=_np(samples['points'], np.float16).reshape(-1, 3),
             occupancies=_np(samples['occupancies'], np.uint8).reshape(-1))


def shape_id(name):
    """The id keying a shape's random numbers: a CRC of its name, so a shape gets the same samples in any list."""
    return zlib.crc32(name.replace(os.sep, '/').encode())


def prepare_shape(sdf_file, shape_dir, name, depth=6, full_depth=4, k=4, seed=0, shape_scale=SHAPE_SCALE, occu=False,
                  occu_points=100000, test_ply=None, test_points=3000, noise_std=0.005):
    """What the three reference functions do for one shape: read the lattice ``sdf_file`` (.npy) and
    ``shape_dir/pointcloud.npz``, build the shape's octree from the cloud (points / shape_scale, as
    tools/repair_mesh.py:284-291) and write ``shape_dir/sdf.npz``; with occu, ``shape_dir/points.npz``; with test_ply,
    that file.  Outputs that exist are left alone.  Returns the list of files written."""
    written = []
    out_sdf = os.path.join(shape_dir, 'sdf.npz')
    out_occu = os.path.join(shape_dir, 'points.npz')
    need = [not os.path.exists(out_sdf), occu and not os.path.exists(out_occu),
            test_ply is not None and not os.path.exists(test_ply)]
    if not any(need):
        return written
    dev = _device()
    sid = shape_id(name)
    with np.load(os.path.join(shape_dir, 'pointcloud.npz')) as z:
        pts = torch.from_numpy(np.asarray(z['points'], np.float32)).to(dev)
        nrm = torch.from_numpy(np.asarray(z['normals'], np.float32)).to(dev)
    sdf = _lattice(np.load(sdf_file)) if need[0] or need[1] else None
    if need[0]:
        cloud = Points(pts / shape_scale, nrm)
        cloud.clip(min=-1, max=1)
        octree = Octree(depth, full_depth, 1, dev).build_octree(cloud)
        write_sdf_npz(out_sdf, sample_sdf(sdf, octree, full_depth, depth, k, seed, sid, shape_scale))
        written.append(out_sdf)
    if need[1]:
        write_occu_npz(out_occu, sample_occu(sdf, occu_points, seed, sid, shape_scale))
        written.append(out_occu)
    if need[2]:
        mesh.write_ply(test_ply, noisy_points(pts, test_points, noise_std, (int(seed) + sid) & (2 ** 63 - 1)))
        written.append(test_ply)
    return written


# ---------------------------------------------------------------------------------------------------- loading
def _flag(flags, name, default=None):
    if isinstance(flags, dict):
        return flags.get(name, default)
    return getattr(flags, name, default)


_UNSUPPORTED = ('load_octree', 'load_split_small', 'load_split_large', 'load_color')


class ReadFile:
    """datasets/dualoctree_snet.py:110-168 for the files this project writes or reads: ``flags`` (a dict or an object
    with attributes) turns on load_pointcloud (pointcloud.npz), load_sdf (sdf.npz) and load_occu (points.npz).  The
    reference's other loaders (octree.pth, split_*.pth, color.npz) have no counterpart and raise when asked for."""

    def __init__(self, flags):
        for name in _UNSUPPORTED:
            if _flag(flags, name, False):
                raise ValueError('ReadFile: %s is not supported' % name)
        self.load_pointcloud = bool(_flag(flags, 'load_pointcloud', False))
        self.load_occu = bool(_flag(flags, 'load_occu', False))
        self.load_sdf = bool(_flag(flags, 'load_sdf', False))

    def __call__(self, filename):
        output = {}
        if self.load_pointcloud:
            with np.load(os.path.join(filename, 'pointcloud.npz')) as raw:
                output['point_cloud'] = {'points': raw['points'], 'normals': raw['normals'], 'colors': None}
        if self.load_occu:
            with np.load(os.path.join(filename, 'points.npz')) as raw:
                output['occu'] = {'points': raw['points'], 'occupancies': raw['occupancies']}
        if self.load_sdf:
            with np.load(os.path.join(filename, 'sdf.npz')) as raw:
                output['sdf'] = {'points': raw['points'], 'grad': raw['grad'], 'sdf': raw['sdf']}
        return output


class TransformShape:
    """datasets/dualoctree_snet.py:19-107: a ReadFile sample -> {'points': Points in [-1, 1]^3, 'pos', 'sdf', 'grad'}.
    Flags: depth, full_depth, point_scale, point_sample_num, load_pointcloud, load_sdf, sample_surf_points.  The random
    index choices (with replacement, as np.random.choice) come from torch's device generator seeded with ``seed`` and
    the sample's index: a shape's draw does not depend on what was loaded before it.  Tensors live on ``device``
    (default: the current HIP device; 'cpu' keeps everything on the host, e.g. in a loader worker)."""

    def __init__(self, flags, seed=0, device=None):
        for name in _UNSUPPORTED:
            if _flag(flags, name, False):
                raise ValueError('TransformShape: %s is not supported' % name)
        self.flags = flags
        self.depth = _flag(flags, 'depth')
        self.full_depth = _flag(flags, 'full_depth')
        self.point_sample_num = int(_flag(flags, 'point_sample_num'))
        self.point_scale = float(_flag(flags, 'point_scale'))
        self.noise_std = 0.005
        self.seed = int(seed)
        self.device = None if device is None else torch.device(device)

    def _dev(self):
        if self.device is None:
            _lib.require_device()
            self.device = _device()
        return self.device

    def _tensor(self, a):
        return torch.from_numpy(np.asarray(a)).to(self._dev()).float()

    def _choice(self, n, g):
        return torch.randint(n, (self.point_sample_num,), generator=g, device=self._dev())

    def process_points_cloud(self, sample):
        points_gt = Points(self._tensor(sample['points']) / self.point_scale, self._tensor(sample['normals']))
        points_gt.clip(min=-1, max=1)
        return {'points': points_gt}

    def sample_sdf(self, sample, g):
        points = self._tensor(sample['points']) / self.point_scale
        rand_idx = self._choice(points.shape[0], g)
        return {'pos': points[rand_idx], 'sdf': self._tensor(sample['sdf'])[rand_idx],
                'grad': self._tensor(sample['grad'])[rand_idx]}

    def sample_on_surface(self, points, normals, g):
        rand_idx = self._choice(points.shape[0], g)
        return {'pos': self._tensor(points)[rand_idx], 'sdf': torch.zeros(self.point_sample_num, device=self._dev()),
                'grad': self._tensor(normals)[rand_idx]}

    def sample_off_surface(self, xyz, g):
        xyz = self._tensor(xyz) / self.point_scale
        xyz = xyz[self._choice(xyz.shape[0], g)]
        grad = xyz / (xyz.norm(p=2, dim=1, keepdim=True) + 1.0e-6)
        return {'pos': xyz, 'sdf': -torch.ones(self.point_sample_num, device=self._dev()), 'grad': grad}

    def __call__(self, sample, idx):
        g = _generator(self._dev(), (self.seed * 1000003 + int(idx)) & (2 ** 63 - 1))
        output = {}
        if _flag(self.flags, 'load_pointcloud', False):
            output = self.process_points_cloud(sample['point_cloud'])
        if _flag(self.flags, 'load_sdf', False):
            output.update(self.sample_sdf(sample['sdf'], g))
        if _flag(self.flags, 'sample_surf_points', False):
            # the reference reads sample['points'] / sample['normals'] here, keys its ReadFile never sets
            # (dualoctree_snet.py:99): the cloud of 'point_cloud' is what it means, unscaled as there
            cloud = sample['point_cloud']
            on_surf = self.sample_on_surface(cloud['points'], cloud['normals'], g)
            off_surf = self.sample_off_surface(sample['sdf']['points'], g)
            output.update({key: torch.cat([on_surf[key], off_surf[key]], dim=0) for key in ('pos', 'grad', 'sdf')})
        return output


def collate(batch):
    """datasets/utils.py:13-35 (CollateBatch(merge_points=False) + collate_func): a list of per-shape dicts -> a dict of
    lists; 'pos' becomes one [n, 4] tensor whose last column is the shape's position in the batch, 'grad' / 'sdf' /
    'occu' / 'weight' are concatenated."""
    output = {}
    for sample in batch:
        for key, val in sample.items():
            output.setdefault(key, []).append(val)
    if 'pos' in output:
        pos = output['pos']
        batch_idx = torch.cat([torch.full((p.shape[0], 1), float(i), dtype=p.dtype, device=p.device)
                               for i, p in enumerate(pos)], dim=0)
        output['pos'] = torch.cat([torch.cat(pos, dim=0), batch_idx], dim=1)
    for key in ('grad', 'sdf', 'occu', 'weight'):
        if key in output:
            output[key] = torch.cat(output[key], dim=0)
    return output


def to_device_batch(batch, cfg):
    """batch_to_cuda + set_input (models/octfusion_model_vae.py:135-160) on a collated batch: the shapes' clouds become
    one input octree (build_octree_batch at cfg['depth'] / cfg['full_depth']) and its dual octree, which is also the
    ground-truth side (the reference deep-copies octree_in).  Returns the keyword arguments of
    ``vae_training.vae_stage_step(vae, opt, **args)``: data, doctree_in, doctree_out, pos [n, 4], sdf_gt, grad_gt."""
    from .dual_octree import DualOctree
    _lib.require_device()
    dev = _device()
    clouds = [p.to(dev) for p in batch['points']]
    octree_in = build_octree_batch(clouds, int(cfg['depth']), int(cfg['full_depth']))
    doctree = DualOctree(octree_in)
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
    return {'data': doctree.get_input_feature(), 'doctree_in': doctree, 'doctree_out': doctree,
            'pos': f32(batch['pos']), 'sdf_gt': f32(batch['sdf']).reshape(-1), 'grad_gt': f32(batch['grad'])}


# ---------------------------------------------------------------------------------------------------- driver
def list_names(sdf_dir, names_file=None):
    """Shape names: the lines of names_file (first word of each), or every ``<name>.npy`` below sdf_dir."""
    if names_file:
        with open(names_file) as fh:
            return [ln.split()[0] for ln in fh if ln.strip()]
    names = []
    for dirpath, dirnames, files in os.walk(sdf_dir):
        dirnames.sort()
        for f in sorted(files):
            if f.endswith('.npy'):
                names.append(os.path.relpath(os.path.join(dirpath, f[:-4]), sdf_dir).replace(os.sep, '/'))
    return names


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.dataset', description=__doc__.split('\n\n')[0])
    ap.add_argument('--sdf-dir', required=True, help='holds <name>.npy: [S, S, S] SDF lattices over [-1, 1]^3')
    ap.add_argument('--dataset-dir', required=True, help='holds <name>/pointcloud.npz; receives <name>/sdf.npz')
    ap.add_argument('--names', default=None, metavar='FILE', help='one shape name per line (default: all of --sdf-dir)')
    ap.add_argument('--occu', action='store_true', help='also write <name>/points.npz (100000 occupancy samples)')
    ap.add_argument('--test-points', action='store_true', help='also write test.input/<name>.ply (3000 noisy points)')
    ap.add_argument('--test-dir', default=None, help='where the .ply files go (default: test.input beside --dataset-dir)')
    ap.add_argument('--depth', type=int, default=6)
    ap.add_argument('--full-depth', type=int, default=4)
    ap.add_argument('--samples', type=int, default=4, help='samples per octree node')
    ap.add_argument('--seed', type=int, default=0)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    _lib.require_device()
    test_dir = args.test_dir or os.path.join(os.path.dirname(os.path.normpath(args.dataset_dir)), 'test.input')
    done = skipped = 0
    for name in list_names(args.sdf_dir, args.names):
        sdf_file = os.path.join(args.sdf_dir, name + '.npy')
        shape_dir = os.path.join(args.dataset_dir, name)
        if not os.path.exists(sdf_file) or not os.path.exists(os.path.join(shape_dir, 'pointcloud.npz')):
            skipped += 1
            continue
        ply = os.path.join(test_dir, name + '.ply') if args.test_points else None
        done += bool(prepare_shape(sdf_file, shape_dir, name, args.depth, args.full_depth, args.samples, args.seed,
                                   occu=args.occu, test_ply=ply))
    print('dataset: %d shapes written, %d without a lattice or a point cloud' % (done, skipped))


if __name__ == '__main__':
    main()
