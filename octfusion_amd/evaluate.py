"""Score generated shapes against references: COV / MMD and 1-NNA with Chamfer and approximate EMD, on the device.

The reference runs metrics/generate_pointclouds.py (meshes -> 2048-point .npy clouds), then metrics/cov_mmd.py and
metrics/1-NNA.py on .pth tensors.  This driver does all three (octfusion_amd.metrics):

    python -m octfusion_amd.evaluate --samples PATH --refs PATH [--points 2048] [--seed 0] [--no-emd] [--clean]
                                     [--out metrics.json]

A PATH is a directory of .obj files (sampled on the device after the unit-cube normalisation, --points per shape),
a directory of .npy [n, 3] clouds (what generate_pointclouds.py and ``generate --points`` write), or a .pt / .pth
tensor [N, n, 3] (like the reference's chair_sample_pcs.pth).  As 1-NNA.py does, 1-NNA uses the first len(refs)
samples.  Prints one JSON line with the reference's keys and writes it to --out when given.
"""
import argparse
import json
import os

import numpy as np
import torch

SAMPLE_GROUP = 64            # meshes per sample_surface call


def load_clouds(path, points=2048, seed=0, clean=False):
    """[N, n, 3] float32 (device for OBJ input, host otherwise) from a PATH as described in the module docstring.
    clean: keep only the largest component of every mesh read from .obj (mesh.largest_component) before sampling;
    no effect on .npy / .pt input."""
    from . import mesh, metrics
    if os.path.isdir(path):
        names = sorted(os.listdir(path))
        objs = [f for f in names if f.endswith('.obj')]
        npys = [f for f in names if f.endswith('.npy')]
        if objs and npys:
            raise ValueError('%s holds both .obj and .npy files' % path)
        if objs:
            meshes = []
            for f in objs:
                v, fc = mesh.read_obj(os.path.join(path, f))
                if len(fc) == 0:
                    raise ValueError('%s has no faces' % os.path.join(path, f))
                meshes.append((v, fc))
            if clean:
                meshes = clean_meshes(meshes)
            parts = [metrics.sample_surface(meshes[g:g + SAMPLE_GROUP], n=points, seed=seed,
                                            ids=list(range(g, g + len(meshes[g:g + SAMPLE_GROUP]))))
                     for g in range(0, len(meshes), SAMPLE_GROUP)]
            return torch.cat(parts)
        if npys:
            clouds = [np.load(os.path.join(path, f)) for f in npys]
            if len({c.shape for c in clouds}) != 1 or clouds[0].ndim != 2 or clouds[0].shape[1] != 3:
                raise ValueError('%s: the .npy clouds must all be [n, 3] with one n' % path)
            return torch.from_numpy(np.stack(clouds).astype(np.float32))
        raise ValueError('%s holds no .obj or .npy files' % path)
    if path.endswith(('.pt', '.pth')):
        t = torch.load(path, map_location='cpu', weights_only=True)
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError('%s: expected a tensor [N, n, 3]' % path)
        return t.to(torch.float32)
    raise ValueError('%s: not a directory, .pt or .pth file' % path)


def clean_meshes(meshes):
    """The largest component of every host (verts, faces) pair, as device tensors (mesh.largest_component)."""
    from . import mesh, metrics
    dev = metrics._device()
    out = []
    for g in range(0, len(meshes), SAMPLE_GROUP):
        out += mesh.largest_component([(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
                                       for v, f in meshes[g:g + SAMPLE_GROUP]])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', required=True)
    ap.add_argument('--refs', required=True)
    ap.add_argument('--points', type=int, default=2048, help='points per shape sampled from .obj input')
    ap.add_argument('--seed', type=int, default=0, help='seed of the surface sampler')
    ap.add_argument('--no-emd', action='store_true', help='Chamfer only')
    ap.add_argument('--clean', action='store_true',
                    help='keep only the largest connected component of every mesh loaded from .obj before sampling '
                         '(the reference\'s clean=True); no effect on .npy, .pt or .pth input')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    from . import _lib, metrics
    _lib.require_device()
    sample = load_clouds(args.samples, args.points, args.seed, args.clean)
    ref = load_clouds(args.refs, args.points, args.seed, args.clean)
    res = metrics.evaluate(sample, ref, emd=not args.no_emd)
    line = json.dumps(res)
    print(line)
    if args.out:
        d = os.path.dirname(args.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
