"""Evaluation metrics of generated shapes on the device (csrc/ofx_metrics.hip): surface sampling, Chamfer and
approximate-EMD matrices, and the reference's reductions COV / MMD and 1-NNA.

Replaces the reference's metrics/ package: generate_pointclouds.py (scale_to_unit_cube, then trimesh's mesh.sample
of 2048 points), evaluation_metrics.py (_pairwise_EMD_CD_ over the nndistance / approxmatch CUDA extension,
lgan_mmd_cov, knn, compute_cov_mmd, compute_1_nna) and its drivers cov_mmd.py / 1-NNA.py.

Differences a caller can observe:
  * the sampler draws its random numbers from the project's counter hash of (seed, shape id, point, draw), not from
    numpy's generator: the points are a pure function of the meshes and the seed, bitwise reproducible, but they are
    not trimesh's points;
  * each distance matrix is computed once, in one launch, instead of per sample against 256-shape batches, and the
    reductions run in float64 on the device;
  * EMD needs n == m <= 2048 points per cloud (the reference protocol; both clouds live in LDS).
"""
import numpy as np
import torch

from . import _lib

EMD_MAX_POINTS = 2048        # include/ofx.h OFX_EMD_MAX_POINTS


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _clouds(X, what):
    """[N, n, 3] float32 contiguous on the device."""
    _lib.require_device()
    if not torch.is_tensor(X):
        X = torch.from_numpy(np.asarray(X, np.float32))
    if X.dim() != 3 or X.shape[2] != 3 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('%s: point clouds must be [N, n, 3] with N, n >= 1, got %s' % (what, tuple(X.shape)))
    dev = X.device if X.device.type == 'cuda' else _device()
    return X.to(device=dev, dtype=torch.float32).contiguous()


def sample_surface(meshes, n=2048, seed=0, normalize=True, ids=None, normals=False):
    """[B, n, 3] float32 device tensor of points drawn uniformly by area from each mesh of ``meshes``: the list that
    ``mesh.marching_cubes`` returns, or ``(verts, faces)`` pairs as ``mesh.read_obj`` reads them (numpy or tensors,
    faces 0-based).  normalize: first map each mesh to (v - bbox centre) * 2 / max bbox extent, as the reference's
    scale_to_unit_cube (padding 0) does before trimesh's mesh.sample.  ids: one int per mesh keying its random
    numbers (default: the position in the list), so a shape gets the same points in any batch.  normals: return
    ``(points, normals)``, normals [B, n, 3] = the unit face normal (B - A) x (C - A) / |.| of the triangle each point
    was drawn from (ofx_surface_sample_oriented; the points are the same bits) -- the oriented cloud the VAE encoder
    takes.  Raises ValueError naming the shape for a mesh without faces or with an out-of-range index."""
    _lib.require_device()
    if int(n) < 1:
        raise ValueError('sample_surface: n must be >= 1')
    meshes = list(meshes)
    if not meshes:
        raise ValueError('sample_surface: no meshes')
    if ids is not None and len(ids) != len(meshes):
        raise ValueError('sample_surface: %d ids for %d meshes' % (len(ids), len(meshes)))
    dev = _device()
    vs, fs = [], []
    for k, (v, f) in enumerate(meshes):
        v = (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v, np.float32))).reshape(-1, 3)
        f = (f if torch.is_tensor(f) else torch.from_numpy(np.asarray(f, np.int64))).reshape(-1, 3)
        if f.shape[0] == 0:
            raise ValueError('sample_surface: shape %d has no faces' % k)
        vs.append(v.to(device=dev, dtype=torch.float32))
        fs.append(f.to(device=dev, dtype=torch.int32))
    nv = [int(v.shape[0]) for v in vs]
    nf = [int(f.shape[0]) for f in fs]
    rng = torch.stack([torch.stack([f.min(), f.max()]) for f in fs]).cpu()        # one host sync
    for k in range(len(fs)):
        if int(rng[k, 0]) < 0 or int(rng[k, 1]) >= nv[k]:
            raise ValueError('sample_surface: shape %d has a face index outside [0, %d)' % (k, nv[k]))
    B = len(meshes)
    voff = np.cumsum([0] + nv[:-1])
    foff = np.cumsum([0] + nf[:-1])
    offs = torch.tensor(np.concatenate([voff, nv, foff, nf]), dtype=torch.int64).to(dev)
    idt = None if ids is None else torch.tensor([int(i) for i in ids], dtype=torch.int64).to(dev)
    V = torch.cat(vs).contiguous()
    F = torch.cat(fs).contiguous()
    T = int(sum(nf))
    ws = torch.empty(_lib.lib().ofx_surface_sample_ws_bytes(B, T), dtype=torch.uint8, device=dev)
    out = torch.empty(B, int(n), 3, dtype=torch.float32, device=dev)
    args = (_lib.ptr(V), _lib.ptr(F), _lib.ptr(offs), _lib.ptr(idt), B, T, int(n), int(seed) & (2 ** 64 - 1),
            1 if normalize else 0, _lib.ptr(ws), _lib.ptr(out))
    if not normals:
        _lib.call('ofx_surface_sample', *args, _lib.stream())
        return out
    nrm = torch.empty_like(out)
    _lib.call('ofx_surface_sample_oriented', *args, _lib.ptr(nrm), _lib.stream())
    return out, nrm


def nn_matrix(A, B):
    """Directed [NA, NB]: D[i, j] = mean over the points p of A[i] of min over B[j] of |p - q|^2 (one launch)."""
    A, B = _clouds(A, 'nn_matrix'), _clouds(B, 'nn_matrix')
    D = torch.empty(A.shape[0], B.shape[0], dtype=torch.float32, device=A.device)
    _lib.call('ofx_nn_matrix', _lib.ptr(A), A.shape[0], A.shape[1], _lib.ptr(B), B.shape[0], B.shape[1], _lib.ptr(D),
              _lib.stream())
    return D


def chamfer_matrix(X, Y=None):
    """[NX, NY] Chamfer distances CD[i, j] = D(X[i] -> Y[j]) + D(Y[j] -> X[i]), the reference's
    ``dl.mean(1) + dr.mean(1)`` (squared distances, evaluation_metrics.py:133-137).  Y=None: the self matrix, from ONE
    launch (diagonal exactly 0, exactly symmetric)."""
    X = _clouds(X, 'chamfer_matrix')
    if Y is None:
        D = nn_matrix(X, X)
        return D + D.t()
    Y = _clouds(Y, 'chamfer_matrix')
    return nn_matrix(X, Y) + nn_matrix(Y, X).t()


def emd_matrix(X, Y=None):
    """[NX, NY] approximate EMD: E[i, j] = approxmatch cost of (xyz1 = X[i], xyz2 = Y[j]) / n, the reference's
    ``emd_approx_cuda(X[i], Y[j])`` (evaluation_metrics.py:57-62).  Not symmetric.  Y=None: X against itself.
    Needs the same n for both sets and n <= 2048."""
    X = _clouds(X, 'emd_matrix')
    Y = X if Y is None else _clouds(Y, 'emd_matrix')
    n, m = int(X.shape[1]), int(Y.shape[1])
    if n != m:
        raise ValueError('emd_matrix: clouds of %d and %d points (the approximate EMD needs n == m)' % (n, m))
    if n > EMD_MAX_POINTS:
        raise ValueError('emd_matrix: %d points per cloud, at most %d' % (n, EMD_MAX_POINTS))
    E = torch.empty(X.shape[0], Y.shape[0], dtype=torch.float32, device=X.device)
    _lib.call('ofx_emd_matrix', _lib.ptr(X), X.shape[0], _lib.ptr(Y), Y.shape[0], n, m, _lib.ptr(E), _lib.stream())
    return E


# ---------------------------------------------------------------------------------------------------- reductions
def lgan_mmd_cov(all_dist):
    """The reference's lgan_mmd_cov (evaluation_metrics.py:189-201) of an [N_sample, N_ref] matrix, in float64."""
    d = all_dist.double()
    min_val_fromsmp, min_idx = torch.min(d, dim=1)
    min_val = torch.min(d, dim=0).values
    return {'lgan_mmd': float(min_val.mean()),
            'lgan_cov': float(min_idx.unique().numel()) / float(d.shape[1]),
            'lgan_mmd_smp': float(min_val_fromsmp.mean())}


def knn(Mxx, Mxy, Myy, k=1):
    """The reference's knn (evaluation_metrics.py:157-186, sqrt=False) in float64: label 1 for the n0 rows of Mxx,
    the diagonal excluded through +inf, each column's k nearest rows vote.  Returns acc, acc_t, acc_f."""
    Mxx, Mxy, Myy = Mxx.double(), Mxy.double(), Myy.double()
    n0, n1 = Mxx.shape[0], Myy.shape[0]
    label = torch.cat([torch.ones(n0), torch.zeros(n1)]).to(Mxx)
    M = torch.cat([torch.cat([Mxx, Mxy], 1), torch.cat([Mxy.t(), Myy], 1)], 0)
    M = M + torch.diag(torch.full((n0 + n1,), float('inf'), dtype=M.dtype, device=M.device))
    _, idx = M.topk(k, 0, False)
    count = label[idx].sum(0)
    pred = (count >= float(k) / 2).to(Mxx)
    tp = float((pred * label).sum())
    fp = float((pred * (1 - label)).sum())
    fn = float(((1 - pred) * label).sum())
    tn = float(((1 - pred) * (1 - label)).sum())
    return {'acc_t': tp / (tp + fn + 1e-10), 'acc_f': tn / (tn + fp + 1e-10),
            'acc': float((label == pred).sum()) / float(n0 + n1)}


def _named(res, fmt):
    return {fmt % k: v for k, v in res.items()}


def cov_mmd(sample, ref, emd=True):
    """compute_cov_mmd (evaluation_metrics.py:204-218): lgan_mmd-CD, lgan_cov-CD, lgan_mmd_smp-CD (and -EMD) of the
    [sample, ref] matrices (the reference's M_rs.t(); EMD with the reference clouds as xyz1)."""
    S, R = _clouds(sample, 'cov_mmd'), _clouds(ref, 'cov_mmd')
    res = _named(lgan_mmd_cov(chamfer_matrix(S, R)), '%s-CD')
    if emd:
        res.update(_named(lgan_mmd_cov(emd_matrix(R, S).t()), '%s-EMD'))
    return res


def one_nna(sample, ref, emd=True):
    """compute_1_nna (evaluation_metrics.py:221-238): 1-NN-CD-acc, -acc_t, -acc_f (and 1-NN-EMD-*), references
    labelled 1.  Chamfer: one launch over the union refs + samples."""
    S, R = _clouds(sample, 'one_nna'), _clouds(ref, 'one_nna')
    return _evaluate(S, R, emd, with_cov=False, truncate=False)


def evaluate(sample, ref, emd=True):
    """Both drivers at once, as metrics/cov_mmd.py and metrics/1-NNA.py run them: COV / MMD over all samples, 1-NNA
    over the first len(ref) samples.  Each matrix is built once: Chamfer in one launch over the union refs + samples,
    EMD as refs x union (M_rr and M_rs) plus samples x samples -- exactly the ordered pairs the reference's three
    _pairwise_EMD_CD_ calls compute.  Returns the reference's twelve keys (six with emd=False) as floats."""
    S, R = _clouds(sample, 'evaluate'), _clouds(ref, 'evaluate')
    return _evaluate(S, R, emd, with_cov=True, truncate=True)


def _evaluate(S, R, emd, with_cov, truncate):
    nr, ns = int(R.shape[0]), int(S.shape[0])
    t = min(ns, nr) if truncate else ns
    U = torch.cat([R, S])
    CD = chamfer_matrix(U)
    res = {}
    if with_cov:
        res.update(_named(lgan_mmd_cov(CD[nr:, :nr]), '%s-CD'))
    res.update(_named(knn(CD[:nr, :nr], CD[:nr, nr:nr + t], CD[nr:nr + t, nr:nr + t]), '1-NN-CD-%s'))
    if emd:
        E_ru = emd_matrix(R, U)
        E_ss = emd_matrix(S[:t])
        if with_cov:
            res.update(_named(lgan_mmd_cov(E_ru[:, nr:].t()), '%s-EMD'))
        res.update(_named(knn(E_ru[:, :nr], E_ru[:, nr:nr + t], E_ss), '1-NN-EMD-%s'))
    return res
