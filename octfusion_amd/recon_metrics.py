"""Reconstruction scores on the device: the table of the occupancy-network / dual-octree line of work -- Chamfer-L1
and -L2, F-score at a few thresholds, normal consistency and volumetric IoU -- on top of an exact nearest-neighbour
search that reports which point was nearest (csrc/ofx_nnsearch.hip, ``ofx_nn_search``).

* ``nearest``          per query point the squared distance to, and the index of, its nearest target point, for a batch
                       of ragged cloud pairs in one call; the target cloud of a pair is cut into slices over the chip,
                       so one pair of 100 000-point clouds fills the device (metrics.nn_matrix runs it on one block).
* ``surface_scores``   completeness / accuracy, Chamfer, normal consistency and precision / recall / F-score of two
                       oriented clouds or meshes.
* ``occupancy_iou``    IoU of the SDF field's occupancy against the packed occupancies of ``points.npz``
                       (dataset.sample_occu / write_occu_npz).

tests/recon_metrics_oracle.py restates all three in numpy float64.  There is no CPU path.
"""
import numpy as np
import torch

from . import _lib, metrics

THRESHOLDS = (0.01, 0.015, 0.02)      # the F-score thresholds the occupancy-network papers report, in file units


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _cloud_list(X, what, dev):
    """(list of [n_i, 3] float32 contiguous device tensors, X was one [N, n, 3] tensor)."""
    stacked = torch.is_tensor(X) or isinstance(X, np.ndarray)
    if stacked:
        X = torch.as_tensor(X)
        if X.dim() != 3 or X.shape[2] != 3:
            raise ValueError('%s: a stacked batch must be [N, n, 3], got %s' % (what, tuple(X.shape)))
    out = []
    for k, x in enumerate(X):
        x = torch.as_tensor(x)
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError('%s: cloud %d must be [n, 3], got %s' % (what, k, tuple(x.shape)))
        out.append(x.to(device=dev, dtype=torch.float32))
    return out, stacked


def nearest(A, B, splits=0):
    """Exact nearest neighbours of the points of A[i] among the points of B[i], for every pair i in one call.

    A, B: lists of [n_i, 3] / [m_i, 3] tensors (ragged; a cloud may be empty), or one [N, n, 3] / [N, m, 3] tensor each.
    Returns (dist2, idx): per pair dist2 [n_i] float32 = min_j |a - b_j|^2 from direct fp32 differences and idx [n_i]
    int32 = the lowest j that attains it (+inf and -1 against an empty B[i]); lists for list inputs, [N, n] tensors
    for stacked ones.  The result is bitwise the same for every ``splits`` (slices per target cloud; 0: chosen so
    that the call fills the device, k >= 1: forced) and every repeat."""
    _lib.require_device()
    on_dev = [x.device for X in (A, B) for x in ([X] if torch.is_tensor(X) else X)
              if torch.is_tensor(x) and x.device.type == 'cuda']
    dev = on_dev[0] if on_dev else _device()
    qa, stacked_a = _cloud_list(A, 'nearest', dev)
    tb, stacked_b = _cloud_list(B, 'nearest', dev)
    if len(qa) != len(tb):
        raise ValueError('nearest: %d query clouds for %d target clouds' % (len(qa), len(tb)))
    if int(splits) < 0:
        raise ValueError('nearest: splits must be >= 0')
    nq = [int(x.shape[0]) for x in qa]
    nt = [int(x.shape[0]) for x in tb]
    Q = sum(nq)
    dist2 = torch.empty(Q, dtype=torch.float32, device=dev)
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q:
        offs = torch.tensor(np.concatenate([np.cumsum([0] + nq), np.cumsum([0] + nt)]), dtype=torch.int64).to(dev)
        q = torch.cat(qa).contiguous()
        t = torch.cat(tb).contiguous()
        ws = torch.empty(_lib.lib().ofx_nn_search_ws_bytes(Q), dtype=torch.uint8, device=dev)
        _lib.call('ofx_nn_search', _lib.ptr(q), _lib.ptr(offs), _lib.ptr(t) if t.shape[0] else None,
                  _lib.ptr(offs[len(nq) + 1:]), len(nq), Q, max(nq), max(nt), int(splits), _lib.ptr(ws),
                  _lib.ptr(dist2), _lib.ptr(idx), _lib.stream())
    if stacked_a and stacked_b:
        return dist2.view(len(nq), -1), idx.view(len(nq), -1)
    return list(dist2.split(nq)), list(idx.split(nq))


# ---------------------------------------------------------------------------------------------------- surface scores
def _is_mesh(side):
    second = side[1]
    if torch.is_tensor(second):
        return not second.dtype.is_floating_point
    return np.asarray(second).dtype.kind in 'iu'


def _oriented(sides, n, seed, dev):
    """[(points [m, 3], normals [m, 3])] float32 on the device: meshes sampled (one call for all of them, every one
    with shape id 0, so a mesh draws the same points on either side), oriented clouds taken as they are."""
    out = [None] * len(sides)
    pos = [k for k, s in enumerate(sides) if _is_mesh(s)]
    if pos:
        p, nm = metrics.sample_surface([sides[k] for k in pos], n=n, seed=seed, normalize=False, ids=[0] * len(pos),
                                       normals=True)
        for j, k in enumerate(pos):
            out[k] = (p[j], nm[j])
    for k, s in enumerate(sides):
        if out[k] is None:
            p = torch.as_tensor(s[0]).to(device=dev, dtype=torch.float32).reshape(-1, 3)
            nm = torch.as_tensor(s[1]).to(device=dev, dtype=torch.float32).reshape(-1, 3)
            if p.shape != nm.shape or p.shape[0] == 0:
                raise ValueError('surface_scores: an oriented cloud needs as many normals as points, and at least one')
            out[k] = (p, nm)
    return out


def surface_scores(gt, pred, n=100000, seed=0, thresholds=THRESHOLDS, exact=False):
    """The surface half of the reconstruction table.  gt, pred: each a ``(verts, faces)`` mesh, of which n oriented
    surface points are drawn (metrics.sample_surface(normalize=False, normals=True), both sides with the same seed and
    shape id: a mesh against itself scores exactly 0), or a ``(points, normals)`` oriented cloud taken as it is; or
    lists of such sides, scored pairwise in the same launches.  Per shape a dict:

      completeness, accuracy      mean distance gt -> pred, pred -> gt;  completeness2, accuracy2: mean squared
      chamfer_l1, chamfer_l2      (completeness + accuracy) / 2, (completeness2 + accuracy2) / 2
      normals_completeness, normals_accuracy   mean |n_gt . n_pred[nearest]|, mean |n_pred . n_gt[nearest]|
      normal_consistency          their mean
      thresholds                  the list of tau, and per tau in the same order:
      recall, precision, fscore   share of gt / pred points with dist2 <= tau^2, and 2PR / (P + R) (0 when P + R == 0)

    The thresholds are in the clouds' own units; the defaults fit the [-0.5, 0.5] file frame.  All reductions run in
    float64 on the device over the fp32 dist2 of ``nearest``; one host read.  A dict for one pair, a list for lists.

    exact: both sides must be meshes (ValueError otherwise).  The samples of each side are then measured against the
    other side's TRIANGLES (mesh_query.closest_point) instead of its samples, so accuracy and completeness no longer
    carry the sampling noise of the target side, and the normal compared is the unit normal of the nearest face (a
    zero-area face has the zero normal).  One more host read, the status words of that call."""
    _lib.require_device()
    single = not isinstance(gt, list)
    gts, preds = ([gt], [pred]) if single else (gt, pred)
    if len(gts) != len(preds) or not gts:
        raise ValueError('surface_scores: %d gt sides for %d pred sides' % (len(gts), len(preds)))
    taus = [float(t) for t in thresholds]
    dev = _device()
    G = _oriented(gts, n, seed, dev)
    P = _oriented(preds, n, seed, dev)
    N = len(G)
    if exact:
        if not all(_is_mesh(s) for s in list(gts) + list(preds)):
            raise ValueError('surface_scores: exact=True needs a (verts, faces) mesh on both sides')
        from . import mesh_query
        targets = [mesh_query._dev_mesh(s, dev) for s in list(preds) + list(gts)]
        hit = mesh_query.closest_point(targets, [g[0].contiguous() for g in G] + [p[0].contiguous() for p in P],
                                       want_point=False)
        d2 = [h[0] * h[0] for h in hit]
        face_n = []
        for (v, f), h in zip(targets, hit):
            tri = v[f[h[1].long()].long()]                                    # [m, 3, 3]
            face_n.append(torch.nn.functional.normalize(torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0],
                                                                    dim=1), dim=1))
    else:
        d2, ix = nearest([g[0] for g in G] + [p[0] for p in P], [p[0] for p in P] + [g[0] for g in G])
    tau2 = torch.tensor([t * t for t in taus], dtype=torch.float64, device=dev)
    rows = []
    for k in range(2 * N):
        src, dst = (G[k], P[k]) if k < N else (P[k - N], G[k - N])
        d = d2[k].double()
        other = face_n[k] if exact else dst[1][ix[k].long()]
        dots = (src[1].double() * other.double()).sum(1).abs()
        within = (d[:, None] <= tau2[None, :]).double().mean(0)
        rows.append(torch.cat([torch.stack([d.sqrt().mean(), d.mean(), dots.mean()]), within]))
    rows = torch.stack(rows).tolist()                  # the one host read
    res = []
    for k in range(N):
        (c1, c2, nc), rec = rows[k][:3], rows[k][3:]
        (a1, a2, na), pre = rows[N + k][:3], rows[N + k][3:]
        res.append({'completeness': c1, 'accuracy': a1, 'completeness2': c2, 'accuracy2': a2,
                    'chamfer_l1': (c1 + a1) / 2, 'chamfer_l2': (c2 + a2) / 2,
                    'normals_completeness': nc, 'normals_accuracy': na, 'normal_consistency': (nc + na) / 2,
                    'thresholds': taus, 'recall': rec, 'precision': pre,
                    'fscore': [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(pre, rec)]})
    return res[0] if single else res


# ---------------------------------------------------------------------------------------------------- volumetric IoU
def unpack_bits(bits, n):
    """[n] bool on the device from occupancies packed as numpy.packbits packs them (include/ofx.h,
    ofx_sdf_sample_occu): point i is bit 7 - i % 8 of byte i // 8; the padding bits of the last byte are dropped."""
    if bits.shape[0] * 8 < n:
        raise ValueError('occupancy_iou: %d bytes of occupancies for %d points' % (bits.shape[0], n))
    i = torch.arange(n, device=bits.device)
    return ((bits[i >> 3].to(torch.int32) >> (7 - (i & 7)).to(torch.int32)) & 1).bool()


def occupancy_iou(field, points, bits, point_scale, level=0.0, batch_index=0):
    """Volumetric IoU of a reconstruction against the occupancies of ``points.npz``.  field: an mpu.MpuField
    (``GraphVAE.forward(evaluate=True)['neural_mpu']``) or any callable pos [n, 4] -> sdf [n]; points [n, 3] fp16 or
    fp32 in file units; bits [ceil(n / 8)] uint8 packed as numpy.packbits.  The predicted occupancy of point i is
    ``field([points_i / point_scale, batch_index]) < level`` (strict, as dataset.sample_occu's value < 0).  Returns
    (iou, intersection, union): the counts as ints, iou = intersection / union or None when the union is empty.  One
    host read."""
    _lib.require_device()
    dev = _device()
    p = torch.as_tensor(points).to(dev).to(torch.float32).reshape(-1, 3)
    b = torch.as_tensor(bits).to(device=dev, dtype=torch.uint8).reshape(-1)
    n = int(p.shape[0])
    gt = unpack_bits(b, n)
    pos = torch.cat([p / float(point_scale), torch.full((n, 1), float(batch_index), device=dev)], 1).contiguous()
    pred = field(pos).reshape(-1) < level
    inter, union = torch.stack([(pred & gt).sum(), (pred | gt).sum()]).tolist()
    return (inter / union if union else None), int(inter), int(union)
