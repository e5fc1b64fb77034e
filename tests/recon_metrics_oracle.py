"""numpy float64 restatement of octfusion_amd.recon_metrics: the nearest-neighbour search with its tie rule, the surface
scores and the occupancy IoU.  Written from the contract in include/ofx.h and the module's docstrings, not from the
kernels."""
import numpy as np


def nearest(q, t, chunk=256):
    """(dist2 [n] float64, idx [n] int32): min_j |q_i - t_j|^2 in float64 from direct differences, and the LOWEST j
    attaining it (numpy.argmin returns the first minimum).  An empty t gives (+inf, -1)."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    n = q.shape[0]
    if t.shape[0] == 0:
        return np.full(n, np.inf), np.full(n, -1, np.int32)
    d2, ix = np.empty(n), np.empty(n, np.int32)
    chunk = max(1, min(chunk, (1 << 21) // t.shape[0]))
    for i in range(0, n, chunk):
        dx, dy, dz = (q[i:i + chunk, None, a] - t[None, :, a] for a in range(3))
        d = dz * dz + (dy * dy + dx * dx)
        ix[i:i + chunk] = np.argmin(d, axis=1)
        d2[i:i + chunk] = d[np.arange(d.shape[0]), ix[i:i + chunk]]
    return d2, ix


def tied_queries(q, t, chunk=256):
    """How many queries have their float64 minimum attained by more than one target."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    chunk = max(1, min(chunk, (1 << 21) // max(1, t.shape[0])))
    ties = 0
    for i in range(0, q.shape[0], chunk):
        dx, dy, dz = (q[i:i + chunk, None, a] - t[None, :, a] for a in range(3))
        d = dz * dz + (dy * dy + dx * dx)
        ties += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    return ties


def dist2_to(q, t, idx):
    """float64 |q_i - t_idx[i]|^2."""
    diff = np.asarray(q, np.float64) - np.asarray(t, np.float64)[idx]
    return (diff * diff).sum(1)


def scores_from_nearest(gt_n, pred_n, d2_gp, ix_gp, d2_pg, ix_pg, thresholds):
    """The reductions of surface_scores from the two directed searches (gt -> pred, pred -> gt), in float64.  d2_*:
    the squared distances exactly as the device reported them (fp32 values)."""
    gt_n, pred_n = np.asarray(gt_n, np.float64), np.asarray(pred_n, np.float64)
    d_gp, d_pg = np.asarray(d2_gp, np.float64), np.asarray(d2_pg, np.float64)
    c1, a1 = np.sqrt(d_gp).mean(), np.sqrt(d_pg).mean()
    c2, a2 = d_gp.mean(), d_pg.mean()
    nc = np.abs((gt_n * pred_n[ix_gp]).sum(1)).mean()
    na = np.abs((pred_n * gt_n[ix_pg]).sum(1)).mean()
    taus = [float(t) for t in thresholds]
    rec = [float((d_gp <= t * t).mean()) for t in taus]
    pre = [float((d_pg <= t * t).mean()) for t in taus]
    return {'completeness': float(c1), 'accuracy': float(a1), 'completeness2': float(c2), 'accuracy2': float(a2),
            'chamfer_l1': float(c1 + a1) / 2, 'chamfer_l2': float(c2 + a2) / 2,
            'normals_completeness': float(nc), 'normals_accuracy': float(na), 'normal_consistency': float(nc + na) / 2,
            'thresholds': taus, 'recall': rec, 'precision': pre,
            'fscore': [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(pre, rec)]}


def surface_scores(gt, pred, thresholds=(0.01, 0.015, 0.02)):
    """gt, pred: (points [n, 3], normals [n, 3]) oriented clouds.  Distances in float64 (on inputs whose fp32
    differences, squares and sums are exact, the values the device computes)."""
    d_gp, i_gp = nearest(gt[0], pred[0])
    d_pg, i_pg = nearest(pred[0], gt[0])
    return scores_from_nearest(gt[1], pred[1], d_gp, i_gp, d_pg, i_pg, thresholds)


def unpack_bits(bits, n):
    """[n] bool: point i is bit 7 - i % 8 of byte i // 8 (numpy.packbits' order), padding ignored."""
    bits = np.asarray(bits, np.uint8).reshape(-1)
    i = np.arange(n)
    return ((bits[i >> 3] >> (7 - (i & 7))) & 1).astype(bool)


def occupancy_iou(values, bits, level=0.0):
    """(iou | None, intersection, union) of ``values < level`` (the field's values at the points, as given) against the
    packed occupancies."""
    values = np.asarray(values).reshape(-1)
    gt = unpack_bits(bits, values.shape[0])
    pred = values < level
    inter, union = int((pred & gt).sum()), int((pred | gt).sum())
    return (inter / union if union else None), inter, union
