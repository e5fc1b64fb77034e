"""numpy restatement of the reference's training-data samplers (tools/repair_mesh.py: sample_sdf :293-334, sample_occu
:358-375, generate_test_points :381-413) with explicit uniforms -- what csrc/ofx_sdfdata.hip is tested against.

* sample_sdf: the positions are the reference's fp32 arithmetic to the bit (fl32(node + u), then the scale); the
  interpolation and the gradient, torch fp32 in the reference, are evaluated in float64 from those positions, so the
  oracle is the value both the reference and the kernel round.
* sample_occu: float64 throughout, as the reference.
"""
import numpy as np

GRID = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]])


def sphere_lattice(S, centre=(0.07, -0.05, 0.03), radius=0.55):
    """[S, S, S] float32 SDF of a sphere; lattice index i sits at coordinate i / (S/2) - 1."""
    c = np.arange(S, dtype=np.float64) / (S / 2) - 1
    x, y, z = np.meshgrid(c, c, c, indexing='ij')
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return d.astype(np.float32)


def full_nodes(depths):
    """(xyz [N, 3] int32, depth_off) of every node of the given depths, depth-major, x slowest."""
    xyz, off = [], [0]
    for d in depths:
        r = np.arange(2 ** d)
        g = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3)
        xyz.append(g)
        off.append(off[-1] + len(g))
    return np.concatenate(xyz).astype(np.int32), off


def trilinear(sdf, xyz):
    """(value [n], corner values [n, 8]) in float64 at float64 lattice positions xyz [n, 3]."""
    xyz = xyz.astype(np.float64)
    xyzi = np.floor(xyz)
    corners = xyzi[:, None, :] + GRID
    coordsf = xyz[:, None, :] - corners
    weights = np.prod(1 - np.abs(coordsf), axis=-1)
    c = corners.astype(np.int64).reshape(-1, 3)
    s = sdf[c[:, 0], c[:, 1], c[:, 2]].reshape(-1, 8).astype(np.float64)
    return np.sum(s * weights, axis=1), s


def sample_sdf(sdf, xyz, depth_off, depth_start, k, u, shape_scale=0.5):
    """dict(points, grad, sdf fp16; pos fp32 = the kept lattice positions; keep = mask over the N*k candidates)."""
    S = sdf.shape[0]
    u = np.asarray(u, np.float32).reshape(-1, k, 3)
    ps = []
    for i in range(len(depth_off) - 1):
        d = depth_start + i
        lo, hi = depth_off[i], depth_off[i + 1]
        p = (xyz[lo:hi, None, :].astype(np.float32) + u[lo:hi]).reshape(-1, 3)      # fp32 add
        ps.append(p * np.float32(S / 2 ** d))
    p = np.concatenate(ps) if ps else np.zeros((0, 3), np.float32)
    assert p.dtype == np.float32
    keep = (p < S - 1).all(axis=1)
    p = p[keep]
    value, s = trilinear(sdf, p)
    gx = s[:, 4] - s[:, 0] + s[:, 5] - s[:, 1] + s[:, 6] - s[:, 2] + s[:, 7] - s[:, 3]
    gy = s[:, 2] - s[:, 0] + s[:, 3] - s[:, 1] + s[:, 6] - s[:, 4] + s[:, 7] - s[:, 5]
    gz = s[:, 1] - s[:, 0] + s[:, 3] - s[:, 2] + s[:, 5] - s[:, 4] + s[:, 7] - s[:, 6]
    grad = np.stack([gx, gy, gz], -1)
    norm = np.sqrt(np.sum(grad ** 2, -1, keepdims=True))
    points = (p / np.float32(S / 2) - np.float32(1)).astype(np.float16) * np.float16(shape_scale)
    return {'points': points, 'grad': (grad / (norm + 1.0e-8)).astype(np.float16), 'sdf': value.astype(np.float16),
            'pos': p, 'keep': keep, 'grad_sum_norm': norm[:, 0], 'value': value}


def packbits(bits):
    """numpy.packbits written out: the first bit of every eight is the most significant, the tail is zero-padded."""
    bits = np.asarray(bits, bool).reshape(-1)
    out = np.zeros((len(bits) + 7) // 8, np.uint8)
    for i in np.nonzero(bits)[0]:
        out[i >> 3] |= np.uint8(0x80 >> (i & 7))
    return out


def sample_occu(sdf, u, shape_scale=0.5):
    """dict(points fp16 [n, 3], occupancies uint8 [ceil(n/8)], value float64 [n])."""
    S = sdf.shape[0]
    factor = (S - 1.0) / S
    points_uniform = np.asarray(u, np.float64).reshape(-1, 3) * factor
    points = ((points_uniform - 0.5) * (2 * float(np.float32(shape_scale)))).astype(np.float16)
    value, _ = trilinear(sdf, points_uniform * S)
    return {'points': points, 'occupancies': packbits(value < 0), 'value': value}


def generate_test_points(points, idx, noise):
    """points[idx] + noise as float32 (the reference draws idx and noise from numpy's global state)."""
    return (np.asarray(points, np.float32)[idx] + noise).astype(np.float32)
