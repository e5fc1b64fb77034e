"""Host restatement of the scan and the octree container kernels (csrc/ofx_octree.hip) in plain numpy, from the comments
in include/ofx.h and ofx_octree.hip.  TEST INFRASTRUCTURE: nothing here imports the product.

Keys: level bit i of x sits at key bit 3 i + 2, y at 3 i + 1, z at 3 i; the batch id from bit 48.  Node i of a full layer
of depth d is element i // 8^d, Morton code i % 8^d.  Functions that the kernels run "in place" (grow, the label1
kernels) take the destination arrays and write only what the kernel may write.
"""
import numpy as np

M48 = (1 << 48) - 1


def exclusive_scan(v):
    """int64 [n + 1]: out[i] = sum(v[:i]), out[n] the total (ofx_scan_i32)"""
    out = np.zeros(len(v) + 1, dtype=np.int64)
    np.cumsum(np.asarray(v, dtype=np.int64), out=out[1:])
    return out


def morton_xyz(k, depth):
    k = np.asarray(k, dtype=np.int64)
    x, y, z = np.zeros_like(k), np.zeros_like(k), np.zeros_like(k)
    for i in range(depth):
        x |= ((k >> (3 * i + 2)) & 1) << i
        y |= ((k >> (3 * i + 1)) & 1) << i
        z |= ((k >> (3 * i)) & 1) << i
    return x, y, z


def full_layer(depth, B):
    """(keys, children) of ofx_octree_full_layer"""
    per = 8 ** depth
    i = np.arange(per * B, dtype=np.int64)
    return (i % per) | ((i // per) << 48), i.copy()


def split(label):
    """(children, scan [n + 1]) of ofx_octree_split: any non-zero label splits"""
    flag = (np.asarray(label, dtype=np.int64) != 0).astype(np.int64)
    scan = exclusive_scan(flag)
    return np.where(flag != 0, scan[:-1], -1), scan


def grow(keys_parent, children_parent, keys_child, children_child):
    """ofx_octree_grow, into the given child arrays: parents with children < 0 write nothing"""
    for key, c in zip(np.asarray(keys_parent, dtype=np.int64).tolist(), np.asarray(children_parent).tolist()):
        if c < 0:
            continue
        for o in range(8):
            keys_child[8 * c + o] = (((key & M48) << 3) | o) | (key >> 48 << 48)
            children_child[8 * c + o] = 8 * c + o
    return keys_child, children_child


def _small_index(B, fd):
    """per full-layer node: (element, x, y, z)"""
    per = 8 ** fd
    i = np.arange(per * B, dtype=np.int64)
    x, y, z = morton_xyz(i % per, fd)
    return i // per, x, y, z


def positive(v):
    """`> 0` in float32: false for 0.0, -0.0, NaN and everything negative, true for the smallest denormal and +inf"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return v > np.float32(0)


def split_small_label0(split_small, fd):
    """split [B, 8, S, S, S] -> label [B * 8^fd] (any channel > 0)"""
    B = split_small.shape[0]
    b, x, y, z = _small_index(B, fd)
    return positive(split_small)[b, :, x, y, z].any(-1).astype(np.int64)


def split_small_label1(split_small, fd, children, label1):
    """label1[8 c + j] = split[b, j, x, y, z] > 0 for every full-layer node with children = c >= 0; the rest of label1
    stays as it is"""
    B = split_small.shape[0]
    b, x, y, z = _small_index(B, fd)
    pos = positive(split_small)[b, :, x, y, z]                     # [nodes, 8]
    for i, c in enumerate(np.asarray(children).tolist()):
        if c >= 0:
            label1[8 * c:8 * c + 8] = pos[i]
    return label1


def split_large_label0(split_large):
    return positive(split_large).reshape(-1, 8).any(-1).astype(np.int64)


def split_large_label1(split_large, children, label1):
    pos = positive(split_large).reshape(-1, 8)
    for i, c in enumerate(np.asarray(children).tolist()):
        if c >= 0:
            label1[8 * c:8 * c + 8] = pos[i]
    return label1


def octree2voxel_cf(data, B, depth):
    """data [B * 8^d, C] (row = element * 8^d + Morton code) -> vox [B, C, S, S, S]"""
    S, C = 1 << depth, data.shape[1]
    b, x, y, z = _small_index(B, depth)
    vox = np.zeros((B, C, S, S, S), dtype=data.dtype)
    vox[b, :, x, y, z] = data
    return vox


def voxel2octree_cf(vox, depth):
    B = vox.shape[0]
    b, x, y, z = _small_index(B, depth)
    return np.ascontiguousarray(vox[b, :, x, y, z])


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=np.float32)


def special_split(shape, seed, p_special=0.6):
    """float32 values for the `> 0` threshold: mostly the special values (zeros of both signs, the smallest denormals
    of both signs, the infinities, NaN), the rest normal random numbers"""
    g = np.random.default_rng(seed)
    v = g.standard_normal(shape).astype(np.float32)
    pick = g.random(shape) < p_special
    v[pick] = SPECIAL[g.integers(0, SPECIAL.shape[0], size=int(pick.sum()))]
    return v
