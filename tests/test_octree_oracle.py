"""tests/octree_oracle.py on the host: equal to oracle/octree.py and oracle/sampler.py wherever they overlap -- the full
layers, split / grow on ragged trees, the split-to-label conversions as split2octree_small / _large use them, and
octree2voxel -- and the threshold of the label kernels at the special float32 values."""
import numpy as np
import pytest
import torch

import graph_oracle as G
import octree_oracle as O


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('depth', range(5))
def test_full_layer(depth, B):
    from oracle import sampler as OS
    oc = OS.create_full_octree(depth, depth, B)
    keys, children = O.full_layer(depth, B)
    assert np.array_equal(keys, oc.keys[depth].numpy()) and np.array_equal(children, oc.children[depth].numpy())
    assert np.array_equal(keys >> 48, np.repeat(np.arange(B), 8 ** depth))


@pytest.mark.parametrize('name', ['deep_a', 'deep_b_mid', 'deep_c', 'full_face'])
def test_split_and_grow_rebuild_the_tree(name):
    """every level of an oracle tree from the one above it; and the whole tree from its two splits"""
    oc = G.tree(name)[0]
    for d in range(oc.full_depth, oc.depth):
        label = (oc.children[d].numpy() >= 0).astype(np.int64) * np.where(np.arange(int(oc.nnum[d])) % 2, -7, 3)
        children, scan = O.split(label)
        assert np.array_equal(children, oc.children[d].numpy()) and scan[-1] == int(oc.nnum_nempty[d])
        n = int(oc.nnum[d + 1])
        assert n == 8 * scan[-1]
        kc, cc = O.grow(oc.keys[d].numpy(), children, np.full(n, -5, dtype=np.int64), np.full(n, -5, dtype=np.int64))
        assert np.array_equal(kc, oc.keys[d + 1].numpy()) and np.array_equal(cc, np.arange(n))
    fd, small, large = G.tree_splits(name)
    keys, children = O.full_layer(fd, small.shape[0])
    children, scan = O.split(O.split_small_label0(small.numpy(), fd))
    assert np.array_equal(children, oc.children[fd].numpy())
    label1 = O.split_small_label1(small.numpy(), fd, children, np.full(8 * scan[-1], -5, dtype=np.int64))
    assert np.array_equal(O.split(label1)[0], oc.children[fd + 1].numpy())
    ls = large(int(oc.nnum[fd + 2])).numpy()
    children2, scan2 = O.split(O.split_large_label0(ls))
    assert np.array_equal(children2, oc.children[fd + 2].numpy())
    label1 = O.split_large_label1(ls, children2, np.full(8 * scan2[-1], -5, dtype=np.int64))
    assert np.array_equal(O.split(label1)[0], oc.children[fd + 3].numpy())


def test_grow_leaves_absent_children_alone():
    keys = np.array([5 | (2 << 48), 6 | (2 << 48), 7 | (3 << 48)], dtype=np.int64)
    kc, cc = O.grow(keys, np.array([-1, 1, -1]), np.full(24, -5, dtype=np.int64), np.full(24, -5, dtype=np.int64))
    assert np.all(kc[:8] == -5) and np.all(kc[16:] == -5) and np.all(cc[:8] == -5)
    assert np.array_equal(kc[8:16], ((6 << 3) | np.arange(8)) | (2 << 48)) and np.array_equal(cc[8:16], np.arange(8, 16))


@pytest.mark.parametrize('B', [1, 3, 9])
@pytest.mark.parametrize('depth', range(4))
def test_octree2voxel(depth, B):
    from oracle import octree as OO, sampler as OS
    oc = OS.create_full_octree(depth, depth, B)
    data = np.random.default_rng(depth * 10 + B).standard_normal((B * 8 ** depth, 5)).astype(np.float32)
    want = OO.octree2voxel(torch.tensor(data), oc, depth).permute(0, 4, 1, 2, 3).contiguous().numpy()
    vox = O.octree2voxel_cf(data, B, depth)
    assert np.array_equal(vox, want)
    assert np.array_equal(O.voxel2octree_cf(vox, depth), data)


def test_threshold_at_the_special_values():
    v = O.SPECIAL
    assert O.positive(v).tolist() == [False, False, True, False, True, False, False, True, False]
    assert v[2] > 0 and v[2] == np.float32(2.0 ** -149) and v[3] == -v[2]
    ds = torch.tensor(v)
    assert np.array_equal((ds > 0).numpy(), O.positive(v))         # the reference's `split > 0`
    sp = O.special_split((3, 8, 2, 2, 2), 1)
    for s in O.SPECIAL:
        assert np.any(sp.view(np.int32) == np.array(s, dtype=np.float32).view(np.int32)), s
    want = (torch.tensor(sp) > 0).float().sum(1) > 0
    b, x, y, z = O._small_index(3, 1)
    assert np.array_equal(O.split_small_label0(sp, 1), want.numpy()[b, x, y, z].astype(np.int64))
    assert np.array_equal(O.exclusive_scan([3, 0, 4]), [0, 3, 3, 7])
