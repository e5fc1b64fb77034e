"""tests/gridtab_oracle.py on the host: a gather through the oracle's tap tables is torch's conv3d (stride 1, stride 2,
nearest-upsample then stride 1) on the voxel grid the rows are the Morton order of; the brute-force reverse names every
valid entry exactly once, in ascending rows.  No GPU, no octfusion_amd."""
import pytest
import torch
import torch.nn.functional as F

import gridtab_oracle as T
from oracle.octree import key2xyz

torch.set_grad_enabled(False)


def _voxels(feat, B, depth):
    """rows b * 8^d + morton -> [B, 1, S, S, S]."""
    S = 1 << depth
    x, y, z, _ = key2xyz(torch.arange(S ** 3), depth=max(depth, 1))
    vox = torch.zeros(B, 1, S, S, S, dtype=feat.dtype)
    for b in range(B):
        vox[b, 0, x, y, z] = feat[b * S ** 3:(b + 1) * S ** 3]
    return vox


@pytest.mark.parametrize('mode,depth_out', [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 1), (2, 2)])
def test_gather_through_the_table_is_conv3d(mode, depth_out):
    B = 2
    d_in, n_in = T.depth_in(mode, depth_out), T.n_in(mode, depth_out, B)
    g = torch.Generator().manual_seed(10 * mode + depth_out)
    feat = torch.randn(n_in, generator=g, dtype=torch.float64)
    w = torch.randn(27, generator=g, dtype=torch.float64)
    tab = T.table(mode, depth_out, B, n_in).long()                       # pad = the zero row
    assert tab.shape == (B * 8 ** depth_out, 27) and int(tab.min()) >= 0 and int(tab.max()) <= n_in
    got = torch.cat([feat, torch.zeros(1, dtype=torch.float64)])[tab] @ w
    vox = _voxels(feat, B, d_in)
    k = w.view(1, 1, 3, 3, 3)
    if mode == 0:
        ref = F.conv3d(vox, k, padding=1)
    elif mode == 1:
        ref = F.conv3d(vox, k, stride=2, padding=1)
    else:
        ref = F.conv3d(F.interpolate(vox, scale_factor=2, mode='nearest'), k, padding=1)
    assert torch.allclose(_voxels(got, B, depth_out), ref, rtol=0, atol=1e-12)
    for pad in (-1, 123456789):
        other = T.table(mode, depth_out, B, pad).long()
        assert torch.equal(other == pad, tab == n_in) and torch.equal(other[other != pad], tab[tab != n_in])


def test_reverse_names_every_valid_entry_once():
    g = torch.Generator().manual_seed(3)
    tab = torch.randint(-2, 12, (40, 7), generator=g, dtype=torch.int32)
    cnt, ptr, row = T.reverse(tab, 9)
    valid = (tab >= 0) & (tab < 9)
    assert int(cnt.sum()) == int(valid.sum()) == row.numel() == int(ptr[-1])
    for s in range(9):
        for t in range(7):
            seg = row[int(ptr[s * 7 + t]):int(ptr[s * 7 + t + 1])]
            assert seg.tolist() == torch.nonzero(tab[:, t] == s).reshape(-1).tolist()
    up = T.table(2, 1, 1, -1)                                            # several output rows name one (source, tap)
    assert int(T.reverse(up, 1)[0].max()) > 1
