"""Host-side oracle for the dense levels' tap tables (csrc/ofx_dense.hip: ofx_grid_conv_table) and their reverse
(csrc/ofx_graph.hip: ofx_table_reverse_count / ofx_table_reverse_fill), by plain loops.  Rows are b * 8^d + morton(x, y, z)
in the Morton order of oracle/octree.py (x -> key bit 3i + 2, y -> 3i + 1, z -> 3i); tap = (kx * 3 + ky) * 3 + kz with
offsets k - 1.  No GPU, no octfusion_amd.

  mode 0  nn.Conv3d(k3, p1): in and out at depth d; source = o + tap - 1 where that is inside the grid.
  mode 1  ConvDownsample (k3, s2, p1): out at depth d, in at depth d + 1; source = 2 o + tap - 1 inside the fine grid.
  mode 2  ConvUpsample (nearest x2, then k3 p1): out at depth d, in at depth d - 1; the upsampled voxel f = o + tap - 1
          inside the out-sized grid reads source f >> 1.
Anything else is `pad`."""
import functools

import torch

from oracle.octree import xyz2key


def depth_in(mode, depth_out):
    return depth_out + (0, 1, -1)[mode]


@functools.lru_cache(maxsize=None)
def _morton(depth):
    """[S][S][S] nested lists of the Morton index of (x, y, z) at `depth`, from the oracle's interleave."""
    S = 1 << depth
    g = torch.arange(S)
    x, y, z = torch.meshgrid(g, g, g, indexing='ij')
    return xyz2key(x, y, z, depth=max(depth, 1)).tolist()


@functools.lru_cache(maxsize=None)
def _table(mode, depth_out, B):
    """The table with None for padding, as a list of rows."""
    S, Sin = 1 << depth_out, 1 << depth_in(mode, depth_out)
    mo, mi = _morton(depth_out), _morton(depth_in(mode, depth_out))
    rows = [None] * (B * S ** 3)
    for b in range(B):
        for x in range(S):
            for y in range(S):
                for z in range(S):
                    taps = []
                    for tap in range(27):
                        t = (tap // 9 - 1, tap // 3 % 3 - 1, tap % 3 - 1)
                        if mode == 0:
                            i, lim = (x + t[0], y + t[1], z + t[2]), S
                        elif mode == 1:
                            i, lim = (2 * x + t[0], 2 * y + t[1], 2 * z + t[2]), Sin
                        else:
                            i, lim = (x + t[0], y + t[1], z + t[2]), S
                        ok = all(0 <= c < lim for c in i)
                        if ok and mode == 2:
                            i = tuple(c >> 1 for c in i)
                        taps.append(b * Sin ** 3 + mi[i[0]][i[1]][i[2]] if ok else None)
                    rows[b * S ** 3 + mo[x][y][z]] = taps
    assert all(r is not None for r in rows)
    return rows


def table(mode, depth_out, B, pad):
    """int32 [B * 8^depth_out, 27]."""
    return torch.tensor([[pad if s is None else s for s in r] for r in _table(mode, depth_out, B)], dtype=torch.int32)


def n_in(mode, depth_out, B):
    return B * 8 ** depth_in(mode, depth_out)


def reverse(tab, n_in):
    """Brute-force reverse CSR of a tap table [n_out, ndir]: (rev_cnt [n_in * ndir], rev_ptr [n_in * ndir + 1], rev_row [E])
    keyed by source * ndir + tap, each segment the ascending list of the output rows whose entry names that source;
    entries outside [0, n_in) are padding."""
    n_out, ndir = tab.shape
    seg = [[] for _ in range(n_in * ndir)]
    for r, row in enumerate(tab.tolist()):
        for t, s in enumerate(row):
            if 0 <= s < n_in:
                seg[s * ndir + t].append(r)
    cnt = [len(s) for s in seg]
    ptr = [0]
    for c in cnt:
        ptr.append(ptr[-1] + c)
    return (torch.tensor(cnt, dtype=torch.int32).reshape(-1), torch.tensor(ptr, dtype=torch.int32),
            torch.tensor([r for s in seg for r in s], dtype=torch.int32).reshape(-1))
