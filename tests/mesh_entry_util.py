"""Helpers of the mesh entry-point tests (test_gpu_mesh_entry.py, test_gpu_mesh_cc_entry.py, test_gpu_simplify_entry.py):
raw calls through the C ABI with every output and workspace between sentinel bands, and the batch meshes the component
and the simplification tests share.  The mesh builders are numpy only; test_mesh_entry_oracle.py checks them without a
GPU.  Nothing here touches the device at import.
"""
import ctypes

import numpy as np
import pytest
import torch

BAND = 256                        # bytes of sentinel on both sides of a buffer: 64 words, and the payload stays aligned
SENT = {torch.int32: -1234567, torch.int64: -123456789012, torch.uint8: 0xA5, torch.float32: -12345.678}
OFX_EINVAL_TEXT = 'invalid argument'
INT32_MAX = 2 ** 31 - 1


def dev():
    return torch.device('cuda:0')


def lib():
    from octfusion_amd import _lib
    return _lib.lib()


def _call(name, *args):
    """A status-returning entry point on the current stream; raises OfxError unless it returns OFX_OK."""
    from octfusion_amd._lib import call, stream
    return call(name, *args, stream())


def _refused(name, *args):
    from octfusion_amd import _lib
    with pytest.raises(_lib.OfxError, match=OFX_EINVAL_TEXT):
        _call(name, *args)


class Guarded:
    """`n` elements prefilled with the dtype's sentinel between two sentinel bands of BAND bytes; `.ptr` points at the
    first of the n (256-byte aligned, as the workspaces want it)."""

    def __init__(self, n, dtype, cols=None):
        self.n, self.dtype, self.cols = int(n) * (cols or 1), dtype, cols
        self.pad = BAND // torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((self.n + 2 * self.pad,), SENT[dtype], dtype=dtype, device=dev())
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf[self.pad:self.pad + self.n]
        self.ptr = self.buf.data_ptr() + BAND

    def bands_intact(self):
        want = torch.full((self.pad,), SENT[self.dtype], dtype=self.dtype, device=dev())
        return torch.equal(self.buf[:self.pad], want) and torch.equal(self.buf[self.pad + self.n:], want)

    def untouched(self):
        return torch.equal(self.buf, torch.full_like(self.buf, SENT[self.dtype]))

    def set(self, values):
        self.view.copy_(torch.as_tensor(np.ascontiguousarray(values)).to(self.dtype).reshape(-1))
        return self

    def reset(self):
        self.buf.fill_(SENT[self.dtype])
        return self

    def get(self):
        """The payload on the host (int64 for the integer types); fails if a band was written."""
        assert self.bands_intact(), 'wrote outside its extent'
        a = self.view.cpu().numpy()
        a = a.astype(np.int64) if self.dtype != torch.float32 else a
        return a.reshape(-1, self.cols) if self.cols else a

    def raw(self):
        """The payload's bytes on the host, for bit comparisons (NaN payloads, signed zeros)."""
        assert self.bands_intact(), 'wrote outside its extent'
        return self.view.cpu().numpy().view(np.uint8).copy()

    def is_sentinel(self, rows):
        """True iff all the given rows (elements when there are no columns) still hold the sentinel."""
        a = self.view.cpu().numpy()
        a = a.reshape(-1, self.cols) if self.cols else a
        want = np.asarray(SENT[self.dtype]).astype(a.dtype)
        return bool((a[rows] == want).all())


class Arena:
    """Several int32 tensors carved out of one allocation filled with the sentinel, each with a band of BAND bytes
    around it: what one stray index of a neighbour would hit first."""

    def __init__(self, sizes, dtype=torch.int32):
        self.dtype = dtype
        pad = BAND // torch.empty(0, dtype=dtype).element_size()
        self.spans, off = [], pad
        for n in sizes:
            self.spans.append((off, int(n)))
            off = (off + int(n) + pad + pad - 1) // pad * pad
        self.buf = torch.full((off,), SENT[dtype], dtype=dtype, device=dev())
        assert self.buf.data_ptr() % 256 == 0

    def view(self, i):
        s, n = self.spans[i]
        return self.buf[s:s + n]

    def ptr(self, i):
        return self.buf.data_ptr() + self.spans[i][0] * self.buf.element_size()

    def get(self, i):
        return self.view(i).cpu().numpy().astype(np.int64)

    def guards_intact(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for s, n in self.spans:
            mask[s:s + n] = False
        return bool((self.buf[mask] == SENT[self.dtype]).all())

    def untouched(self):
        return bool((self.buf == SENT[self.dtype]).all())


def settled(*guards):
    """After refused calls: nothing was launched, so every buffer is sentinel from end to end."""
    torch.cuda.synchronize()
    for g in guards:
        assert g.untouched()


def up(a, dtype):
    """Host array -> device tensor of at least one element (an empty tensor has a NULL data pointer)."""
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).reshape(-1)
    if t.numel() == 0:
        t = torch.zeros(1, dtype=dtype)
    return t.to(dev())


def workspace(nbytes):
    nbytes = int(nbytes)
    assert nbytes > 0
    return Guarded(nbytes, torch.uint8)


def max_grid_dim_y():
    """hipDeviceAttributeMaxGridDimY of device 0, read through the runtime the library is linked against."""
    L = lib()
    fn = L.hipDeviceGetAttribute
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int]

    def attr(k):
        v = ctypes.c_int(-1)
        assert fn(ctypes.byref(v), k, 0) == 0
        return v.value
    # hip_runtime_api.h, hipDeviceAttribute_t: MaxBlockDimX = 26, MaxGridDimX = 29, MaxGridDimY = 30
    assert attr(26) == 1024 and attr(29) >= 2 ** 31 - 1, 'the attribute numbering is not the one this helper knows'
    return attr(30)


# ---- batch meshes -------------------------------------------------------------------------------------------------
TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
KINDS = ('tetra', 'pair', 'no_verts', 'no_faces', 'unused')


def tiny_shape(kind, rng):
    """One small mesh (verts [V, 3] float32, faces [F, 3] int32) at a random place and scale."""
    s = np.float32(rng.uniform(0.25, 2.0))
    t = rng.uniform(-3, 3, 3).astype(np.float32)
    if kind == 'no_verts':
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    if kind == 'no_faces':
        return (rng.standard_normal((3, 3)).astype(np.float32)), np.zeros((0, 3), np.int32)
    if kind == 'tetra':
        return TETRA_V * s + t, TETRA_F.copy()
    if kind == 'pair':
        v = np.concatenate([TETRA_V * s + t, TETRA_V * np.float32(0.5) * s + t + np.float32(4.0)])
        return v.astype(np.float32), np.concatenate([TETRA_F, TETRA_F + 4]).astype(np.int32)
    if kind == 'unused':                       # two stray vertices in front of a tetrahedron, one behind
        v = np.concatenate([rng.standard_normal((2, 3)).astype(np.float32) + 9, TETRA_V * s + t,
                            rng.standard_normal((1, 3)).astype(np.float32) - 9])
        return v.astype(np.float32), (TETRA_F + 2).astype(np.int32)
    raise ValueError(kind)


def tiny_batch(n=300, seed=5):
    """`n` tiny shapes of all KINDS in random order (the first five are one of each, then shuffled)."""
    rng = np.random.default_rng(seed)
    kinds = list(KINDS) + [KINDS[k] for k in rng.integers(0, len(KINDS), n - len(KINDS))]
    kinds = [kinds[i] for i in rng.permutation(n)]
    return kinds, [tiny_shape(k, rng) for k in kinds]


def uv_sphere(n_lat=40, n_lon=50, r=1.0, center=(0.1, -0.2, 0.3)):
    """A UV sphere of n_lat rings of n_lon vertices (no pole vertices: it is open at its two smallest rings) -- 2000
    vertices and 3900 faces by default, one component."""
    th = (np.arange(n_lat) + 0.5) * np.pi / n_lat
    ph = np.arange(n_lon) * 2 * np.pi / n_lon
    T, P = np.meshgrid(th, ph, indexing='ij')
    v = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3) * r + np.asarray(center)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing='ij')
    a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    c, d = a + n_lon, b + n_lon
    f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def cat(meshes):
    """Batch layout of a list of meshes: verts [V, 3], faces [F, 3] (local indices), vert_off, tri_off int64 [B + 1]."""
    nv = [len(m[0]) for m in meshes]
    nf = [len(m[1]) for m in meshes]
    v = np.concatenate([m[0].reshape(-1, 3) for m in meshes]).astype(np.float32)
    f = np.concatenate([m[1].reshape(-1, 3) for m in meshes]).astype(np.int32)
    return v, f, np.concatenate([[0], np.cumsum(nv)]).astype(np.int64), \
        np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)


def gapped(counts, rng, lead=3):
    """Offsets [B] with a gap of 0 .. 4 rows in front of every shape (and `lead` in front of the first), and the total
    number of rows: what a caller may pass instead of the running sums."""
    counts = np.asarray(counts, np.int64)
    gaps = rng.integers(0, 5, len(counts))
    gaps[0] = lead
    off = np.cumsum(gaps + np.concatenate([[0], counts[:-1]]))
    return off.astype(np.int64), int(off[-1] + counts[-1] + 2)


def rows_of(off, counts):
    """Boolean mask over the rows that the shapes' ranges cover."""
    total = int((np.asarray(off) + np.asarray(counts)).max()) if len(off) else 0
    m = np.zeros(total, bool)
    for o, c in zip(off, counts):
        m[o:o + c] = True
    return m


# cell sizes for a mesh of extent exactly 1 (TETRA_V): 1 / s = 1024.5 needs cell 1024 and is flagged, 1023.5 fits
OVERFLOW_CELL_SIZES = (1.0 / 1024.5, 1.0 / 1023.5)


def fan(n_faces):
    """One hub vertex 0 and n_faces faces (0, i, i + 1) around it: every union of the device contends for one root."""
    i = np.arange(1, n_faces + 1)
    f = np.stack([np.zeros_like(i), i, i + 1], 1).astype(np.int32)
    a = np.arange(n_faces + 2) * (2 * np.pi / (n_faces + 1))
    v = np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], 1).astype(np.float32)
    v[0] = 0
    return v, f


def comb(teeth, length):
    """A spine strip with `teeth` strips hanging off it, all joined: one component whose faces are listed tooth by
    tooth, so the roots of the teeth meet late."""
    verts, faces = [], []
    base = 0
    spine = []
    for t in range(teeth):
        ids = base + np.arange(length + 2)
        k = np.arange(length)
        faces.append(np.stack([ids[k], ids[k + 1], ids[k + 2]], 1))
        verts.append(np.stack([np.full(length + 2, float(t)), np.arange(length + 2) * 0.5,
                               (np.arange(length + 2) % 2) * 0.25], 1))
        spine.append(ids[0])
        base += length + 2
    spine = np.array(spine)
    k = np.arange(teeth - 2)
    faces.append(np.stack([spine[k], spine[k + 1], spine[k + 2]], 1))          # listed last
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32)


def reversed_strip(n_faces):
    i = np.arange(n_faces)[::-1]
    f = np.stack([i, i + 1, i + 2], 1).astype(np.int32)
    t = np.arange(n_faces + 2, dtype=np.float32)
    return np.stack([t * np.float32(0.5), (np.arange(n_faces + 2) % 2).astype(np.float32), np.zeros_like(t)], 1), f
