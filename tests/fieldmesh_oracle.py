"""numpy restatement of the field-meshing contract of csrc/ofx_fieldmesh.hip (octfusion_amd.mesh.field_mesh), on top
of tests/mc_oracle.py.

  * lattice: R^3 points, coordinate of index i is fl(fl(i * step) + bbmin), step = fp32((bbmax - bbmin) / R)
    (mpu.calc_sdf's); the SDF values are GIVEN (a dense lattice [R, R, R]) -- the oracle never evaluates a field;
  * bricks: nb = ceil((R - 1) / 8) per axis, brick (I, J, K) has linear index (I * nb + J) * nb + K, owns the cells
    [8I, min(8I + 8, R - 1)) per axis and holds the points [8I, min(8I + 8, R - 1)] (its frame);
  * active: per axis lo = cell(c(first point)), hi = cell(c(last point)), cell(c) = floor((c + 1) * 2^(de - 1)) in
    fp32; the box [lo - m, hi + m], clipped to [0, 2^de - 1], holds at least one depth-de node of the shape (`nodes`:
    integer cell coordinates [n, 3]; None = the depth is dense, every brick is active);
  * mesh: mc_oracle.marching_cubes restricted to the cells of active bricks.  A crossing lattice edge is HELD by every
    brick whose frame has both endpoints; it becomes a vertex iff an active brick holds it, emitted by the one of the
    lowest linear index.  Vertex order: (rank of the emitting brick among the active bricks, owner point
    (lx * 9 + ly) * 9 + lz in that brick's frame, axis).  Triangle order: (rank of the brick, cell (cx * 8 + cy) * 8 +
    cz in the brick, table order);
  * positions: with fused=False a vertex is mc_oracle's, bit for bit: fl(fl(fl(p * step) + bbmin) * scale).  The device
    rounds p * step + bbmin ONCE (csrc/ofx_mesh.hip's mapping compiles to a fused multiply-add, which is why
    tests/test_gpu_mesh.py compares its vertices with mc_oracle to 1e-6 and not bitwise; csrc/ofx_fieldmesh.hip says
    fmaf outright): fused=True restates that, fl(fl(p * step + bbmin) * scale), exactly;
  * stats: seeds = active bricks at m = 0, bricks = active bricks, leaks = crossing lattice edges that lie in a face
    shared by an active and an inactive brick, i.e. that are held by at least one of each.
"""
import numpy as np

import mc_oracle


def n_bricks(R):
    return -(-(R - 1) // 8)


def brick_boxes(R, de, bbmin=-0.9, bbmax=0.9):
    """(lo [nb], hi [nb]) depth-de cells of the first / last point of the bricks along one axis (all three alike)."""
    nb = n_bricks(R)
    step = np.float32((bbmax - bbmin) / R)
    first = np.arange(nb, dtype=np.int64) * 8
    last = np.minimum(first + 8, R - 1)

    def cell(i):
        c = (i.astype(np.float32) * step).astype(np.float32) + np.float32(bbmin)
        f = np.floor((c.astype(np.float32) + np.float32(1.0)).astype(np.float32) * np.float32(2.0 ** (de - 1)))
        return np.clip(f, -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    return cell(first), cell(last)


def active_bricks(R, de, nodes, margin, bbmin=-0.9, bbmax=0.9):
    """bool [nb, nb, nb]."""
    nb = n_bricks(R)
    if nodes is None:
        return np.ones((nb, nb, nb), bool)
    S = 1 << de
    occ = np.zeros((S, S, S), np.int64)
    nodes = np.asarray(nodes, np.int64).reshape(-1, 3)
    occ[nodes[:, 0], nodes[:, 1], nodes[:, 2]] = 1
    acc = np.zeros((S + 1, S + 1, S + 1), np.int64)           # summed-volume table
    acc[1:, 1:, 1:] = occ.cumsum(0).cumsum(1).cumsum(2)
    lo, hi = brick_boxes(R, de, bbmin, bbmax)
    l = np.maximum(lo - margin, 0)
    h = np.minimum(hi + margin, S - 1)
    ok = l <= h
    l, h1 = np.where(ok, l, 0), np.where(ok, h + 1, 0)
    ix = np.ix_

    def box(a0, a1, b0, b1, c0, c1):
        return (acc[ix(a1, b1, c1)] - acc[ix(a0, b1, c1)] - acc[ix(a1, b0, c1)] - acc[ix(a1, b1, c0)] +
                acc[ix(a0, b0, c1)] + acc[ix(a0, b1, c0)] + acc[ix(a1, b0, c0)] - acc[ix(a0, b0, c0)])
    cnt = box(l, h1, l, h1, l, h1)
    return (cnt > 0) & ok[:, None, None] & ok[None, :, None] & ok[None, None, :]


def _holders(x, nb, along):
    """Brick coordinates along one axis of the bricks whose frame holds lattice coordinate x (and x + 1 if `along`):
    (first [n], second [n] or -1)."""
    first = x // 8
    second = np.where((x % 8 == 0) & (x > 0) & ~along, first - 1, -1)
    first = np.where(first < nb, first, -1)                    # x = 8 nb is the last point of brick nb - 1 only
    return first, second


def fma32(a, b, c):
    """fl32(a * b + c) of float32 arrays with one rounding: the product is exact in float64, the sum is rounded to odd
    there (two-sum error term), and 53 >= 24 + 2 bits make the final rounding to float32 the correct one."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    prod = a * b
    s = prod + c
    t = s - prod
    err = (prod - (s - t)) + (c - t)
    odd = (s.view(np.int64) & 1).astype(bool)
    fix = (err != 0) & ~odd
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def positions(sdf, p, a, level, bbmin, bbmax, scale, fused):
    """Output coordinates [n, 3] float32 of the crossing edges (owner linear index p, axis a) of lattice sdf."""
    v = np.asarray(sdf, np.float32)
    R = v.shape[0]
    lev = np.float32(level)
    vf = v.reshape(-1)
    stride = np.array([R * R, R, 1], np.int64)
    va, vb = vf[p], vf[p + stride[a]]
    with np.errstate(divide='ignore', invalid='ignore'):
        t = ((lev - va) / (vb - va)).astype(np.float32)
    pos = np.stack([p // (R * R), (p // R) % R, p % R], 1).astype(np.float32)
    pos[np.arange(len(p)), a] += t
    step = np.float32((bbmax - bbmin) / R)
    if fused:
        return (fma32(pos, step, np.float32(bbmin)) * np.float32(scale)).astype(np.float32)
    return ((pos * step + np.float32(bbmin)) * np.float32(scale)).astype(np.float32)


def field_mesh(sdf, de, nodes, margin=1, level=0.0, bbmin=-0.9, bbmax=0.9, scale=1.0, fused=False):
    """(verts [V, 3] float32, faces [F, 3] int32, stats dict) of one lattice [R, R, R]."""
    v = np.ascontiguousarray(np.asarray(sdf, np.float32))
    R = v.shape[0]
    nb = n_bricks(R)
    act = active_bricks(R, de, nodes, margin, bbmin, bbmax)
    seeds = active_bricks(R, de, nodes, 0, bbmin, bbmax)
    actf = act.reshape(-1)
    rank = np.cumsum(actf) - 1                                  # rank among the active bricks, by linear index
    dv, df = mc_oracle.marching_cubes(v, level, bbmin, bbmax, scale)

    # the dense vertices, in mc_oracle's order: crossing edge (owner point p, axis a)
    inside = v < np.float32(level)
    cr = np.zeros((R, R, R, 3), bool)
    cr[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cr[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cr[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    idx = np.nonzero(cr.reshape(-1))[0]
    assert len(idx) == len(dv)
    p, a = idx // 3, idx % 3
    xyz = np.stack([p // (R * R), (p // R) % R, p % R], 1)
    big = nb ** 3
    emit = np.full(len(idx), big, np.int64)                     # linear index of the emitting brick
    any_inactive = np.zeros(len(idx), bool)
    opts = [_holders(xyz[:, c], nb, a == c) for c in range(3)]
    for q in range(8):
        I = [opts[c][(q >> c) & 1] for c in range(3)]
        ok = (I[0] >= 0) & (I[1] >= 0) & (I[2] >= 0)
        lin = np.where(ok, (I[0] * nb + I[1]) * nb + I[2], 0)
        on = ok & actf[lin]
        emit = np.where(on, np.minimum(emit, lin), emit)
        any_inactive |= ok & ~actf[lin]
    keep_v = emit < big
    leaks = int((keep_v & any_inactive).sum())
    eb = np.where(keep_v, emit, 0)
    EI = np.stack([eb // (nb * nb), (eb // nb) % nb, eb % nb], 1)
    loc = xyz - 8 * EI
    assert ((loc[keep_v] >= 0) & (loc[keep_v] <= 8)).all()
    key = (rank[eb] * 729 + (loc[:, 0] * 9 + loc[:, 1]) * 9 + loc[:, 2]) * 3 + a
    order = np.argsort(np.where(keep_v, key, np.iinfo(np.int64).max), kind='stable')[:int(keep_v.sum())]
    new_id = np.full(len(idx), -1, np.int64)
    new_id[order] = np.arange(len(order))
    verts = positions(v, p[order], a[order], level, bbmin, bbmax, scale, fused)
    assert fused or np.array_equal(verts.view(np.uint32), dv[order].view(np.uint32))

    # the dense triangles, cell-major: the cell of every triangle
    ci = mc_oracle.cube_index(inside).reshape(-1)
    nt = mc_oracle._NTRI[ci].astype(np.int64)
    cell_of = np.repeat(np.arange(len(ci)), nt)
    assert len(cell_of) == len(df)
    cx, cy, cz = cell_of // ((R - 1) ** 2), (cell_of // (R - 1)) % (R - 1), cell_of % (R - 1)
    blin = ((cx // 8) * nb + cy // 8) * nb + cz // 8
    keep_f = actf[blin]
    fkey = rank[blin] * 512 + ((cx % 8) * 8 + cy % 8) * 8 + cz % 8
    forder = np.argsort(np.where(keep_f, fkey, np.iinfo(np.int64).max), kind='stable')[:int(keep_f.sum())]
    faces = new_id[df[forder].astype(np.int64)]
    assert (faces >= 0).all()
    stats = dict(seeds=int(seeds.sum()), bricks=int(act.sum()), leaks=leaks, active=act)
    return verts.reshape(-1, 3), faces.astype(np.int32).reshape(-1, 3), stats


def dense_cells_of_faces(sdf, level=0.0):
    """The cell (cx, cy, cz) of every triangle of mc_oracle.marching_cubes(sdf, level), in its order."""
    v = np.asarray(sdf, np.float32)
    R = v.shape[0]
    ci = mc_oracle.cube_index(v < np.float32(level)).reshape(-1)
    cell_of = np.repeat(np.arange(len(ci)), mc_oracle._NTRI[ci].astype(np.int64))
    return np.stack([cell_of // ((R - 1) ** 2), (cell_of // (R - 1)) % (R - 1), cell_of % (R - 1)], 1)


def canonical_triangles(verts, faces):
    """Order-free form of a mesh: every triangle as nine fp32 bit patterns, rotated to start at its smallest vertex
    (as a bit-pattern triple), the rows sorted."""
    t = np.ascontiguousarray(np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]).view(np.uint32)   # [F, 3, 3]
    t = t.astype(np.int64)
    if len(t) == 0:
        return t.reshape(0, 9)
    best = np.zeros(len(t), np.int64)                           # the lexicographically smallest (x, y, z) pattern
    for j in (1, 2):
        cur = t[np.arange(len(t)), best]
        cand = t[:, j]
        less = np.zeros(len(t), bool)
        tie = np.ones(len(t), bool)
        for c in range(3):
            less |= tie & (cand[:, c] < cur[:, c])
            tie &= cand[:, c] == cur[:, c]
        best = np.where(less, j, best)
    rot = (best[:, None] + np.arange(3)[None, :]) % 3
    t = t[np.arange(len(t))[:, None], rot].reshape(-1, 9)
    return t[np.lexsort(t.T[::-1])]
