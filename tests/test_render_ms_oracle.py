"""CPU checks of the multisample oracle (tests/render_ms_oracle.py): the sample tables, the shift identity against exact
rational arithmetic at the sample positions, exactly-once coverage per sample plane, and the resolve.  They pin the
oracle, not the product: tests/test_gpu_render_msaa.py holds the device to it."""
from fractions import Fraction

import numpy as np
import pytest

import render_ms_oracle as MS
import render_oracle as O
from test_render_oracle import CASES, P, SIZE

T4 = [(96, 32), (224, 96), (32, 160), (160, 224)]
T16 = [(144, 144), (112, 80), (80, 160), (192, 112), (48, 96), (160, 208), (208, 176), (176, 48),
       (96, 224), (128, 16), (64, 32), (32, 192), (0, 128), (240, 64), (224, 240), (16, 0)]
TABLES = {1: [(128, 128)], 4: T4, 16: T16}


def test_sample_tables():
    assert MS.OFFSETS == TABLES
    assert TABLES[1] == [(O.HALF, O.HALF)]
    for S, step in ((4, 64), (16, 16)):
        t = np.array(TABLES[S])
        assert t.shape == (S, 2) and t.min() >= 0 and t.max() < O.SUB
        # rook property: every one of the S columns and S rows of the pixel holds exactly one sample
        assert sorted(t[:, 0] // step) == list(range(S)) and sorted(t[:, 1] // step) == list(range(S))
        assert len({tuple(r) for r in t.tolist()}) == S
    assert (np.array(T4) % 64 == 32).all()                      # the rotated grid: the centres of its cells
    assert (np.array(T16) % 16 == 0).all()


def _brute_coverage(tri, size, ox, oy):
    """The tie rule by its definition, at sample (ox, oy) of every pixel: the sample moved by (+eps, +eps^2) lies
    strictly inside the triangle (a left edge or a top edge owns the points on it).  Coordinates are multiples of
    1/256 pixel and edge functions multiples of 2^-16, so eps = 2^-40 decides every on-edge case and no other."""
    eps = Fraction(1, 2 ** 40)
    (ax, ay), (bx, by), (cx, cy) = [(Fraction(int(x), 256), Fraction(int(y), 256)) for x, y in tri]
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    out = np.zeros((size, size), bool)
    if area == 0:
        return out
    for j in range(size):
        for i in range(size):
            px, py = i + Fraction(ox, 256) + eps, j + Fraction(oy, 256) + eps * eps
            e = [(bx - ax) * (py - ay) - (by - ay) * (px - ax), (cx - bx) * (py - by) - (cy - by) * (px - bx),
                 (ax - cx) * (py - cy) - (ay - cy) * (px - cx)]
            out[j, i] = all(x * area > 0 for x in e)
    return out


def _coverage_ms(tri, size, offsets):
    keys, _ = MS.raster_ms(np.asarray(tri, np.int64).reshape(3, 2), np.zeros(3), [[0, 1, 2]], size, offsets)
    return keys != np.uint64(O.EMPTY)


# the existing cases, and two that put a shared edge and a vertex on sample positions of both patterns: (96, 32) is
# sample 0 of the 4-table, (144, 144) sample 0 of the 16-table, and the edge x = 3 P + 32 passes through sample 2 of
# the 4-table and sample 11 of the 16-table of every pixel of column 3
MS_CASES = dict(CASES)
MS_CASES['vertex_on_samples'] = ([(2 * P + 96, 2 * P + 32), (6 * P + 144, 2 * P + 144), (2 * P + 96, 6 * P + 32),
                                  (6 * P + 144, 6 * P + 144)], [(0, 1, 2), (2, 1, 3)], [0.5] * 4)
MS_CASES['edge_through_samples'] = ([(3 * P + 32, 0), (3 * P + 32, 8 * P), (0, 4 * P), (8 * P, 4 * P)],
                                    [(0, 1, 2), (1, 0, 3)], [0.5] * 4)


@pytest.mark.parametrize('S', [4, 16])
@pytest.mark.parametrize('name', sorted(MS_CASES))
def test_sample_shift_against_exact_rationals(name, S):
    pts, faces, depth = MS_CASES[name]
    for tri in faces:
        t = [pts[k] for k in tri]
        have = _coverage_ms(t, SIZE, TABLES[S])
        for s, (ox, oy) in enumerate(TABLES[S]):
            assert np.array_equal(have[:, :, s], _brute_coverage(t, SIZE, ox, oy)), (tri, s)
    # visibility: every plane is the one-sample rasteriser's on the shifted coordinates, so the coincident and
    # zero-area rules carry over
    keys, dropped = MS.raster_ms(np.array(pts, np.int64), np.array(depth), faces, SIZE, TABLES[S])
    assert dropped == 0 and keys.shape == (SIZE, SIZE, S)
    ids = O.split_keys(keys)[0]
    if name == 'coincident':
        assert set(np.unique(ids)) == {-1, 0}
    if name == 'zero_area':
        assert not np.isin(ids, (0, 1, 2)).any()
    if name == 'edge_through_samples':
        # the samples ON the shared vertical edge belong to exactly one of the two triangles (the one it is a left
        # edge of), in both patterns
        s_on = [s for s, (ox, _) in enumerate(TABLES[S]) if ox == 32]
        assert len(s_on) == 1
        col = ids[:, 3, s_on[0]]
        assert (col >= 0).all() and len(set(col.tolist())) == 1


def test_one_sample_plane_is_the_one_sample_rasteriser():
    pts, faces, depth = CASES['fan_opposite_windings']
    keys, _ = MS.raster_ms(np.array(pts), np.array(depth), faces, SIZE, TABLES[1])
    want, _ = O.raster(np.array(pts), np.array(depth), faces, SIZE)
    assert np.array_equal(keys[:, :, 0], want)
    # dropped vertices keep their marker under the shift and drop their triangles once, not once per sample
    sxy = np.array([(P, P), (6 * P, P), (P, 6 * P), (O.DROPPED, 0)], np.int64)
    keys, dropped = MS.raster_ms(sxy, np.full(4, 0.5), [(0, 1, 2), (0, 1, 3), (3, 3, 3)], SIZE, TABLES[4])
    assert dropped == 2 and set(np.unique(O.split_keys(keys)[0])) == {-1, 0}


@pytest.mark.parametrize('S', [4, 16])
def test_shared_edges_cover_every_sample_exactly_once(S):
    """The random fans of the one-sample test: the triangles tile the polygon, so per sample plane the per-triangle
    coverages are disjoint and their union is the polygon's."""
    rng = np.random.default_rng(3)
    done = 0
    for trial in range(8):
        n = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        if np.diff(np.concatenate([ang, ang[:1] + 2 * np.pi])).max() >= np.pi:
            continue
        rad = rng.uniform(1.5, 3.9, n)
        c = np.array([4 * P, 4 * P]) + rng.integers(-200, 200, 2)
        rim = np.rint(np.stack([np.cos(ang), np.sin(ang)], 1) * rad[:, None] * P).astype(np.int64) + c
        total = np.zeros((SIZE, SIZE, S), int)
        tris = []
        for k in range(n):
            tri = [tuple(c), tuple(rim[k]), tuple(rim[(k + 1) % n])]
            tris.append(tri)
            total += _coverage_ms(tri[::-1] if rng.random() < 0.5 else tri, SIZE, TABLES[S])
        assert total.max() <= 1
        for s in range(0, S, 5 if S == 16 else 1):         # the exact hull is slow: 4 of the 16 planes
            poly = np.zeros((SIZE, SIZE), bool)
            for tri in tris:
                poly |= _brute_coverage(tri, SIZE, *TABLES[S][s])
            assert np.array_equal(total[:, :, s].astype(bool), poly)
        done += 1
    assert done >= 3


def _half_plane(x_top, x_bottom, size):
    """Two triangles covering everything left of the edge from (x_top, 0) to (x_bottom, size P)."""
    far = -4 * P
    pts = [(far, 0), (x_top, 0), (x_bottom, size * P), (far, size * P)]
    return np.array(pts, np.int64), [(0, 1, 2), (0, 2, 3)]


@pytest.mark.parametrize('S', [4, 16])
def test_resolve_of_a_half_plane_edge(S):
    c, bg = 0.25, 1.0                                      # dyadic: every partial sum is exact
    # a vertical edge through column 3: the samples left of it are covered
    size = 8
    x_edge = 3 * P + 100
    sxy, faces = _half_plane(x_edge, x_edge, size)
    keys, _ = MS.raster_ms(sxy, np.full(4, 0.5), faces, size, TABLES[S])
    hit = O.split_keys(keys)[0] >= 0
    k_want = sum(1 for ox, _ in TABLES[S] if ox < 100)
    assert 0 < k_want < S and (hit[:, 3].sum(1) == k_want).all()
    assert (hit[:, :3].sum(2) == S).all() and (hit[:, 4:].sum(2) == 0).all()
    img = MS.resolve([np.full(hit.shape, c)] * 3, hit, [bg] * 3)
    k = hit.sum(2)
    want = np.floor(255.0 * (k * c + (S - k) * bg) / S + 0.5).astype(np.uint8)
    assert np.array_equal(img[..., 0], want) and np.array_equal(img[..., 1], want)
    assert img[0, 3, 0] == int(255.0 * (k_want * c + (S - k_want) * bg) / S + 0.5)
    # a slanted edge at size 16, one pixel to the left over the 16 rows (1/16 pixel, the 16-table's column width, per
    # row): every count 0 .. S occurs, and every pixel has its mixture's level
    size = 16
    sxy, faces = _half_plane(8 * P - 16, 7 * P - 16, size)
    keys, _ = MS.raster_ms(sxy, np.full(4, 0.5), faces, size, TABLES[S])
    hit = O.split_keys(keys)[0] >= 0
    k = hit.sum(2)
    assert set(np.unique(k)) == set(range(S + 1))
    img = MS.resolve([np.full(hit.shape, c)] * 3, hit, [bg] * 3)
    want = np.floor(255.0 * (k * c + (S - k) * bg) / S + 0.5).astype(np.uint8)
    assert np.array_equal(img[..., 2], want)
    assert len(np.unique(img)) == S + 1                    # S + 1 distinct levels between 64 and 255


def test_shade_ms_of_agreeing_samples_is_the_one_sample_shade():
    """face_colours restates render_oracle.shade: where all samples of every pixel carry the one-sample id, the
    resolve of S equal colours is exact and the image is render_oracle.shade's, bit for bit."""
    size = 9
    v = np.array([[-1, -1, 0], [1, -1, 0.3], [1, 1, 0], [-1, 1, -0.2]], np.float32)
    faces = [(0, 1, 2), (0, 2, 3)]
    pose = O.look_at((0.3, -0.2, 2.0))
    sxy, d, _, _ = O.project(v, pose, size, np.zeros(3), 1.0)
    ids = O.split_keys(O.raster(sxy, d, faces, size)[0])[0]
    assert (ids >= 0).any() and (ids < 0).any()
    want = O.shade(v, faces, ids, pose, size, np.zeros(3), 1.0, background=(0.2, 0.5, 0.9), base_color=(0.8, 0.3, 0.1))
    for S in (1, 4, 16):
        have = MS.shade_ms(v, faces, np.repeat(ids[:, :, None], S, 2), pose, size, np.zeros(3), 1.0,
                           background=(0.2, 0.5, 0.9), base_color=(0.8, 0.3, 0.1))
        assert np.array_equal(have, want), S
