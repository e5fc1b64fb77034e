"""Generate octfusion_amd/csrc/ofx_mc_table.h: the marching-cubes triangulation table of csrc/ofx_mesh.hip.

    python tools/gen_mc_table.py            # rewrites the header
    python tools/gen_mc_table.py --check    # exits 1 if the committed header differs

The table is derived, not typed in.  For each of the 256 sign cases every cube face contributes iso-line segments:
a face with two crossing edges gets one segment; an ambiguous face (diagonal corners alike, four crossing edges)
always SEPARATES its inside corners -- a rule that depends only on that face's four signs, so the two cells sharing a
face cut it identically.  Each segment is oriented so that (b - a) x n_out points to the inside side of the face.
Every crossing edge then has exactly one outgoing and one incoming segment; the loops are followed from their lowest
edge id and fanned from their first vertex.  A segment a -> b of one cell is b -> a in its neighbour, so the mesh is
closed wherever the field does not reach the lattice boundary, and every triangle's normal points to increasing values.

Conventions (shared with the kernel and the tests' oracle):
  corner c = dx*4 + dy*2 + dz; cube index bit c set iff corner c is inside (v < level).
  edge e = axis*4 + k, axis 0/1/2 = x/y/z; k's two bits are the owner corner's coordinates on the other two axes in
  x, y, z order (hi bit first); the edge runs from the owner corner along +axis.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'octfusion_amd', 'csrc', 'ofx_mc_table.h')


def corner_xyz(c):
    return ((c >> 2) & 1, (c >> 1) & 1, c & 1)


def edge_owner(e):
    """(owner corner xyz, axis) of edge e."""
    axis, k = e >> 2, e & 3
    others = [a for a in range(3) if a != axis]
    xyz = [0, 0, 0]
    xyz[others[0]] = (k >> 1) & 1
    xyz[others[1]] = k & 1
    return tuple(xyz), axis


def edge_ends(e):
    o, axis = edge_owner(e)
    b = list(o)
    b[axis] += 1
    return o, tuple(b)


def cidx(xyz):
    return xyz[0] * 4 + xyz[1] * 2 + xyz[2]


def edge_mid(e):
    a, b = edge_ends(e)
    return tuple((a[i] + b[i]) / 2.0 for i in range(3))


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def dot(u, v):
    return sum(a * b for a, b in zip(u, v))


def sub(u, v):
    return tuple(a - b for a, b in zip(u, v))


EDGES = list(range(12))


def faces():
    """(outward normal, corner ids, edge ids) of the six faces."""
    out = []
    for axis in range(3):
        for s in (0, 1):
            n = [0, 0, 0]
            n[axis] = 1 if s else -1
            cs = [c for c in range(8) if corner_xyz(c)[axis] == s]
            es = [e for e in EDGES if (e >> 2) != axis and edge_owner(e)[0][axis] == s]
            out.append((tuple(n), cs, es))
    return out


def case_segments(case):
    inside = [(case >> c) & 1 for c in range(8)]
    segs = []
    for n, cs, es in faces():
        cross_e = [e for e in es if inside[cidx(edge_ends(e)[0])] != inside[cidx(edge_ends(e)[1])]]
        if not cross_e:
            continue
        if len(cross_e) == 4:
            # ambiguous face: one segment around each inside corner (inside corners separated)
            pairs = []
            for c in cs:
                if inside[c]:
                    pairs.append([e for e in es if c in (cidx(edge_ends(e)[0]), cidx(edge_ends(e)[1]))])
        else:
            pairs = [cross_e]
        for ea, eb in pairs:
            a, b = edge_mid(ea), edge_mid(eb)
            mid = tuple((a[i] + b[i]) / 2 for i in range(3))
            w = cross(sub(b, a), n)
            pos = [c for c in cs if dot(sub(corner_xyz(c), mid), w) > 0]
            neg = [c for c in cs if dot(sub(corner_xyz(c), mid), w) < 0]
            assert len(pos) + len(neg) == 4
            if len(pos) == 1:
                pos_inside = bool(inside[pos[0]])
            elif len(neg) == 1:
                pos_inside = not inside[neg[0]]
            else:
                assert len(pos) == 2 and inside[pos[0]] == inside[pos[1]] != inside[neg[0]]
                pos_inside = bool(inside[pos[0]])
            segs.append((ea, eb) if pos_inside else (eb, ea))
    return segs


def case_triangles(case):
    nxt = {}
    for a, b in case_segments(case):
        assert a not in nxt, (case, a)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), case
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3, (case, loop)
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def table():
    return [case_triangles(c) for c in range(256)]


def render():
    tab = table()
    mt = max(len(t) for t in tab)
    width = 3 * mt + 1
    lines = ['// Generated by tools/gen_mc_table.py -- do not edit.',
             '// Marching-cubes triangulation: ambiguous faces separate their inside corners (face-consistent, closed).',
             '// corner c = dx*4 + dy*2 + dz; edge e = axis*4 + k (k: owner coordinates on the other two axes, hi first).',
             '#pragma once',
             '#include <stdint.h>',
             '',
             '#define OFX_MC_MAX_TRI %d' % mt,
             '#define OFX_MC_TRI_STRIDE %d' % width,
             '',
             'static constexpr uint8_t OFX_MC_NTRI[256] = {']
    for r in range(0, 256, 32):
        lines.append('    ' + ', '.join(str(len(tab[c])) for c in range(r, r + 32)) + ',')
    lines.append('};')
    lines.append('')
    lines.append('// [case][3 * OFX_MC_MAX_TRI + 1] edge ids, -1 padded')
    lines.append('static constexpr int8_t OFX_MC_TRI[256][OFX_MC_TRI_STRIDE] = {')
    for c in range(256):
        flat = [e for t in tab[c] for e in t]
        flat += [-1] * (width - len(flat))
        lines.append('    {' + ', '.join(str(v) for v in flat) + '},')
    lines.append('};')
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    text = render()
    if '--check' in sys.argv:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print('ofx_mc_table.h up to date' if same else 'ofx_mc_table.h differs from the generator')
        sys.exit(0 if same else 1)
    with open(OUT, 'w') as f:
        f.write(text)
    print(OUT)
