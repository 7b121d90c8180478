"""Generates evennicer-slam_amd/csrc/mc_tables.hpp: the marching-cubes case table of csrc/marching_cubes.hip.

The table is derived, not typed in.  For each of the 256 corner cases the crossing edges of every cube face are joined
into segments, the segments are chained into closed loops on the cube's surface and every loop is fan-triangulated.

Conventions (shared with csrc/marching_cubes.hip and tests/mc_numpy.py):
  corner c = x + 2y + 4z (bit c of the case set  <=>  that corner's value > level, "occupied");
  edge   e = 4*axis + j joins corner c0 (bit `axis` clear) to c0 | (1 << axis); j's bit 0 / bit 1 give c0's coordinate
             along the lower / higher of the two other axes.  The lattice point at c0 owns the edge.

Face rule: a face with two crossing edges gets one segment.  A face with four (the ambiguous face: its occupied corners
are diagonal) gets two segments, each cutting off one OCCUPIED corner, so the free region stays connected across the
face.  The rule reads only that face's four corner bits, so both cells that share a face draw the same segments on it
and the mesh has no cracks.

Winding: on a face with outward normal n, a segment p -> q is directed with the occupied side on its right seen from
outside (n . ((q - p) x (o - p)) < 0 for an occupied corner o on that side).  The loops then run so that a fan
triangle's right-hand normal points from occupied to free.

Fans: a loop's fan starts at the first vertex (in loop order from its lowest edge id) whose diagonals join no two
vertices lying on a common cube face; such a diagonal could be drawn by the neighbouring cell as well and make an edge of
four triangles.

    python tools/gen_mc_tables.py            # rewrites the header
    python tools/gen_mc_tables.py --check    # exits 1 if the committed header differs
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "evennicer-slam_amd", "csrc", "mc_tables.hpp")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_corners(e):
    """(c0, c1) of edge e."""
    axis, j = divmod(e, 4)
    u, v = [a for a in range(3) if a != axis]
    c0 = ((j & 1) << u) | (((j >> 1) & 1) << v)
    return c0, c0 | (1 << axis)


EDGES = [edge_corners(e) for e in range(12)]
EDGE_ID = {frozenset(p): e for e, p in enumerate(EDGES)}


def faces():
    """[(axis, side, cyclic corner list)] of the six cube faces."""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            base = side << axis
            cyc = [base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)]
            out.append((axis, side, cyc))
    return out


FACES = faces()
EDGE_FACES = [{f for f, (_, _, cyc) in enumerate(FACES) if set(EDGES[e]) <= set(cyc)} for e in range(12)]


def _mid(e):
    a, b = (corner_pos(c) for c in EDGES[e])
    return tuple((x + y) / 2 for x, y in zip(a, b))


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def face_segments(case, cyc):
    """[(edge, edge, occupied corner on the occupied side)] drawn on the face with corners `cyc` (cyclic order)."""
    occ = [(case >> c) & 1 for c in cyc]
    edge = [EDGE_ID[frozenset((cyc[k], cyc[(k + 1) % 4]))] for k in range(4)]
    crossing = [k for k in range(4) if occ[k] != occ[(k + 1) % 4]]
    if len(crossing) == 0:
        return []
    if len(crossing) == 2:
        o = cyc[occ.index(1)]
        return [(edge[crossing[0]], edge[crossing[1]], o)]
    # ambiguous face: cut off each occupied corner k (its two face edges are k-1 and k)
    return [(edge[(k - 1) % 4], edge[k], cyc[k]) for k in range(4) if occ[k]]


def case_loops(case):
    nxt = {}
    for axis, side, cyc in FACES:
        n = [0, 0, 0]
        n[axis] = 1 if side else -1
        for a, b, o in face_segments(case, cyc):
            p, q = _mid(a), _mid(b)
            s = sum(x * y for x, y in zip(n, _cross(_sub(q, p), _sub(corner_pos(o), p))))
            assert s != 0
            if s > 0:
                a, b = b, a
            assert a not in nxt, (case, a)
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, v = [], start
        while v not in seen:
            seen.add(v)
            loop.append(v)
            v = nxt[v]
        loops.append(loop)
    return loops


def _share_face(a, b):
    return bool(EDGE_FACES[a] & EDGE_FACES[b])


def fan(loop):
    k = len(loop)
    for r in range(k):
        rl = loop[r:] + loop[:r]
        if not any(_share_face(rl[0], rl[i]) for i in range(2, k - 1)):
            return [(rl[0], rl[i], rl[i + 1]) for i in range(1, k - 1)]
    raise AssertionError(f"no fan start for loop {loop}")


def case_triangles(case):
    return [t for loop in case_loops(case) for t in fan(loop)]


TRIS = [case_triangles(c) for c in range(256)]
MAX_TRIS = max(len(t) for t in TRIS)


def render():
    lines = ["// GENERATED by tools/gen_mc_tables.py -- do not edit; regenerate with `python tools/gen_mc_tables.py`.",
             "// Marching-cubes case table of marching_cubes.hip (conventions: the generator's docstring).",
             "#pragma once",
             "#include <stdint.h>",
             "",
             f"#define ENS_MC_MAX_TRIS {MAX_TRIS}",
             "",
             "// corner c0 (x + 2y + 4z) of edge e; the edge runs along axis e >> 2",
             "__device__ static const uint8_t mc_edge_c0[12] = {" + ", ".join(str(EDGES[e][0]) for e in range(12)) + "};",
             "",
             "// triangles per case",
             "__device__ static const uint8_t mc_tri_count[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(TRIS[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"// edge ids of each case's triangles, 3 per triangle, -1 beyond mc_tri_count")
    lines.append(f"__device__ static const int8_t mc_tri_edges[256][{3 * MAX_TRIS}] = {{")
    for c in range(256):
        flat = [e for t in TRIS[c] for e in t] + [-1] * (3 * (MAX_TRIS - len(TRIS[c])))
        lines.append("    {" + ", ".join(str(e) for e in flat) + f"}},  // {c}")
    lines.append("};")
    return "\n".join(lines) + "\n"


def main(argv):
    text = render()
    if "--check" in argv:
        with open(OUT) as f:
            same = f.read() == text
        print("mc_tables.hpp is current" if same else "mc_tables.hpp differs from the generator's output")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}: max {MAX_TRIS} triangles per case")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
