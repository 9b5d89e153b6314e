"""numpy restatement of include/ssrlcv_hip.h "disparity mesh", items 1-6, with per-cell loops: written for clarity, not speed.
A mesh is (vertex_index uint32 (gh, gw), cells uint8 (gh - 1, gw - 1)); NONE marks a node without a vertex.  Every float
operation is a numpy float32 scalar operation, one rounding each, in the contract's order."""
import numpy as np

INVALID_BITS = np.uint32(0x7FC00000)
INVALID = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
NONE = np.uint32(0xFFFFFFFF)
f32 = np.float32

# the corners of a cell as (di, dj) from its corner a
A, B, C, D = (0, 0), (1, 0), (0, 1), (1, 1)
TRIANGLES = {False: ((A, C, D), (A, D, B)),   # diagonal a-d
             True: ((A, C, B), (B, C, D))}    # diagonal b-c
AROUND = ((-1, -1), (0, -1), (-1, 0), (0, 0))  # item 5: the cells around node (i, j), as offsets of their corner a


def grid(w, h, step):
    return ((w - 1) // step + 1 if w else 0), ((h - 1) // step + 1 if h else 0)


def nodes_of(disparity, step):
    """the disparities of the nodes (gh, gw): node (i, j) is pixel (i step, j step)"""
    return np.ascontiguousarray(disparity[::step, ::step])


def is_valid(d):
    return np.array(d, np.float32).view(np.uint32) != INVALID_BITS


def joined(p, q, max_jump):
    """item 2, for two VALID nodes' disparities"""
    with np.errstate(all="ignore"):
        return bool(np.abs(f32(p) - f32(q)) <= f32(max_jump))   # false for a NaN


def cell_byte(da, db, dc, dd, max_jump):
    """item 3: the byte of a cell from its four corners' disparities"""
    d = {A: f32(da), B: f32(db), C: f32(dc), D: f32(dd)}
    ok = {k: bool(is_valid(v)) for k, v in d.items()}
    if sum(ok.values()) < 3:
        return 0
    if all(ok.values()):
        with np.errstate(all="ignore"):
            bc = bool(np.abs(d[B] - d[C]) < np.abs(d[A] - d[D]))
    else:
        bc = ok[B] and ok[C] and not (ok[A] and ok[D])

    def edge(p, q):
        return ok[p] and ok[q] and joined(d[p], d[q], max_jump)

    byte = 0
    for t, (p, q, r) in enumerate(TRIANGLES[bc]):
        if edge(p, q) and edge(q, r) and edge(r, p):
            byte |= 1 << t
    return (byte | 4) if (byte and bc) else byte


def mesh(disparity, step, max_jump):
    """items 1 and 3 -> (vertex_index, cells, n_vertices)"""
    n = nodes_of(disparity, step)
    gh, gw = n.shape
    valid = is_valid(n)
    vertex_index = np.full((gh, gw), NONE, np.uint32)
    vertex_index[valid] = np.arange(int(valid.sum()), dtype=np.uint32)     # raster order
    cells = np.zeros((max(gh - 1, 0), max(gw - 1, 0)), np.uint8)
    for j in range(gh - 1):
        for i in range(gw - 1):
            cells[j, i] = cell_byte(n[j, i], n[j, i + 1], n[j + 1, i], n[j + 1, i + 1], max_jump)
    return vertex_index, cells, int(valid.sum())


def cell_triangles(cells, i, j):
    """the emitted triangles of cell (i, j), T0 before T1, as node triples ((i, j), (i, j), (i, j))"""
    byte = int(cells[j, i])
    out = []
    for t, tri in enumerate(TRIANGLES[bool(byte & 4)]):
        if byte >> t & 1:
            out.append(tuple((i + di, j + dj) for di, dj in tri))
    return out


def faces(vertex_index, cells):
    """item 4 -> uint32 (T, 3)"""
    out = []
    for j in range(cells.shape[0]):
        for i in range(cells.shape[1]):
            for tri in cell_triangles(cells, i, j):
                out.append([vertex_index[y, x] for x, y in tri])
    return np.array(out, np.uint32).reshape(-1, 3)


def normals(points, vertex_index, cells, out=None):
    """item 5.  points float32 (n, 3) -> float32 (n, 3); rows no node of the map names keep what `out` holds (zeros without)"""
    points = np.asarray(points, np.float32)
    n = len(points)
    res = np.zeros((n, 3), np.float32) if out is None else out
    gh, gw = vertex_index.shape
    with np.errstate(all="ignore"):
        for j in range(gh):
            for i in range(gw):
                me = vertex_index[j, i]
                if me >= n:
                    continue
                s = [f32(0), f32(0), f32(0)]
                for oi, oj in AROUND:
                    ci, cj = i + oi, j + oj
                    if not (0 <= ci < gw - 1 and 0 <= cj < gh - 1):
                        continue
                    for tri in cell_triangles(cells, ci, cj):
                        if (i, j) not in tri:
                            continue
                        ip, iq, ir = (vertex_index[y, x] for x, y in tri)
                        if ip >= n or iq >= n or ir >= n:
                            continue
                        u, v = points[iq] - points[ip], points[ir] - points[ip]
                        t = ((u[1] * v[2]) - (u[2] * v[1]), (u[2] * v[0]) - (u[0] * v[2]), (u[0] * v[1]) - (u[1] * v[0]))
                        s = [s[0] + t[0], s[1] + t[1], s[2] + t[2]]
                length = np.sqrt(((s[0] * s[0]) + (s[1] * s[1])) + (s[2] * s[2]))
                if length > 0 and np.isfinite(length):
                    res[me] = (s[0] / length, s[1] / length, s[2] / length)
                else:
                    res[me] = 0
    return res


def select(vertex_index, cells, n_vertices, kept_index):
    """item 6 -> (vertex_index, cells) of the restricted mesh (new arrays)"""
    new_of = np.full(n_vertices, NONE, np.uint32)
    for j, old in enumerate(np.asarray(kept_index, np.int64)):
        if old < n_vertices:
            new_of[old] = j
    vi = np.full(vertex_index.shape, NONE, np.uint32)
    has = vertex_index < n_vertices
    vi[has] = new_of[vertex_index[has]]
    out = cells.copy()
    for j in range(cells.shape[0]):
        for i in range(cells.shape[1]):
            byte = int(cells[j, i])
            keep = byte & 3
            for t, tri in enumerate(TRIANGLES[bool(byte & 4)]):
                if byte >> t & 1 and any(vi[j + dj, i + di] == NONE for di, dj in tri):
                    keep &= ~(1 << t)
            out[j, i] = (keep | (byte & 4)) if keep else 0
    return vi, out
