"""fp64 numpy restatement of the TSDF fusion and marching-tetrahedra contract (rc_mvsnet_amd/csrc/tsdf_mesh.h, arithmetic as
csrc/tsdf_mesh_math.h writes it): the same correctly rounded operations in the same order, so the kernels' planes, vertices,
colours and faces can be demanded equal in every bit.  Vectorised over voxels; nothing here reads the header's tables -- the 16
cases of a tetrahedron are derived from the parity rule (case_table), and tests/test_tsdf_mesh_cpu.py compares the header's."""
import itertools

import numpy as np

MAX_VIEWS = 16
# the Kuhn split of a cube along its 0-7 diagonal; corner code dx + 2 dy + 4 dz
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))


def corner_offset(code):
    return np.array([code & 1, (code >> 1) & 1, (code >> 2) & 1])


def parity(p):
    s = 1
    for i, j in itertools.combinations(range(len(p)), 2):
        if p[i] > p[j]:
            s = -s
    return s


def tet_signs():
    """sign of det [P1 - P0, P2 - P0, P3 - P0] of each tetrahedron"""
    out = []
    for tet in TETS:
        P = [corner_offset(c).astype(np.float64) for c in tet]
        out.append(int(np.sign(np.linalg.det(np.stack([P[1] - P[0], P[2] - P[0], P[3] - P[0]])))))
    return tuple(out)


def case_table():
    """case (bit c = local corner c inside) -> list of triangles, each three edges (a, b), a < b local corners, in the order a
    tetrahedron of POSITIVE determinant emits them (a negative one swaps the last two edges of every triangle).
    One corner apart: the triangle over the three edges from it, the other corners ascending; its normal points away from
    that corner when (determinant) x (parity of [corner] + others) is positive, which is outward when the corner is the inside
    one and inward when it is the outside one.  Two and two: the quad (i0o0, i0o1, i1o1, i1o0) split as (q0,q1,q2), (q0,q2,q3),
    kept when (determinant) x (parity of [i0, i1, o0, o1]) is positive."""
    table = []
    for m in range(16):
        ins = [c for c in range(4) if m >> c & 1]
        out = [c for c in range(4) if not m >> c & 1]
        edge = lambda a, b: (min(a, b), max(a, b))                                  # noqa: E731
        if len(ins) in (0, 4):
            table.append([])
            continue
        if len(ins) == 1:
            tris, sign = [[edge(ins[0], j) for j in out]], parity(ins + out)
        elif len(ins) == 3:
            tris, sign = [[edge(out[0], j) for j in ins]], -parity(out + ins)
        else:
            (i0, i1), (o0, o1) = ins, out
            q = [edge(i0, o0), edge(i0, o1), edge(i1, o1), edge(i1, o0)]
            tris, sign = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]], parity(ins + out)
        if sign < 0:
            tris = [[t[0], t[2], t[1]] for t in tris]
        table.append(tris)
    return table


# ---- integration ------------------------------------------------------------------------------------------------------------
def new_state(dims, colour=True):
    n = int(dims[0]) * int(dims[1]) * int(dims[2])
    return {"dsum": np.zeros(n, np.float32), "wsum": np.zeros(n, np.float32),
            "csum": np.zeros((3, n), np.float32) if colour else None}


def centres(grid, dims):
    """-> (px, py, pz) fp64 per voxel, voxels numbered x fastest: o + (idx + 0.5) * h"""
    ox, oy, oz, h = [np.float64(v) for v in grid]
    gx, gy, gz = [int(v) for v in dims]
    n = np.arange(gx * gy * gz)
    i, j, k = n % gx, (n // gx) % gy, n // (gx * gy)
    return (ox + (i.astype(np.float64) + 0.5) * h, oy + (j.astype(np.float64) + 0.5) * h, oz + (k.astype(np.float64) + 0.5) * h)


def integrate(state, depth, cams, rgb, trunc, grid, dims):
    """depth (n,H,W) fp32, cams (n,16) fp64 {R 9, t 3, fx, fy, cx, cy}, rgb (n,H,W,3) uint8 or None: any n, view after view (one
    fp32 add per view, so the chunking of the kernel cannot matter)"""
    depth = np.asarray(depth, np.float32)
    n, H, W = depth.shape
    cams = np.asarray(cams, np.float64).reshape(n, 16)
    px, py, pz = centres(grid, dims)
    trunc = np.float64(trunc)
    with np.errstate(all="ignore"):
        for v in range(n):
            c = cams[v]
            xc = ((c[0] * px + c[1] * py) + c[2] * pz) + c[9]
            yc = ((c[3] * px + c[4] * py) + c[5] * pz) + c[10]
            zc = ((c[6] * px + c[7] * py) + c[8] * pz) + c[11]
            u = c[12] * (xc / zc) + c[14]
            w = c[13] * (yc / zc) + c[15]
            ub, wb = u + 0.5, w + 0.5
            ok = (zc > 0) & (ub >= 0) & (ub < W) & (wb >= 0) & (wb < H)
            ix = np.where(ok, np.floor(ub), 0).astype(np.int64)
            iy = np.where(ok, np.floor(wb), 0).astype(np.int64)
            d = depth[v][iy, ix]
            ok &= np.isfinite(d) & (d > 0)
            sdf = d.astype(np.float64) - zc
            ok &= ~(sdf < -trunc)
            val = sdf / trunc
            val = np.where(val > 1.0, 1.0, val)
            state["dsum"][ok] = state["dsum"][ok] + val[ok].astype(np.float32)
            state["wsum"][ok] = state["wsum"][ok] + np.float32(1.0)
            if rgb is not None and state["csum"] is not None:
                col = rgb[v][iy, ix]
                for ch in range(3):
                    state["csum"][ch][ok] = state["csum"][ch][ok] + col[ok, ch].astype(np.float32)
    return state


# ---- extraction -------------------------------------------------------------------------------------------------------------
def extract(dsum, wsum, csum, grid, dims, min_weight=1, sparse=False):
    """-> dict: verts (nv,3) fp32, rgb (nv,3) uint8 or None, faces (nf,3) int32, edge_mask, tri_count (uint8 per voxel),
    vert_start, tri_start (voxels + 1, int64).  sparse: only cubes with mixed signs are visited (the same result)."""
    gx, gy, gz = [int(v) for v in dims]
    n = gx * gy * gz
    shape = (gz, gy, gx)
    d = np.asarray(dsum, np.float32).astype(np.float64).reshape(shape)
    w = np.asarray(wsum, np.float32).reshape(shape)
    with np.errstate(all="ignore"):
        val = d / w.astype(np.float64)
    obs = w >= np.float32(min_weight)
    ins = obs & (val < 0)
    ox, oy, oz, h = [np.float64(v) for v in grid]

    def lower(a, code):
        """the part of array a (indexed k, j, i) at the lower voxels of the edges / cubes towards `code`"""
        dx, dy, dz = code & 1, code >> 1 & 1, code >> 2 & 1
        return a[:gz - dz, :gy - dy, :gx - dx]

    def upper(a, code):
        dx, dy, dz = code & 1, code >> 1 & 1, code >> 2 & 1
        return a[dz:, dy:, dx:]

    edge_mask = np.zeros(shape, np.uint8)
    for code in range(1, 8):
        has = lower(obs, code) & upper(obs, code) & (lower(ins, code) != upper(ins, code))
        lower(edge_mask, code)[...] |= (has.astype(np.uint8) << (code - 1)).astype(np.uint8)
    flat_mask = edge_mask.ravel()
    per_voxel = np.array([bin(m).count("1") for m in range(128)], np.int64)[flat_mask]
    vert_start = np.concatenate([[0], np.cumsum(per_voxel)])

    # vertices, ordered by (owner voxel, edge code)
    owners, codes = [], []
    for code in range(1, 8):
        own = np.nonzero(flat_mask >> (code - 1) & 1)[0]
        owners.append(own)
        codes.append(np.full(len(own), code))
    owners, codes = np.concatenate(owners), np.concatenate(codes)
    order = np.lexsort((codes, owners))
    owners, codes = owners[order], codes[order]
    ai, aj, ak = owners % gx, (owners // gx) % gy, owners // (gx * gy)
    bi, bj, bk = ai + (codes & 1), aj + (codes >> 1 & 1), ak + (codes >> 2 & 1)
    b = bi + gx * (bj + gy * bk)
    vflat = val.ravel()
    da, db = vflat[owners], vflat[b]
    t = da / (da - db)
    verts = np.empty((len(owners), 3), np.float32)
    for axis, (o, ia, ib) in enumerate(((ox, ai, bi), (oy, aj, bj), (oz, ak, bk))):
        pa = o + (ia.astype(np.float64) + 0.5) * h
        pb = o + (ib.astype(np.float64) + 0.5) * h
        verts[:, axis] = (pa + t * (pb - pa)).astype(np.float32)
    rgb = None
    if csum is not None:
        rgb = np.empty((len(owners), 3), np.uint8)
        wflat = w.ravel().astype(np.float64)
        for ch in range(3):
            with np.errstate(all="ignore"):
                c = np.asarray(csum[ch], np.float32).astype(np.float64) / wflat
            x = np.floor((c[owners] + t * (c[b] - c[owners])) + 0.5)
            rgb[:, ch] = np.clip(x, 0.0, 255.0).astype(np.uint8)

    # faces, ordered by (cube, tetrahedron, triangle)
    table, signs = case_table(), tet_signs()
    cube_ok = np.zeros(shape, bool)
    cube_ok[:max(gz - 1, 0), :max(gy - 1, 0), :max(gx - 1, 0)] = True
    cubes = np.nonzero(cube_ok.ravel())[0]
    if sparse and len(cubes):
        ci, cj, ck = cubes % gx, (cubes // gx) % gy, cubes // (gx * gy)
        cnt = np.zeros(len(cubes), np.int64)
        for code in range(8):
            cnt += ins[ck + (code >> 2 & 1), cj + (code >> 1 & 1), ci + (code & 1)]
        cubes = cubes[(cnt > 0) & (cnt < 8)]         # a cube whose corners are all inside or all not inside emits nothing
    ci, cj, ck = cubes % gx, (cubes // gx) % gy, cubes // (gx * gy)
    corner = [(ci + (code & 1)) + gx * ((cj + (code >> 1 & 1)) + gy * (ck + (code >> 2 & 1))) for code in range(8)]
    obs_f, ins_f = obs.ravel(), ins.ravel()
    rows = []                                        # (cube, tet, tri, v0, v1, v2) blocks
    for ti, tet in enumerate(TETS):
        all_obs = np.ones(len(cubes), bool)
        case = np.zeros(len(cubes), np.int64)
        for c in range(4):
            all_obs &= obs_f[corner[tet[c]]]
            case |= ins_f[corner[tet[c]]].astype(np.int64) << c
        for m in range(1, 15):
            sel = np.nonzero(all_obs & (case == m))[0]
            if not len(sel):
                continue
            for k, tri in enumerate(table[m]):
                if signs[ti] < 0:
                    tri = [tri[0], tri[2], tri[1]]
                idx = []
                for a, bb in tri:
                    ca, cb = tet[a], tet[bb]
                    own = corner[ca][sel]
                    code = cb ^ ca
                    assert ca & cb == ca and code > 0
                    idx.append(vert_start[own] + per_voxel_below(flat_mask[own], code))
                rows.append(np.stack([cubes[sel], np.full(len(sel), ti), np.full(len(sel), k)] + idx, axis=1))
    if rows:
        rows = np.concatenate(rows, 0)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        faces = rows[:, 3:].astype(np.int32)
        tri_count = np.bincount(rows[:, 0], minlength=n).astype(np.uint8)
    else:
        faces, tri_count = np.zeros((0, 3), np.int32), np.zeros(n, np.uint8)
    tri_start = np.concatenate([[0], np.cumsum(tri_count.astype(np.int64))])
    return {"verts": verts, "rgb": rgb, "faces": faces, "edge_mask": flat_mask, "tri_count": tri_count,
            "vert_start": vert_start, "tri_start": tri_start, "observed": int(obs.sum())}


_POP = np.array([bin(m).count("1") for m in range(128)], np.int64)


def per_voxel_below(mask, code):
    """number of the owner's vertices before the one on edge `code`"""
    return _POP[mask & ((1 << (code - 1)) - 1)]


# ---- checks of a mesh ----------------------------------------------------------------------------------------------------
def closed_and_oriented(faces):
    """every directed edge occurs once and its reverse once -> (ok, Euler characteristic V - E + F over referenced vertices)"""
    f = np.asarray(faces, np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = de[:, 0] * (f.max() + 1) + de[:, 1]
    rev = de[:, 1] * (f.max() + 1) + de[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    ok = bool((counts == 1).all() and np.array_equal(np.sort(rev), uniq))
    V = len(np.unique(f))
    return ok, V - len(uniq) // 2 + len(f)


def normals_outward(verts, faces, centre):
    """-> (outward, inward, degenerate) counts of (v1 - v0) x (v2 - v0) against the direction from `centre`"""
    v = np.asarray(verts, np.float64)
    nrm = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    dots = (nrm * (v[faces].mean(1) - np.asarray(centre, np.float64))).sum(1)
    deg = (nrm == 0).all(1)
    return int((dots[~deg] > 0).sum()), int((dots[~deg] <= 0).sum()), int(deg.sum())
