"""Readers for the DTU scorer (rc_mvsnet_amd/dtu_eval.py): PLY vertex positions and MATLAB v5 .mat files.

``read_ply_xyz``: ascii, binary_little_endian and binary_big_endian PLY, any scalar property types; returns the vertex element's
x / y / z as (n,3) float32 and skips every other property and element (faces after the vertices included).  It reads what
``fusion.ply_bytes`` writes and DTU's ``Points/stl/stl%03d_total.ply``.  ``read_ply_mesh``: the vertices and the triangles of
a mesh PLY (the 'Surfaces' input of the scorer, what ``plyread.m`` gives MeshSupSamp).

``read_mat``: the MAT-file level 5 format (uncompressed and zlib-compressed variables), full numeric and logical arrays only,
so that scipy is not a runtime dependency.  Arrays come back in MATLAB's index order (``a[i-1, j-1, k-1]`` is ``A(i,j,k)``).
Other classes (cell, struct, char, sparse, objects) are skipped.  v7.3 files (HDF5) are refused with a clear error.
"""
import struct
import zlib

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


class FormatError(ValueError):
    pass


def _ply_header(f):
    if f.readline().strip() != b"ply":
        raise FormatError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise FormatError("PLY header without end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "end_header":
            break
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise FormatError("PLY property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], ("list", _ply_type(tok[2]), _ply_type(tok[3]))))
            else:
                elements[-1][2].append((tok[2], _ply_type(tok[1])))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise FormatError(f"PLY format {fmt!r}")
    return fmt, elements


def _ply_type(name):
    if name not in _PLY_TYPES:
        raise FormatError(f"PLY property type {name!r}")
    return _PLY_TYPES[name]


def _skip_binary_element(f, count, props, end):
    """Skip one binary element (list properties read item by item)."""
    if all(not isinstance(t, tuple) for _, t in props):
        f.seek(count * sum(np.dtype(t).itemsize for _, t in props), 1)
        return
    for _ in range(count):
        for _, t in props:
            if isinstance(t, tuple):
                cdt = np.dtype(t[1]).newbyteorder(end)
                k = int(np.frombuffer(f.read(cdt.itemsize), dtype=cdt)[0])
                f.seek(k * np.dtype(t[2]).itemsize, 1)
            else:
                f.seek(np.dtype(t).itemsize, 1)


def read_ply_xyz(path):
    """-> (n,3) float32 vertex positions of a PLY file."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f)
        names = [e[0] for e in elements]
        if "vertex" not in names:
            raise FormatError(f"{path}: no vertex element")
        vprops = elements[names.index("vertex")][2]
        pnames = [p for p, _ in vprops]
        for k in ("x", "y", "z"):
            if k not in pnames:
                raise FormatError(f"{path}: vertex has no property {k}")
        if any(isinstance(t, tuple) for _, t in vprops):
            raise FormatError(f"{path}: list properties in the vertex element are not supported")
        if fmt == "ascii":
            lines = f.read().decode("ascii").splitlines()
            row = 0
            for name, count, props in elements:
                if name == "vertex":
                    rows = [ln.split() for ln in lines[row:row + count]]
                    if len(rows) != count:
                        raise FormatError(f"{path}: {len(rows)} of {count} vertices")
                    cols = [pnames.index(k) for k in ("x", "y", "z")]
                    return np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).astype(np.float32).reshape(count, 3)
                row += count
        end = "<" if fmt == "binary_little_endian" else ">"
        for name, count, props in elements:
            if name == "vertex":
                dt = np.dtype([(p, np.dtype(t).newbyteorder(end)) for p, t in props])
                buf = f.read(dt.itemsize * count)
                if len(buf) != dt.itemsize * count:
                    raise FormatError(f"{path}: truncated vertex data")
                rec = np.frombuffer(buf, dtype=dt)
                return np.stack([rec[k].astype(np.float32) for k in ("x", "y", "z")], axis=1)
            _skip_binary_element(f, count, props, end)
    raise FormatError(f"{path}: no vertex element")       # not reached


_FACE_ELEMENTS = ("face", "Face", "poly", "Poly", "tri", "Tri")                        # the names plyread.m looks for
_INDEX_PROPS = ("vertex_indices", "vertex_indexes", "vertex_index", "indices", "indexes")


def _ascii_rows(tokens, pos, count, props, path, what):
    """count rows of one ascii element from the token stream: -> (rows, each a list of per-property values, new pos)"""
    rows = []
    for _ in range(count):
        row = []
        for _, t in props:
            if pos >= len(tokens):
                raise FormatError(f"{path}: truncated {what} data")
            if isinstance(t, tuple):
                k = int(tokens[pos])
                row.append(tokens[pos + 1:pos + 1 + k])
                pos += 1 + k
            else:
                row.append(tokens[pos])
                pos += 1
        rows.append(row)
    return rows, pos


def _fixed_face_records(f, count, props, end):
    """A binary element whose list properties have the same lengths in every record, read at once -> the records (list i: its count
    as "n<i>", its items as "l<i>"; scalar i as "p<i>"), the file left after the element; None, the file where it was, when the
    lengths differ or the data is short.  The lengths are those of the first record."""
    here = f.tell()
    fields = []
    for i, (_, t) in enumerate(props):
        if isinstance(t, tuple):
            cdt, idt = np.dtype(t[1]).newbyteorder(end), np.dtype(t[2]).newbyteorder(end)
            b = f.read(cdt.itemsize)
            if len(b) != cdt.itemsize:
                f.seek(here)
                return None
            k = int(np.frombuffer(b, dtype=cdt)[0])
            f.seek(k * idt.itemsize, 1)
            fields += [(f"n{i}", cdt), (f"l{i}", idt, (k,))]
        else:
            fields.append((f"p{i}", np.dtype(t).newbyteorder(end)))
            f.seek(fields[-1][1].itemsize, 1)
    dt = np.dtype(fields)
    f.seek(here)
    buf = f.read(dt.itemsize * count)
    if len(buf) == dt.itemsize * count:
        rec = np.frombuffer(buf, dtype=dt)
        if all(bool((rec[name] == rec[name][0]).all()) for name, *_ in fields if name[0] == "n"):
            return rec
    f.seek(here)
    return None


def read_ply_mesh_texture(path):
    """read_ply_mesh_normals plus the per-face texture coordinates of a PLY that tsdf_mesh.mesh_ply_bytes wrote with ``texcoords``
    -> (verts, faces, rgb or None, normals or None, texcoords (m,3,2) float32 with their bits as stored or None, the name after
    ``comment TextureFile`` or None).  The coordinates are the face element's list ``texcoord`` of six floats per face (binary
    files); anything else gives None."""
    verts, faces, rgb, nrm = _read_ply_mesh(path, True, True)
    uv, name = None, None
    with open(path, "rb") as f:
        for line in f:
            tok = line.decode("ascii", "replace").split()
            if tok[:2] == ["comment", "TextureFile"] and len(tok) == 3:
                name = tok[2]
            if tok[:1] == ["end_header"]:
                break
        f.seek(0)
        fmt, elements = _ply_header(f)
        names = [e[0] for e in elements]
        face_name = next((k for k in _FACE_ELEMENTS if k in names), None)
        if fmt != "ascii" and face_name is not None:
            end = "<" if fmt == "binary_little_endian" else ">"
            for ename, count, props in elements:
                if ename != face_name:
                    _skip_binary_element(f, count, props, end)
                    continue
                at = next((i for i, (p, t) in enumerate(props) if p == "texcoord" and isinstance(t, tuple) and np.dtype(t[2]) == np.float32), None)
                if at is not None and count:
                    rec = _fixed_face_records(f, count, props, end)
                    if rec is not None and rec[f"n{at}"][0] == 6:
                        uv = rec[f"l{at}"].astype("<f4").astype(np.float32).reshape(count, 3, 2)
                elif at is not None:
                    uv = np.zeros((0, 3, 2), np.float32)
                break
    return verts, faces, rgb, nrm, uv, name


def _binary_faces(f, count, props, idx, end, path):
    """-> (count, 3) int64 indices of a binary face element; a single list property with 3 indices per face is read at once"""
    lists = [i for i, (_, t) in enumerate(props) if isinstance(t, tuple)]
    if lists == [idx]:
        _, cnt_t, idx_t = props[idx][1]
        fields = [(f"p{i}", np.dtype(t).newbyteorder(end)) for i, (_, t) in enumerate(props) if i != idx]
        fields.insert(idx, ("n", np.dtype(cnt_t).newbyteorder(end)))
        fields.insert(idx + 1, ("i", np.dtype(idx_t).newbyteorder(end), (3,)))
        dt = np.dtype(fields)
        here = f.tell()
        buf = f.read(dt.itemsize * count)
        rec = np.frombuffer(buf[:len(buf) - len(buf) % dt.itemsize], dtype=dt)
        bad = np.nonzero(rec["n"] != 3)[0]
        if len(rec) == count and not len(bad):
            return rec["i"].astype(np.int64)
        # the first face that is not a triangle was read at its true offset: name it
        k = int(bad[0]) if len(bad) else None
        if k is not None:
            raise FormatError(f"{path}: face {k} has {int(rec['n'][k])} vertices (only triangles are supported)")
        f.seek(here)
    elif count:
        rec = _fixed_face_records(f, count, props, end)              # several lists (a textured PLY's texcoord): every face the same lengths
        if rec is not None:
            if int(rec[f"n{idx}"][0]) != 3:
                raise FormatError(f"{path}: face 0 has {int(rec[f'n{idx}'][0])} vertices (only triangles are supported)")
            return rec[f"l{idx}"].astype(np.int64)
    out = np.empty((count, 3), dtype=np.int64)
    for r in range(count):
        for i, (_, t) in enumerate(props):
            if isinstance(t, tuple):
                cdt = np.dtype(t[1]).newbyteorder(end)
                b = f.read(cdt.itemsize)
                if len(b) != cdt.itemsize:
                    raise FormatError(f"{path}: truncated face data")
                k = int(np.frombuffer(b, dtype=cdt)[0])
                idt = np.dtype(t[2]).newbyteorder(end)
                b = f.read(k * idt.itemsize)
                if len(b) != k * idt.itemsize:
                    raise FormatError(f"{path}: truncated face data")
                if i == idx:
                    if k != 3:
                        raise FormatError(f"{path}: face {r} has {k} vertices (only triangles are supported)")
                    out[r] = np.frombuffer(b, dtype=idt)
            else:
                f.seek(np.dtype(t).itemsize, 1)
    return out


def read_ply_mesh(path):
    """-> (verts (n,3) float32, faces (m,3) int32) of a triangle mesh PLY (ascii or binary, either byte order).  The faces are
    the first element plyread.m would take (face, Face, poly, Poly, tri, Tri) with its index list (vertex_indices,
    vertex_indexes, vertex_index, indices, indexes; any integer types); other properties are skipped.  No face element gives
    (0,3) faces.  Refused with FormatError: non-triangle faces, indices outside 0 .. n-1, non-finite vertices."""
    return _read_ply_mesh(path, False)[:2]


def read_ply_mesh_rgb(path):
    """read_ply_mesh plus the vertex colours, in the same single pass -> (verts, faces, rgb (n,3) uint8 or None).  The colours are
    the vertex element's red green blue (or r g b, or diffuse_red diffuse_green diffuse_blue) when all three are there as uchar;
    anything else gives None."""
    return _read_ply_mesh(path, True)


_COLOUR_PROPS = (("red", "green", "blue"), ("r", "g", "b"), ("diffuse_red", "diffuse_green", "diffuse_blue"))


def read_ply_mesh_normals(path):
    """read_ply_mesh_rgb plus the vertex normals, in the same single pass -> (verts, faces, rgb (n,3) uint8 or None, normals (n,3)
    float32 or None).  The normals are the vertex element's nx ny nz when all three are there as floating-point properties, with
    their bits as stored when they are float; anything else gives None."""
    return _read_ply_mesh(path, True, True)


def read_ply_cloud_normals(path):
    """A point cloud that fusion.ply_bytes wrote -> (xyz (n,3) float32, rgb (n,3) uint8 or None, normals (n,3) float32 or None, with
    their bits as stored): read_ply_mesh_normals without the faces."""
    verts, _, rgb, nrm = _read_ply_mesh(path, True, True)
    return verts, rgb, nrm


def _read_ply_mesh(path, colours, normals=False):
    """the reader behind read_ply_mesh, read_ply_mesh_rgb and read_ply_mesh_normals -> (verts, faces, rgb or None), with normals
    (verts, faces, rgb or None, normals or None); colours False: rgb is not looked for"""
    rgb, nrm = None, None
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f)
        names = [e[0] for e in elements]
        if "vertex" not in names:
            raise FormatError(f"{path}: no vertex element")
        face_name = next((k for k in _FACE_ELEMENTS if k in names), None)
        vprops = elements[names.index("vertex")][2]
        pnames = [p for p, _ in vprops]
        for k in ("x", "y", "z"):
            if k not in pnames:
                raise FormatError(f"{path}: vertex has no property {k}")
        if any(isinstance(t, tuple) for _, t in vprops):
            raise FormatError(f"{path}: list properties in the vertex element are not supported")
        triple = next((t for t in _COLOUR_PROPS if all(k in pnames and np.dtype(vprops[pnames.index(k)][1]) == np.uint8 for k in t)), None) if colours else None
        ntriple = ("nx", "ny", "nz") if normals and all(k in pnames and np.dtype(vprops[pnames.index(k)][1]).kind == "f" for k in ("nx", "ny", "nz")) else None
        idx = None
        if face_name is not None:
            fprops = elements[names.index(face_name)][2]
            fnames = [p for p, _ in fprops]
            idx = next((fnames.index(k) for k in _INDEX_PROPS if k in fnames), None)
            if idx is None or not isinstance(fprops[idx][1], tuple):
                raise FormatError(f"{path}: element {face_name} has no vertex index list")
            if np.dtype(fprops[idx][1][2]).kind not in "iu" or np.dtype(fprops[idx][1][1]).kind not in "iu":
                raise FormatError(f"{path}: face indices must be integers")
        verts, faces = None, np.zeros((0, 3), dtype=np.int64)
        if fmt == "ascii":
            tokens = f.read().decode("ascii").split()
            pos = 0
            for name, count, props in elements:
                rows, pos = _ascii_rows(tokens, pos, count, props, path, name)
                if name == "vertex":
                    cols = [pnames.index(k) for k in ("x", "y", "z")]
                    verts = np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).astype(np.float32).reshape(count, 3)
                    if triple is not None:
                        cols = [pnames.index(k) for k in triple]
                        rgb = np.array([[int(r[c]) for c in cols] for r in rows], dtype=np.uint8).reshape(count, 3)
                    if ntriple is not None:
                        cols = [pnames.index(k) for k in ntriple]
                        nrm = np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).astype(np.float32).reshape(count, 3)
                elif name == face_name:
                    bad = next((r for r, row in enumerate(rows) if len(row[idx]) != 3), None)
                    if bad is not None:
                        raise FormatError(f"{path}: face {bad} has {len(rows[bad][idx])} vertices (only triangles are supported)")
                    faces = np.array([[int(v) for v in row[idx]] for row in rows], dtype=np.int64).reshape(count, 3)
        else:
            end = "<" if fmt == "binary_little_endian" else ">"
            done = 0
            for name, count, props in elements:
                if name == "vertex":
                    dt = np.dtype([(p, np.dtype(t).newbyteorder(end)) for p, t in props])
                    buf = f.read(dt.itemsize * count)
                    if len(buf) != dt.itemsize * count:
                        raise FormatError(f"{path}: truncated vertex data")
                    rec = np.frombuffer(buf, dtype=dt)
                    verts = np.stack([rec[k].astype(np.float32) for k in ("x", "y", "z")], axis=1).reshape(count, 3)
                    if triple is not None:
                        rgb = np.stack([rec[k] for k in triple], axis=1).astype(np.uint8).reshape(count, 3)
                    if ntriple is not None:
                        nrm = np.stack([rec[k].astype(np.float32) for k in ntriple], axis=1).reshape(count, 3)
                    done += 1
                elif name == face_name:
                    faces = _binary_faces(f, count, props, idx, end, path)
                    done += 1
                else:
                    _skip_binary_element(f, count, props, end)
                if done == (1 if face_name is None else 2):
                    break
    if not np.isfinite(verts).all():
        raise FormatError(f"{path}: non-finite vertex coordinates")
    n = len(verts)
    if len(faces) and (faces.min() < 0 or faces.max() >= n):
        raise FormatError(f"{path}: face indices outside 0 .. {n - 1}")
    if normals:
        return verts, faces.astype(np.int32).reshape(-1, 3), rgb, nrm
    return verts, faces.astype(np.int32).reshape(-1, 3), rgb


# ---- MAT v5 --------------------------------------------------------------------------------------------------------------
_MI = {1: "i1", 2: "u1", 3: "i2", 4: "u2", 5: "i4", 6: "u4", 7: "f4", 9: "f8", 12: "i8", 13: "u8"}
_MX = {6: "f8", 7: "f4", 8: "i1", 9: "u1", 10: "i2", 11: "u2", 12: "i4", 13: "u4", 14: "i8", 15: "u8"}
MI_MATRIX, MI_COMPRESSED = 14, 15


def _elements(buf, end):
    """Yield (type, payload bytes) of the data elements of buf."""
    pos = 0
    while pos + 8 <= len(buf):
        first, second = struct.unpack(end + "II", buf[pos:pos + 8])
        if first >> 16:                                        # small data element: 2-byte size, 2-byte type, 4 bytes of data
            n, typ = first >> 16, first & 0xFFFF
            yield typ, buf[pos + 4:pos + 4 + n]
            pos += 8
            continue
        typ, n = first, second
        payload = buf[pos + 8:pos + 8 + n]
        if len(payload) != n:
            raise FormatError("truncated MAT data element")
        yield typ, payload
        pos += 8 + n
        if typ != MI_COMPRESSED:
            pos += (-n) % 8


def _numeric(typ, payload, end):
    if typ not in _MI:
        raise FormatError(f"MAT data type {typ}")
    return np.frombuffer(payload, dtype=np.dtype(_MI[typ]).newbyteorder(end))


def _matrix(payload, end):
    """-> (name, array) of a miMATRIX element, or (name, None) for a class this reader skips."""
    sub = list(_elements(payload, end))
    if len(sub) < 3:
        raise FormatError("malformed MAT matrix")
    flags = _numeric(*sub[0], end)
    cls, logical, cplx = int(flags[0]) & 0xFF, bool(int(flags[0]) & 0x200), bool(int(flags[0]) & 0x800)
    dims = [int(d) for d in _numeric(*sub[1], end)]
    name = bytes(sub[2][1]).decode("ascii", "replace")
    if cls not in _MX or cplx:
        return name, None
    real = _numeric(*sub[3], end) if len(sub) > 3 else np.zeros(0)
    if real.size != int(np.prod(dims)):
        raise FormatError(f"MAT variable {name}: {real.size} values for dims {dims}")
    a = real.astype(np.dtype(_MX[cls]).newbyteorder("=")).reshape(dims, order="F")
    return name, (a != 0) if logical else a


def read_mat(path):
    """-> {name: ndarray} of the full numeric / logical variables of a level-5 MAT file."""
    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 128:
        raise FormatError(f"{path}: not a MAT file")
    if buf[512:516] == b"\x89HDF" or b"MATLAB 7.3" in buf[:116]:
        raise FormatError(f"{path}: MAT v7.3 (HDF5) files are not supported; save with -v7 (or -v6) instead")
    end = {b"IM": "<", b"MI": ">"}.get(buf[126:128])
    if end is None or not buf[:6] == b"MATLAB":
        raise FormatError(f"{path}: not a level-5 MAT file")
    out = {}

    def visit(data):
        for typ, payload in _elements(data, end):
            if typ == MI_COMPRESSED:
                visit(zlib.decompress(payload))
            elif typ == MI_MATRIX:
                name, a = _matrix(payload, end)
                if a is not None:
                    out[name] = a

    visit(buf[128:])
    return out
