"""pytorch3d.io.load_ply / save_ply (datasets/goliath_dataset.py:28,268,303,323,385) on the host with numpy: ascii and binary
little-endian files with vertex `x y z` and triangular `vertex_indices` / `vertex_index` faces.  `f` is a path or a binary
file object (the reference reads `BytesIO(zip member)`)."""
import os

import numpy as np
import torch

__all__ = ["load_ply", "save_ply"]

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
          "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _read_all(f):
    if isinstance(f, (str, os.PathLike)):
        with open(f, "rb") as fh:
            return fh.read()
    raw = f.read()
    return raw.encode("ascii") if isinstance(raw, str) else bytes(raw)


def _header(raw):
    if not raw.startswith(b"ply"):
        raise ValueError("load_ply: not a PLY file")
    end = raw.find(b"end_header")
    if end < 0:
        raise ValueError("load_ply: the header has no end_header")
    stop = raw.index(b"\n", end) + 1
    fmt, elements = None, []                                   # elements: [name, count, [(kind, name, types...)]]
    for line in raw[:end].decode("ascii").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elements:
                raise ValueError("load_ply: a property before any element")
            if tok[1] == "list":
                elements[-1][2].append(("list", tok[4], tok[2], tok[3]))
            else:
                elements[-1][2].append(("scalar", tok[2], tok[1]))
        else:
            raise ValueError(f"load_ply: header line {line!r}")
    for _, _, props in elements:
        for p in props:
            for t in p[2:]:
                if t not in _TYPES:
                    raise ValueError(f"load_ply: property type {t!r}")
    return fmt, elements, stop


def load_ply(f, *, path_manager=None):
    """-> (verts float32 (V,3), faces int64 (F,3)) as CPU tensors; faces is (0,3) when the file has no face element."""
    if path_manager is not None:
        raise NotImplementedError("load_ply: path_manager is not built")
    raw = _read_all(f)
    fmt, elements, pos = _header(raw)
    if fmt not in ("ascii", "binary_little_endian"):
        raise NotImplementedError(f"load_ply: format {fmt!r}; ascii and binary_little_endian are built")
    verts, faces = None, np.zeros((0, 3), np.int64)
    tokens, t = (raw[pos:].split(), 0) if fmt == "ascii" else (None, 0)
    for name, count, props in elements:
        lists = [p for p in props if p[0] == "list"]
        if name == "vertex":
            if lists:
                raise NotImplementedError("load_ply: a list property in the vertex element")
            names = [p[1] for p in props]
            if not all(c in names for c in "xyz"):
                raise ValueError("load_ply: the vertex element has no x, y, z")
            if fmt == "ascii":
                table = np.array(tokens[t:t + count * len(props)], dtype=np.float64).reshape(count, len(props))
                t += count * len(props)
                verts = np.stack([table[:, names.index(c)] for c in "xyz"], axis=1).astype(np.float32)
            else:
                dt = np.dtype([(p[1], "<" + _TYPES[p[2]]) for p in props])
                table = np.frombuffer(raw, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
                verts = np.stack([table[c] for c in "xyz"], axis=1).astype(np.float32)
        elif name == "face":
            if len(props) != 1 or not lists or props[0][1] not in ("vertex_indices", "vertex_index"):
                raise NotImplementedError("load_ply: the face element must hold exactly one list property, vertex_indices")
            if fmt == "ascii":
                table = np.array(tokens[t:t + 4 * count], dtype=np.int64).reshape(count, 4) if count else np.zeros((0, 4), np.int64)
                if count and not (table[:, 0] == 3).all():
                    raise NotImplementedError("load_ply: faces that are not triangles")
                t += 4 * count
                faces = table[:, 1:].astype(np.int64)
            else:
                dt = np.dtype([("n", "<" + _TYPES[props[0][2]]), ("v", "<" + _TYPES[props[0][3]], (3,))])
                if len(raw) - pos < count * dt.itemsize:
                    raise NotImplementedError("load_ply: faces that are not triangles (or a truncated file)")
                table = np.frombuffer(raw, dtype=dt, count=count, offset=pos)
                if count and not (table["n"] == 3).all():
                    raise NotImplementedError("load_ply: faces that are not triangles")
                pos += count * dt.itemsize
                faces = table["v"].astype(np.int64).reshape(count, 3)
        else:
            raise NotImplementedError(f"load_ply: element {name!r}; vertex and face are built")
    if verts is None:
        raise ValueError("load_ply: the file has no vertex element")
    return torch.from_numpy(np.ascontiguousarray(verts)), torch.from_numpy(np.ascontiguousarray(faces))


def save_ply(f, verts, faces=None, verts_normals=None, ascii=False, decimal_places=None, path_manager=None):
    """Writes verts (V,3) and, if given, triangular faces (F,3): binary little-endian float32 / int32, or ascii."""
    if verts_normals is not None:
        raise NotImplementedError("save_ply: verts_normals is not built")
    if path_manager is not None:
        raise NotImplementedError("save_ply: path_manager is not built")
    v = np.asarray(verts.detach().cpu().numpy() if torch.is_tensor(verts) else verts, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"save_ply: expected verts (V,3), got {v.shape}")
    tri = None
    if faces is not None:
        tri = np.asarray(faces.detach().cpu().numpy() if torch.is_tensor(faces) else faces)
        if tri.ndim != 2 or tri.shape[1] != 3:
            raise ValueError(f"save_ply: expected faces (F,3), got {tri.shape}")
        if tri.size and (tri.min() < 0 or tri.max() >= len(v)):
            raise ValueError("save_ply: faces name a vertex the file does not hold")
        tri = tri.astype("<i4")
    head = "ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % (
        "ascii" if ascii else "binary_little_endian", len(v))
    if tri is not None:
        head += "element face %d\nproperty list uchar int vertex_indices\n" % len(tri)
    head += "end_header\n"
    if ascii:
        fmt = "%r" if decimal_places is None else "%%.%df" % decimal_places
        body = "".join(" ".join(fmt % float(c) for c in row) + "\n" for row in v)
        if tri is not None:
            body += "".join("3 %d %d %d\n" % tuple(row) for row in tri)
        payload = body.encode("ascii")
    else:
        payload = np.ascontiguousarray(v, dtype="<f4").tobytes()
        if tri is not None:
            rec = np.empty(len(tri), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            rec["n"], rec["v"] = 3, tri
            payload += rec.tobytes()
    data = head.encode("ascii") + payload
    if isinstance(f, (str, os.PathLike)):
        with open(f, "wb") as fh:
            fh.write(data)
    else:
        f.write(data)
