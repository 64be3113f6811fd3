"""ASCII VTK unstructured grids (.vtu) of a tetrahedral mesh with cell and point data, written by hand, and a reader of exactly what the writer writes
(so that a test can round-trip a file; it is no general VTK reader).

Arrays: a 1-D array is a scalar field, an [n, k] array a field of k components.  A symmetric tensor goes in as six components in VTK's order XX YY ZZ XY YZ
XZ -- the order of the stress record of `Context.elastic_stress`.  Numbers are written with `repr`, so every double comes back bit for bit (NaN as `nan`).
"""
from __future__ import annotations

import re

import numpy as np

VTK_TETRA = 10


def _fmt(a):
    a = np.asarray(a)
    if a.shape[0] == 0:
        return []
    if a.dtype.kind in "iu":
        return [" ".join(str(int(v)) for v in row) for row in a.reshape(a.shape[0], -1)]
    return [" ".join(repr(float(v)) for v in row) for row in a.reshape(a.shape[0], -1)]


def _data_array(name, a, n):
    a = np.asarray(a)
    if a.shape[0] != n or a.ndim > 2:
        raise ValueError(f"field {name!r}: expected {n} rows, got an array of shape {a.shape}")
    kind = "Int32" if a.dtype.kind in "iu" else "Float64"
    ncomp = 1 if a.ndim == 1 else a.shape[1]
    return [f'<DataArray type="{kind}" Name="{name}" NumberOfComponents="{ncomp}" format="ascii">'] + _fmt(a) + ["</DataArray>"]


def write_vtu(path, points, tets, cell_data=None, point_data=None):
    """points [nV, 3], tets [nT, 4]; cell_data / point_data: {name: array with nT / nV rows}, written in the order given"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    nV, nT = points.shape[0], tets.shape[0]
    if nT and (tets.min() < 0 or tets.max() >= nV):
        raise ValueError("element refers to a node that does not exist")
    L = ['<?xml version="1.0"?>', '<VTKFile type="UnstructuredGrid" version="0.1" byte_order="LittleEndian">', "<UnstructuredGrid>",
         f'<Piece NumberOfPoints="{nV}" NumberOfCells="{nT}">', "<Points>"]
    L += _data_array("Points", points, nV) + ["</Points>", "<Cells>"]
    L += _data_array("connectivity", tets.astype(np.int32), nT)
    L += _data_array("offsets", (4 * np.arange(1, nT + 1)).astype(np.int32), nT)
    L += _data_array("types", np.full(nT, VTK_TETRA, dtype=np.int32), nT) + ["</Cells>"]
    for tag, data, n in (("CellData", cell_data, nT), ("PointData", point_data, nV)):
        L.append(f"<{tag}>")
        for name, a in (data or {}).items():
            L += _data_array(name, a, n)
        L.append(f"</{tag}>")
    L += ["</Piece>", "</UnstructuredGrid>", "</VTKFile>"]
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


_ARRAY = re.compile(r'<DataArray type="(\w+)" Name="([^"]+)" NumberOfComponents="(\d+)" format="ascii">\n(.*?)</DataArray>', re.S)


def _arrays(block):
    out = {}
    for kind, name, ncomp, body in _ARRAY.findall(block):
        vals = body.split()
        a = np.array([int(v) for v in vals], dtype=np.int32) if kind == "Int32" else np.array([float(v) for v in vals], dtype=np.float64)
        out[name] = a if int(ncomp) == 1 else a.reshape(-1, int(ncomp))
    return out


def read_vtu(path):
    """a file of write_vtu: dict(points, tets, cell_data, point_data), the data dictionaries in file order"""
    txt = open(path).read()
    m = re.search(r'<Piece NumberOfPoints="(\d+)" NumberOfCells="(\d+)">', txt)
    if not m:
        raise ValueError(f"{path}: not a file of write_vtu")
    nV, nT = int(m.group(1)), int(m.group(2))

    def block(tag):
        b = re.search(rf"<{tag}>\n(.*?)</{tag}>", txt, re.S)
        return b.group(1) if b else ""
    points = _arrays(block("Points"))["Points"].reshape(-1, 3)
    cells = _arrays(block("Cells"))
    tets = cells["connectivity"].reshape(-1, 4)
    if points.shape[0] != nV or tets.shape[0] != nT or not np.array_equal(cells["offsets"].ravel(), 4 * np.arange(1, nT + 1)) or np.any(cells["types"] != VTK_TETRA):
        raise ValueError(f"{path}: counts, offsets or cell types do not describe {nT} tetrahedra on {nV} points")
    return dict(points=points, tets=tets, cell_data=_arrays(block("CellData")), point_data=_arrays(block("PointData")))
