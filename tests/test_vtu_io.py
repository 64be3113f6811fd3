"""Round trip of the hand-written ASCII .vtu writer (`ipc_amd/vtu_io.py`) through its own reader on a two-tet mesh: counts, component order, and every
value to `repr` precision (bit for bit).  No GPU."""
import numpy as np
import pytest

from ipc_amd import vtu_io


def two_tets():
    V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0 / 3.0, 2.0 / 3.0, -0.1]])
    T = np.array([[0, 1, 2, 3], [0, 2, 1, 4]], dtype=np.int32)
    return V, T


def test_round_trip_counts_order_and_bits(tmp_path):
    V, T = two_tets()
    rng = np.random.default_rng(5)
    stress = rng.standard_normal((2, 6)) * 10.0 ** rng.integers(-300, 300, (2, 6))
    stress[0] = [11.0, 22.0, 33.0, 12.0, 23.0, 13.0]  # XX YY ZZ XY YZ XZ: the place of a component is its meaning
    stress[1, 2] = np.nextafter(1.0, 2.0)
    cell = {"stress": stress, "von_mises": np.array([0.1, np.nan]), "J": np.array([1.0, -0.0])}
    point = {"stress": rng.standard_normal((5, 6)), "von_mises": np.abs(rng.standard_normal(5)), "velocity": rng.standard_normal((5, 3)) * 1e-17,
             "contact_force": np.zeros((5, 3))}
    path = tmp_path / "fields7.vtu"
    vtu_io.write_vtu(path, V, T, cell, point)
    txt = open(path).read()
    assert txt.startswith('<?xml version="1.0"?>\n<VTKFile type="UnstructuredGrid"') and 'NumberOfPoints="5" NumberOfCells="2"' in txt
    assert '<DataArray type="Float64" Name="stress" NumberOfComponents="6" format="ascii">\n11.0 22.0 33.0 12.0 23.0 13.0\n' in txt
    R = vtu_io.read_vtu(path)
    assert R["points"].shape == (5, 3) and R["tets"].shape == (2, 4)
    assert R["points"].tobytes() == V.tobytes() and np.array_equal(R["tets"], T)
    assert list(R["cell_data"]) == ["stress", "von_mises", "J"] and list(R["point_data"]) == ["stress", "von_mises", "velocity", "contact_force"]
    for got, want in ((R["cell_data"], cell), (R["point_data"], point)):
        for k, a in want.items():
            assert got[k].shape == a.shape and got[k].dtype == np.float64
            assert got[k].tobytes() == a.tobytes(), k  # repr round-trips every double, the sign of zero and NaN included
    assert np.array_equal(R["cell_data"]["stress"][0], [11.0, 22.0, 33.0, 12.0, 23.0, 13.0])


def test_no_fields_and_bad_input(tmp_path):
    V, T = two_tets()
    vtu_io.write_vtu(tmp_path / "a.vtu", V, T)
    R = vtu_io.read_vtu(tmp_path / "a.vtu")
    assert R["cell_data"] == {} and R["point_data"] == {} and np.array_equal(R["tets"], T)
    with pytest.raises(ValueError):
        vtu_io.write_vtu(tmp_path / "b.vtu", V, T, {"J": np.zeros(3)})  # one value per cell
    with pytest.raises(ValueError):
        vtu_io.write_vtu(tmp_path / "b.vtu", V[:4], T)  # node 4 does not exist
    (tmp_path / "c.vtu").write_text("<VTKFile/>\n")
    with pytest.raises(ValueError):
        vtu_io.read_vtu(tmp_path / "c.vtu")
