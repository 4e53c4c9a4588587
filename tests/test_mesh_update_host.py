"""Vertex updates, the part that needs no GPU: the entry points exist and check their context, and the bounds statement the host shares
with the device refit (csrc/zr_bounds.h) never lets a non-finite vertex shrink a meshlet's bounds."""
import numpy as np

from zeldaengine_amd import abi, engine, scenes


def test_entry_points_refuse_a_null_context():
    L = engine.lib()
    n = engine.C.c_uint32()
    assert L.zr_mesh_set_vertices(None, 0, 0, None, 0) == abi.ERR_ARG
    assert L.zr_mesh_update_vertices_async(None, 0, 0, None, 0, None) == abi.ERR_ARG
    assert L.zr_mesh_get_vertices(None, 0, None, engine.C.byref(n)) == abi.ERR_ARG


def test_a_non_finite_vertex_gives_bounds_no_cull_can_use():
    """Radius +inf, cutoff 1.0 for every meshlet that holds the vertex; the others keep finite, enclosing spheres."""
    v, idx = scenes.uv_sphere()
    bad = v.copy()
    bad["Position"][17, 1] = np.float32("nan")
    bad["Position"][300, 0] = np.float32("inf")
    ml, mv, mt, _ = engine.build_meshlets(bad, idx)
    hit = np.array([bool(np.isin([17, 300], mv[m["VertexOffset"]:m["VertexOffset"] + m["VertexCount"]]).any()) for m in ml])
    assert hit.any() and not hit.all()
    assert np.isposinf(ml["BoundsRadius"][hit]).all() and (ml["ConeCutoff"][hit] == 1.0).all()
    assert np.isfinite(ml["BoundsCenter"][hit]).all() and np.isfinite(ml["ConeAxis"][hit]).all()
    pos = bad["Position"].astype(np.float64)
    for m in ml[~hit]:
        vi = mv[m["VertexOffset"]:m["VertexOffset"] + m["VertexCount"]]
        d = np.linalg.norm(pos[vi] - m["BoundsCenter"].astype(np.float64), axis=1)
        assert np.isfinite(m["BoundsRadius"]) and (d <= float(m["BoundsRadius"])).all()
        assert 0.0 < m["ConeCutoff"] <= 1.0
