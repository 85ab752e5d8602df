"""Intersection pair lists, the part that needs no GPU: the four entry points are declared, exported and bound, reject
NULL handles before any device work, and the Python functions validate their arguments like
``aabbtree_intersections_indices`` does."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meshsearch.h")
SYMBOLS = ["msh_tree_intersection_pairs", "msh_tree_intersection_pairs_device", "msh_tree_self_intersection_pairs",
           "msh_tree_self_intersection_pairs_device"]


def test_symbols_declared_exported_and_bound():
    from mesh_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = ctypes.CDLL(_native.LIB_PATH)
    table = dict((n, (res, args)) for n, res, args in _native.SIGNATURES)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, txt), s
        assert hasattr(L, s), s
        assert s in table and table[s][0] is ctypes.c_int, s
    # argument counts of the table and the header agree
    for s in SYMBOLS:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S).group(1)
        assert len(decl.split(",")) == len(table[s][1]), s


def test_null_handles_rejected():
    from mesh_amd import _native
    L = _native.lib()
    K = ctypes.c_size_t(7)
    qv = np.zeros((3, 3))
    qf = np.array([[0, 1, 2]], np.uint32)
    pairs = np.zeros((4, 2), np.uint32)
    calls = [
        lambda: L.msh_tree_intersection_pairs(None, _native.dptr(qv), 3, _native.uptr(qf), 1, _native.uptr(pairs), 4,
                                              None, ctypes.byref(K)),
        lambda: L.msh_tree_intersection_pairs_device(None, None, 3, None, 1, None, 0, None, ctypes.byref(K), None),
        lambda: L.msh_tree_self_intersection_pairs(None, _native.uptr(pairs), 4, None, ctypes.byref(K)),
        lambda: L.msh_tree_self_intersection_pairs_device(None, None, 0, None, ctypes.byref(K), None),
    ]
    for name, call in zip(SYMBOLS, calls):
        assert call() == _native.MSH_EINVAL, name
        msg = L.msh_last_error()
        assert b"null" in msg and name.encode() in msg, (name, msg)


def test_python_validation_mirrors_intersections_indices():
    from mesh_amd import _native, aabb_normals, spatialsearch
    fake = _native.Handle(1, "triangles")
    fake_n = _native.Handle(1, "normals")
    fake_p = _native.Handle(1, "points")
    fake_b = _native.Handle(1, "batch")
    f = np.zeros((1, 3), np.uint32)
    try:
        with pytest.raises(TypeError, match=r"aabbtree_intersections_pairs\(\) arguments must be numpy.ndarray"):
            spatialsearch.aabbtree_intersections_pairs(fake, [[0.0, 0.0, 0.0]], f)
        with pytest.raises(TypeError, match="must be numpy.ndarray"):
            spatialsearch.aabbtree_intersections_pairs(fake, np.zeros((3, 3)), [[0, 1, 2]])
        with pytest.raises(ValueError, match="Query Vertices must be of type double, and 2 dimensional"):
            spatialsearch.aabbtree_intersections_pairs(fake, np.zeros((3, 3), np.float32), f)
        with pytest.raises(ValueError, match="Query Vertices must be of type double, and 2 dimensional"):
            spatialsearch.aabbtree_intersections_pairs(fake, np.zeros(9), f)
        with pytest.raises(ValueError, match="Query Faces must be of type uint32, and 2 dimensional"):
            spatialsearch.aabbtree_intersections_pairs(fake, np.zeros((3, 3)), np.zeros((1, 3), np.int32))
        with pytest.raises(ValueError, match="Query Faces must be of type uint32, and 2 dimensional"):
            spatialsearch.aabbtree_intersections_pairs(fake, np.zeros((3, 3)), np.zeros(3, np.uint32))
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.aabbtree_intersections_pairs(fake, np.zeros((3, 2)), f)
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.aabbtree_intersections_pairs(fake, np.zeros((3, 3)), np.zeros((1, 4), np.uint32))
        # handles: not a handle at all, a freed one, and the wrong kinds -- all before any native call
        for fn in (spatialsearch.aabbtree_selfintersections_pairs, aabb_normals.aabbtree_n_selfintersections_pairs,
                   lambda h: spatialsearch.aabbtree_intersections_pairs(h, np.zeros((3, 3)), f)):
            with pytest.raises(TypeError):
                fn(object())
            with pytest.raises(TypeError):
                fn(_native.Handle(None, "triangles"))
            with pytest.raises(ValueError):
                fn(fake_p)
            with pytest.raises(ValueError):
                fn(fake_b)
        with pytest.raises(ValueError):
            spatialsearch.aabbtree_selfintersections_pairs(fake_n)
        with pytest.raises(ValueError):
            aabb_normals.aabbtree_n_selfintersections_pairs(fake)
    finally:
        for h in (fake, fake_n, fake_p, fake_b):
            h.ptr = None


def test_methods_exist():
    from mesh_amd.mesh import Mesh
    from mesh_amd.search import AabbNormalsTree, AabbTree
    assert callable(AabbTree.intersections_pairs) and callable(AabbTree.selfintersections_pairs)
    assert callable(AabbNormalsTree.selfintersections_pairs)
    assert callable(Mesh.self_intersection_pairs)
