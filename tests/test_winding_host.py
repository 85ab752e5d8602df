"""Generalised winding numbers: the checks that need no GPU -- every new C entry point rejects a NULL handle and a bad
beta with MSH_EINVAL and a message, and the Python layers validate their arguments before any device work.  (The
header / ctypes table agreement of the new exports is covered by tests/test_abi.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handles_rejected():
    from mesh_amd import _native
    L = _native.lib()
    q, w = np.zeros(3), np.zeros(1)
    info = _native.WindingInfo()
    counts = (ctypes.c_uint64 * 4)()
    calls = {
        "msh_tree_winding_build": lambda: L.msh_tree_winding_build(None),
        "msh_tree_winding_info": lambda: L.msh_tree_winding_info(None, ctypes.byref(info)),
        "msh_tree_winding_number": lambda: L.msh_tree_winding_number(None, _native.dptr(q), 1, 2.0, _native.dptr(w)),
        "msh_tree_winding_number_device": lambda: L.msh_tree_winding_number_device(None, None, 1, 2.0, None, None),
        "msh_tree_winding_stats": lambda: L.msh_tree_winding_stats(None, None, 1, 2.0, counts),
    }
    for name, call in calls.items():
        assert call() == _native.MSH_EINVAL, name
        msg = L.msh_last_error()
        assert msg and b"null" in msg and name.encode() in msg, (name, msg)


def test_bad_beta_rejected():
    # beta is checked before the handle is looked at, so no device (and no real tree) is needed to see the refusal
    from mesh_amd import _native
    L = _native.lib()
    q, w = np.zeros(3), np.zeros(1)
    counts = (ctypes.c_uint64 * 4)()
    for beta in (-1.0, float("nan"), float("-inf")):
        for name, call in (
                ("msh_tree_winding_number",
                 lambda: L.msh_tree_winding_number(None, _native.dptr(q), 1, beta, _native.dptr(w))),
                ("msh_tree_winding_number_device",
                 lambda: L.msh_tree_winding_number_device(None, None, 1, beta, None, None)),
                ("msh_tree_winding_stats", lambda: L.msh_tree_winding_stats(None, None, 1, beta, counts))):
            assert call() == _native.MSH_EINVAL, (name, beta)
            msg = L.msh_last_error()
            assert b"beta" in msg and name.encode() in msg, (name, beta, msg)


def test_python_validation_before_device_work():
    from mesh_amd import _native, spatialsearch
    fake = _native.Handle(1, "triangles")  # never dereferenced: validation must raise first
    fake_n = _native.Handle(1, "normals")
    fake_p = _native.Handle(1, "points")
    try:
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.aabbtree_winding_number(fake, np.zeros((4, 2)))
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.aabbtree_winding_number(fake, np.zeros(3))
        with pytest.raises(TypeError, match=r"aabbtree_winding_number\(\) argument 2 must be numpy.ndarray"):
            spatialsearch.aabbtree_winding_number(fake, [[0.0, 0.0, 0.0]])
        with pytest.raises(TypeError, match="not a triangle tree"):
            spatialsearch.aabbtree_winding_number(fake_n, np.zeros((4, 3)))
        with pytest.raises(TypeError, match="point tree"):
            spatialsearch.aabbtree_winding_number(fake_p, np.zeros((4, 3)))
        with pytest.raises(TypeError, match="expected a tree handle"):
            spatialsearch.aabbtree_winding_number(None, np.zeros((4, 3)))
    finally:
        fake.ptr = fake_n.ptr = fake_p.ptr = None


def test_unknown_sign_and_method_raise():
    from mesh_amd import _native, search
    from mesh_amd.mesh import Mesh
    tree = search.AabbTree.__new__(search.AabbTree)  # no build: the argument check comes first
    tree.cpp_handle = _native.Handle(None, "triangles")
    q = np.zeros((4, 3))
    with pytest.raises(ValueError, match="method"):
        tree.contains(q, method="bogus")
    with pytest.raises(ValueError, match="sign"):
        tree.signed_distance(q, sign="bogus")
    with pytest.raises(ValueError, match="method"):
        Mesh(v=np.zeros((3, 3)), f=np.array([[0, 1, 2]], np.uint32)).contains(q, method="bogus")


def test_winding_info_struct_and_default_beta_match_header():
    # msh_winding_info: int32 state, two u32, one u64, one double
    from mesh_amd import _native
    assert ctypes.sizeof(_native.WindingInfo) == 32
    assert [n for n, _ in _native.WindingInfo._fields_] == ["state", "node_bytes", "stack_lds", "bytes", "build_ms"]
    txt = open(os.path.join(ROOT, "include", "meshsearch.h")).read()
    m = re.search(r"^#define MSH_WINDING_BETA_DEFAULT\s+(\S+)", txt, flags=re.M)
    assert m and float(m.group(1)) == _native.WINDING_BETA_DEFAULT
    assert _native.WINDING_BETA_DEFAULT in (2.0, 3.0, 4.0, 6.0, 8.0)
