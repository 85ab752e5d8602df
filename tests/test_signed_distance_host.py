"""Signed distance: the checks that need no GPU -- the Python shims validate their arguments before any device
work, and every new C entry point rejects a NULL handle with MSH_EINVAL and a message.  (The header / ctypes table
agreement of the new exports is covered by tests/test_abi.py.)"""
import ctypes

import numpy as np
import pytest


def test_python_validation_before_device_work():
    from mesh_amd import _native, spatialsearch
    fake = _native.Handle(1, "triangles")  # never dereferenced: validation must raise first
    fake_n = _native.Handle(1, "normals")
    fake_p = _native.Handle(1, "points")
    try:
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.aabbtree_signed_distance(fake, np.zeros((4, 2)))
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.aabbtree_signed_distance(fake, np.zeros(3))
        with pytest.raises(TypeError, match=r"aabbtree_signed_distance\(\) argument 2 must be numpy.ndarray"):
            spatialsearch.aabbtree_signed_distance(fake, [[0.0, 0.0, 0.0]])
        with pytest.raises(TypeError, match="not a triangle tree"):
            spatialsearch.aabbtree_signed_distance(fake_n, np.zeros((4, 3)))
        with pytest.raises(TypeError, match="point tree"):
            spatialsearch.aabbtree_signed_distance(fake_p, np.zeros((4, 3)))
        with pytest.raises(TypeError, match="expected a tree handle"):
            spatialsearch.aabbtree_signed_distance(None, np.zeros((4, 3)))
        # sign_build without faces (a blob-unpacked handle keeps none) and with faces of the wrong shape
        assert fake.faces is None
        with pytest.raises(ValueError, match=r"sign_build\(f\)"):
            fake.sign_build()
        with pytest.raises(ValueError, match="Faces must be Tx3"):
            fake.sign_build(np.zeros((4, 2), np.uint32))
    finally:
        fake.ptr = fake_n.ptr = fake_p.ptr = None


def test_handle_keeps_a_private_face_copy():
    from mesh_amd import _native
    h = _native.Handle(None, "triangles", np.arange(6, dtype=np.uint32).reshape(2, 3))
    assert h.faces.shape == (2, 3) and h.faces.dtype == np.uint32
    assert _native.Handle(None, "triangles").faces is None


def test_null_handles_rejected():
    from mesh_amd import _native
    L = _native.lib()
    q, pt, sd = np.zeros(3), np.zeros(3), np.zeros(1)
    face, part = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    f = np.array([[0, 1, 2]], np.uint32)
    info = _native.SignInfo()
    calls = {
        "msh_tree_sign_build": lambda: L.msh_tree_sign_build(None, _native.uptr(f), 1),
        "msh_tree_sign_info": lambda: L.msh_tree_sign_info(None, ctypes.byref(info)),
        "msh_tree_signed_distance": lambda: L.msh_tree_signed_distance(
            None, _native.dptr(q), 1, _native.dptr(sd), _native.uptr(face), _native.uptr(part), _native.dptr(pt)),
        "msh_tree_signed_distance_device": lambda: L.msh_tree_signed_distance_device(
            None, None, 1, None, None, None, None, None),
        "msh_tree_sign_from_faces_device": lambda: L.msh_tree_sign_from_faces_device(
            None, None, 1, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == _native.MSH_EINVAL, name
        msg = L.msh_last_error()
        assert b"null" in msg and name.encode() in msg, (name, msg)


def test_sign_info_struct_matches_header():
    # msh_sign_info: int32 state (padded to 8), five u64 counters / sizes, one double
    from mesh_amd import _native
    assert ctypes.sizeof(_native.SignInfo) == 56
    assert [n for n, _ in _native.SignInfo._fields_] == ["state", "boundary_edges", "nonmanifold_edges",
                                                         "inconsistent_edges", "degenerate_faces", "bytes", "build_ms"]
