"""Ray casting (msh_tree_raycast, msh_tree_occluded): the checks that need no GPU -- every new C entry point refuses a
NULL handle with MSH_EINVAL and a message naming it, the Python layers validate their arguments before any device work
(on fake handles that are never dereferenced), and the host property test of the first-hit key and the ranged node test
(tests/csrc/raycast_bound_check.cpp on the kernels' own header).  (The header / ctypes table agreement of the new
exports is covered by tests/test_abi.py.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _calls(L, N, handle):
    o, d, rng = np.zeros(3), np.ones(3), np.array([0.0, 1.0])
    t, face, pt, w = np.zeros(1), np.zeros(1, np.uint32), np.zeros(3), np.zeros(3)
    hit = np.zeros(1, np.uint8)
    hp = hit.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    nodes, leaves = ctypes.c_uint64(0), ctypes.c_uint64(0)
    return {
        "msh_tree_raycast": lambda: L.msh_tree_raycast(handle, N.dptr(o), N.dptr(d), N.dptr(rng), 1, N.dptr(t),
                                                       N.uptr(face), N.dptr(pt), N.dptr(w)),
        "msh_tree_raycast_device": lambda: L.msh_tree_raycast_device(handle, None, None, None, 1, None, None, None, None,
                                                                     None),
        "msh_tree_occluded": lambda: L.msh_tree_occluded(handle, N.dptr(o), N.dptr(d), None, 1, hp),
        "msh_tree_occluded_device": lambda: L.msh_tree_occluded_device(handle, None, None, None, 1, None, None),
        "msh_tree_raycast_stats": lambda: L.msh_tree_raycast_stats(handle, None, None, None, 1, 0, ctypes.byref(nodes),
                                                                   ctypes.byref(leaves)),
    }


def test_null_handles_rejected():
    from mesh_amd import _native as N
    L = N.lib()
    calls = _calls(L, N, None)
    assert len(calls) == 5
    for name, call in calls.items():
        assert call() == N.MSH_EINVAL, name
        msg = L.msh_last_error()
        assert msg and b"null" in msg and name.encode() in msg, (name, msg)


def test_python_validation_before_device_work():
    from mesh_amd import _native as N, search, spatialsearch
    fake = N.Handle(1, "triangles")  # never dereferenced: validation must raise first
    fake_n = N.Handle(1, "normals")
    fake_p = N.Handle(1, "points")
    o, d = np.zeros((4, 3)), np.ones((4, 3))
    try:
        for fn in (spatialsearch.aabbtree_raycast, spatialsearch.aabbtree_occluded):
            with pytest.raises(ValueError, match="Origins and directions must be Nx3"):
                fn(fake, np.zeros((4, 2)), d)
            with pytest.raises(ValueError, match="Origins and directions must be Nx3"):
                fn(fake, o, np.ones((5, 3)))
            with pytest.raises(ValueError, match="Origins and directions must be Nx3"):
                fn(fake, np.zeros(3), np.ones(3))
            with pytest.raises(TypeError, match="must be numpy.ndarray"):
                fn(fake, [[0.0, 0.0, 0.0]], np.ones((1, 3)))
            with pytest.raises(TypeError, match="must be numpy.ndarray"):
                fn(fake, o, None)
            with pytest.raises(TypeError, match="not a triangle tree"):
                fn(fake_n, o, d)
            with pytest.raises(TypeError, match="point tree"):
                fn(fake_p, o, d)
            with pytest.raises(TypeError, match="expected a tree handle"):
                fn(None, o, d)
            # t_range: None, a pair of scalars, an (S, 2) array -- anything else is refused
            for bad in ((0.0,), (0.0, 1.0, 2.0), np.zeros((3, 2)), np.zeros((4, 3)), np.zeros((2, 4)), 1.0):
                with pytest.raises(ValueError, match="t_range must be"):
                    fn(fake, o, d, bad)
            # a scalar pair no ray can have is the caller's mistake (array rows are answered as misses instead)
            for bad in ((2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan")), (float("inf"), 0.0)):
                with pytest.raises(ValueError, match="t0 <= t1"):
                    fn(fake, o, d, bad)
        # the three accepted forms reach the argument builder with the range every row gets
        _, oo, dd, r = spatialsearch._ray_args(fake, o, d, None, "aabbtree_raycast")
        assert r is None and oo.dtype == np.float64 and dd.flags.c_contiguous
        r = spatialsearch._ray_args(fake, o, d, (0.25, np.inf), "aabbtree_raycast")[3]
        assert r.shape == (4, 2) and r.dtype == np.float64 and (r == [0.25, np.inf]).all()
        r = spatialsearch._ray_args(fake, o, d, [-1, 2], "aabbtree_raycast")[3]
        assert (r == [-1.0, 2.0]).all()
        rows = np.array([[0.0, 1.0], [2.0, 1.0], [np.nan, 1.0], [0.5, 0.5]])
        r = spatialsearch._ray_args(fake, o, d, rows, "aabbtree_raycast")[3]
        assert r.shape == (4, 2) and r.flags.c_contiguous and np.array_equal(r, rows, equal_nan=True)
        r = spatialsearch._ray_args(fake, o[:2], d[:2], np.array([[0.0, 1.0], [3.0, 4.0]]), "aabbtree_occluded")[3]
        assert np.array_equal(r, [[0.0, 1.0], [3.0, 4.0]])  # S = 2: a (2, 2) array is per row
        # the classes over them: the same refusals, still with no device work
        tree = search.AabbTree.__new__(search.AabbTree)
        tree.cpp_handle = fake
        with pytest.raises(ValueError, match="Origins and directions must be Nx3"):
            tree.ray_cast(np.zeros((4, 2)), d)
        with pytest.raises(ValueError, match="Origins and directions must be Nx3"):
            tree.occluded(o, np.ones((3, 3)))
        with pytest.raises(ValueError, match="t0 <= t1"):
            tree.ray_cast(o, d, (1.0, 0.0))
        with pytest.raises(ValueError, match="a and b must both be Nx3"):
            tree.line_of_sight(np.zeros((4, 3)), np.zeros((5, 3)))
        with pytest.raises(ValueError, match="a and b must both be Nx3"):
            tree.line_of_sight(np.zeros(3), np.zeros(3))
        with pytest.raises(ValueError, match="a and b must both be Nx3"):
            tree.line_of_sight(np.zeros((4, 2)), np.zeros((4, 2)))
        for m in (-0.1, 0.6, float("nan")):
            with pytest.raises(ValueError, match="margin must be"):
                tree.line_of_sight(o, d, margin=m)
    finally:
        fake.ptr = fake_n.ptr = fake_p.ptr = None


def test_mesh_methods_exist():
    from mesh_amd.mesh import Mesh
    assert callable(Mesh.ray_cast) and callable(Mesh.line_of_sight)


@pytest.mark.parametrize("mutation", [None, "MUTATE_RAYCAST_KEY"])
def test_first_hit_key_is_a_lower_bound(tmp_path, mutation):
    """The ray-casting node test (common.h make_rayf_range, ray_child_first_key, ray_child_slabs) on 300k random and
    adversarial nodes and rays at every scale and offset: a ray through a point x = o + t* d of a child takes that
    child whenever t* lies in the row's range -- t* exactly at t0 and at t1 included -- and the child's first-hit key is
    <= t* |d|.  A host build of the kernels' own header.  The mutated build (the key taken from the far end of the
    child's interval) must find violations, which shows that the cases reach the key."""
    exe = str(tmp_path / "raycast_bound_check")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
           os.path.join(ROOT, "tests", "csrc", "raycast_bound_check.cpp"), "-I", os.path.join(ROOT, "mesh_amd", "csrc"),
           "-o", exe]
    if mutation:
        cmd.insert(1, "-D" + mutation)
    subprocess.check_call(cmd)
    out = subprocess.run([exe, "300000"], capture_output=True, text=True, timeout=300)
    line = [x for x in out.stdout.splitlines() if x.startswith("trials=")][-1]
    viol = int(line.split(" violations=")[1].split()[0])
    ends = int(out.stdout.split("at_range_end=")[1].split()[0])
    assert ends > 100000, out.stdout  # t* on an end of the range is exercised
    if mutation is None:
        assert out.returncode == 0 and viol == 0, out.stdout + out.stderr
    else:
        assert out.returncode == 1 and viol > 0, line
