"""All-hits ray casting (msh_tree_raycast_count, msh_tree_raycast_all): the checks that need no GPU -- every new C entry
point refuses a NULL handle with MSH_EINVAL and a message naming it, the Python layers validate their arguments before
any device work (on fake handles that are never dereferenced; the refusals are _ray_args' own), the Mesh and AabbTree
methods exist, and the host property test of the lists' radix key (tests/csrc/raycast_all_key_check.cpp on the
kernels' own header).  (The header / ctypes table agreement of the new exports is covered by tests/test_abi.py.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handles_rejected():
    from mesh_amd import _native as N
    L = N.lib()
    o, d, rng = np.zeros(3), np.ones(3), np.array([0.0, 1.0])
    counts, t, face, pt = np.zeros(1, np.uint32), np.zeros(1), np.zeros(1, np.uint32), np.zeros(3)
    side = np.zeros(1, np.int8)
    sp = side.ctypes.data_as(ctypes.POINTER(ctypes.c_int8))
    K = N._sz(7)
    calls = {
        "msh_tree_raycast_count": lambda: L.msh_tree_raycast_count(None, N.dptr(o), N.dptr(d), N.dptr(rng), 1,
                                                                   N.uptr(counts)),
        "msh_tree_raycast_count_device": lambda: L.msh_tree_raycast_count_device(None, None, None, None, 1, None, None),
        "msh_tree_raycast_all": lambda: L.msh_tree_raycast_all(None, N.dptr(o), N.dptr(d), N.dptr(rng), 1, N.uptr(counts),
                                                               N.dptr(t), N.uptr(face), N.dptr(pt), sp, 1,
                                                               ctypes.byref(K)),
        "msh_tree_raycast_all_device": lambda: L.msh_tree_raycast_all_device(None, None, None, None, 1, None, None, None,
                                                                             None, None, 0, ctypes.byref(K), None),
    }
    for name, call in calls.items():
        assert call() == N.MSH_EINVAL, name
        msg = L.msh_last_error()
        assert msg and b"null" in msg and name.encode() in msg, (name, msg)
        assert name.encode() + b":" in msg  # the entry point itself, not a longer name that holds it


def test_python_validation_before_device_work():
    from mesh_amd import _native as N, search, spatialsearch
    fake = N.Handle(1, "triangles")  # never dereferenced: validation must raise first
    fake_n = N.Handle(1, "normals")
    fake_p = N.Handle(1, "points")
    o, d = np.zeros((4, 3)), np.ones((4, 3))
    try:
        for fn in (spatialsearch.aabbtree_raycast_count, spatialsearch.aabbtree_raycast_all):
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
            for bad in ((0.0,), (0.0, 1.0, 2.0), np.zeros((3, 2)), np.zeros((4, 3)), 1.0):
                with pytest.raises(ValueError, match="t_range must be"):
                    fn(fake, o, d, bad)
            for bad in ((2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan"))):
                with pytest.raises(ValueError, match="t0 <= t1"):
                    fn(fake, o, d, bad)
            with pytest.raises(ValueError, match=fn.__name__):  # the message names the function the caller used
                fn(fake, o, d, (2.0, 1.0))
        tree = search.AabbTree.__new__(search.AabbTree)
        tree.cpp_handle = fake
        with pytest.raises(ValueError, match="Origins and directions must be Nx3"):
            tree.ray_count(np.zeros((4, 2)), d)
        with pytest.raises(ValueError, match="Origins and directions must be Nx3"):
            tree.ray_cast_all(o, np.ones((3, 3)))
        with pytest.raises(ValueError, match="t0 <= t1"):
            tree.ray_cast_all(o, d, (1.0, 0.0), points=True, sides=True)
    finally:
        fake.ptr = fake_n.ptr = fake_p.ptr = None


def test_methods_exist():
    from mesh_amd import search, spatialsearch
    from mesh_amd.mesh import Mesh
    assert callable(Mesh.ray_cast_all)
    assert callable(search.AabbTree.ray_count) and callable(search.AabbTree.ray_cast_all)
    assert callable(spatialsearch.aabbtree_raycast_count) and callable(spatialsearch.aabbtree_raycast_all)


@pytest.mark.parametrize("mutation", [None, "MUTATE_ALLHITS_KEY"])
def test_t_key_is_monotone(tmp_path, mutation):
    """The radix key of a hit parameter (common.h allhits_t_key) over 400k sorted non-negative doubles -- denormals,
    adjacent ulps around every seventh power of two, +inf -- is strictly monotone, +inf orders last and -0.0 gets +0.0's
    key.  A host build of the kernels' own header.  The mutated build (the raw bits of t) must report the -0.0
    violation, which shows that the check reaches it."""
    exe = str(tmp_path / "raycast_all_key_check")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
           os.path.join(ROOT, "tests", "csrc", "raycast_all_key_check.cpp"), "-I", os.path.join(ROOT, "mesh_amd", "csrc"),
           "-o", exe]
    if mutation:
        cmd.insert(1, "-D" + mutation)
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    line = [x for x in out.stdout.splitlines() if x.startswith("values=")][-1]
    viol = int(line.split(" violations=")[1].split()[0])
    zero = int(line.split("zero_violations=")[1].split()[0])
    if mutation is None:
        assert out.returncode == 0 and viol == 0, out.stdout + out.stderr
    else:
        assert out.returncode == 1 and zero == 1 and viol == 1, out.stdout + out.stderr
