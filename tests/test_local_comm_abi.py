"""The in-process communicator's C entry points without a GPU: the exports, and every argument error that
needs no device. (A communicator itself needs a device: what needs one open — sr_comm_group_close's
-EBUSY, a rank opened twice — is in tests/test_gpu_local_comm.py.)"""
from __future__ import annotations

import ctypes
import errno

LOCAL_FUNCTIONS = ("sr_comm_group_open", "sr_comm_group_close", "sr_comm_open_local", "sr_comm_set_timeout",
                   "sr_comm_transport")


def test_the_five_exports(pkg):
    L = pkg.lib()
    for name in LOCAL_FUNCTIONS:
        assert name in pkg.ABI_FUNCTIONS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes


def test_group_world_bounds(pkg):
    L = pkg.lib()
    for world in (0, 65, -1):
        h = ctypes.c_void_p(1)
        assert L.sr_comm_group_open(ctypes.byref(h), world) == -errno.EINVAL
        assert not h.value
    assert L.sr_comm_group_open(None, 2) == -errno.EINVAL
    assert L.sr_comm_group_close(None) == -errno.EINVAL
    for world in (1, 64):
        g = pkg.CommGroup(world)
        assert g.world == world and g.handle
        g.close()
        g.close()   # closed already: nothing to do


def test_open_local_argument_errors(pkg):
    L = pkg.lib()
    g = pkg.CommGroup(3)
    try:
        h = ctypes.c_void_p(1)
        for rank in (-1, 3, 64):
            assert L.sr_comm_open_local(ctypes.byref(h), g.handle, rank, 0) == -errno.EINVAL
            assert not h.value
        assert L.sr_comm_open_local(ctypes.byref(h), None, 0, 0) == -errno.EINVAL
        assert L.sr_comm_open_local(None, g.handle, 0, 0) == -errno.EINVAL
        # a device that does not exist: -ENODEV, and the rank stays free (a second try is -ENODEV again, not
        # -EBUSY; the group still closes, so no communicator is open on it)
        for _ in range(2):
            assert L.sr_comm_open_local(ctypes.byref(h), g.handle, 1, 1 << 20) == -errno.ENODEV
            assert not h.value
        assert L.sr_comm_open_local(ctypes.byref(h), g.handle, 1, -1) == -errno.ENODEV
    finally:
        g.close()
    assert not g.handle


def test_null_communicator(pkg):
    L = pkg.lib()
    assert L.sr_comm_set_timeout(None, 100) == -errno.EINVAL
    t = pkg.SrTransport()
    assert L.sr_comm_transport(None, None, ctypes.byref(t)) == -errno.EINVAL
    L.sr_comm_close(None)


def test_python_errors(pkg):
    import pytest

    with pytest.raises(pkg.SrError) as e:
        pkg.CommGroup(0)
    assert e.value.errno == errno.EINVAL
    g = pkg.CommGroup(2)
    with pytest.raises(pkg.SrError) as e:
        pkg.Comm.local(g, 2, 0)
    assert e.value.errno == errno.EINVAL
    g.close()
