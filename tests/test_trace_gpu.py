"""The intersection arithmetic on the device: pt_debug_trace_probe (csrc/pt_debug.hip k_trace_probe, one row per lane through csrc/pt_probe.h trace_probe) held
bit for bit to the host build of the same function on EVERY row of every kind -- the degenerate rows included; this is where cn_plane's two implementations
(the device converts a _Float16, the host shifts bits) and the device's own FMA and reciprocal meet the host's -- and to the exact model of
tests/golden/gen_trace_kat.py with the assertions of tests/test_trace_model.py.  One context, one launch per kind."""
import ctypes as C

import numpy as np
import pytest

from tests import trace_kat_io as io

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def host(kat):
    return io.run_all(io.host_fn(), kat)


@pytest.fixture(scope="module")
def dev(kat):
    from vk_raytrace_amd import capi
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.pt_create(0, C.byref(ctx)) == 0
    try:
        out = io.run_all(L.pt_debug_trace_probe, kat, ctx)
        # bad arguments are refused before anything is launched
        a, o = np.zeros((4, 36), np.float32), np.zeros((4, 12), np.float32)
        fn = L.pt_debug_trace_probe
        out["refused"] = [fn(ctx, io.TRP_NODE, 4, a.ctypes.data, 35, o.ctypes.data, 12), fn(ctx, io.TRP_TRI, 4, a.ctypes.data, 36, o.ctypes.data, 3),
                          fn(ctx, 7, 4, a.ctypes.data, 36, o.ctypes.data, 12), fn(ctx, io.TRP_NODE, 4, None, 36, o.ctypes.data, 12)]
        out["invalid"] = capi.PT_ERR_INVALID
    finally:
        L.pt_destroy(ctx)
    return out


def test_device_equals_the_host_build_bit_for_bit(host, dev):
    for name, want in host.items():
        bad = io.same_bits(dev[name], want)
        assert bad == 0, f"{name}: device and host build differ in {bad} words"
    assert dev["refused"] == [dev["invalid"]] * 4


def test_device_t1_t2(kat, dev):
    io.check_t1(dev["world_tri"], kat, "device")
    io.check_t2(dev["tri"], kat, "device")
    io.check_lattice(dev["tri"], kat, "device")


@pytest.mark.parametrize("compact", [False, True], ids=["wide", "compact"])
def test_device_node_visits(kat, dev, compact):
    lost, loose, order = io.check_nodes(dev["cnode" if compact else "node"], kat, compact, "device")
    assert not lost, f"{len(lost)} exact hits lost: {lost[:5]}"
    assert not loose, f"{len(loose)} reports outside the derived margin: {loose[:5]}"
    assert not order, f"{len(order)} visits out of order: {order[:3]}"
    io.check_degenerate_nodes(dev["cnode_degenerate" if compact else "node_degenerate"], kat, compact, "device")


def test_device_cn_plane_raybox_enter(kat, dev):
    io.check_cn_plane(dev["cn_plane"], "device")
    io.check_raybox(dev["raybox"], io.raybox_rows(kat), "device")
    io.check_enter(dev["enter"], dev["raybox"][len(kat["node_in"]):], kat, "device")
