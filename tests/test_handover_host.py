"""The hand-over of the packet stage's pass A to the trace machine, on the CPU (tests/cpp/handover_host.cpp: the product's pt_trace.h,
pt_machine.h and pt_settle.h compiled for the host, the th_handover entry point of the host harness, tests/host_harness.py).

Claim under test: a ray whose pass A cannot stand may enter pass B with the pass-A hit somebody else computed -- stored
by store_handover, restored by lane_fetch_handover -- and nothing observable changes: the hit record, the RNG state afterwards, the number of
draws and the way the ray took (settled by the two passes / by the exact key-ordered loop) are those of a lane that started at the root.  Rays
known to need the exact loop after pass A go straight to it; they must arrive at the same record too.  Every case the rule distinguishes is
asserted to occur in the fixture, on the flat and on the two-level structure."""
import numpy as np
import pytest

from tests.handover_scene import handover_scene, EYE
from tests.host_harness import NONE, TracedScene

TF_SAW_ZERO, TF_SAW_FRAC, TRI_OPAQUE = 1, 2, 1


def fixed_rays(n_side=72):
    """camera rays through a regular grid over the cards (the outermost ones pass beside them and meet the wall or nothing), fixed seeds"""
    eye = np.asarray(EYE, np.float64)
    x, y = np.meshgrid(np.linspace(-1.45, 1.45, n_side), np.linspace(-1.45, 1.45, n_side))
    target = np.stack([x.ravel() + 0.003, y.ravel() - 0.002, np.full(x.size, 0.5)], 1)
    d = target - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    org = np.broadcast_to(eye, d.shape)
    seeds = np.random.default_rng(20240607).integers(0, 2 ** 32, len(d), dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(org, np.float32), np.ascontiguousarray(d, np.float32), seeds


@pytest.fixture(scope="module")
def routes():
    """both routes for every ray, flat and two-level: computed once"""
    sc = handover_scene()
    tr = TracedScene(sc)
    org, dirs, seeds = fixed_rays()
    out = {}
    try:
        for two in (0, 1):
            a, b, info = np.zeros((len(org), 7), np.uint32), np.zeros((len(org), 7), np.uint32), np.zeros((len(org), 9), np.uint32)
            over = tr.L.th_handover(tr.h, two, len(org), org.ctypes.data, dirs.ctypes.data, seeds.ctypes.data, a.ctypes.data, b.ctypes.data, info.ctypes.data)
            assert over == 0, "traversal stack overflow"
            out[two] = (a, b, info)
    finally:
        tr.close()
    assert sc.num_triangles < 1000
    return out, seeds


def classify(info):
    flags, bt = info[:, 0], info[:, 5].view(np.float32)
    z = info[:, 2:5].view(np.float32)
    hit = info[:, 6] != NONE
    frac_a, frac_front = (flags & TF_SAW_FRAC) != 0, (info[:, 7] & TF_SAW_FRAC) != 0
    return {
        "three or more zero-opacity candidates behind the hit": hit & ~frac_a & (z[:, 2] > bt),
        "a zero-opacity candidate tying the hit in t": hit & ~frac_a & (z == bt[:, None]).any(1),
        "a fractional candidate in front of the hit": frac_front,
        "a fractional candidate behind the hit only": hit & frac_a & ~frac_front,
        "a non-opaque certain hit": hit & ((info[:, 6] & TRI_OPAQUE) == 0),
        "an opaque hit": hit & ((info[:, 6] & TRI_OPAQUE) != 0),
    }


@pytest.mark.parametrize("two", [0, 1], ids=["flat", "two-level"])
def test_handed_over_rays_end_like_rays_from_the_root(routes, two):
    (a, b, info), seeds = routes[0][two], routes[1]
    names = ("hit.t", "hit.triangle", "hit.u", "hit.v", "seed afterwards", "nDraw", "route")
    for k, name in enumerate(names):
        bad = np.nonzero(a[:, k] != b[:, k])[0]
        assert bad.size == 0, f"{name}: {bad.size} rays differ between the routes, first {bad[:5]}"
    handed = info[:, 8] == 1
    assert handed.sum() >= 20, "the fixture must hand rays over"
    cases = classify(info)
    for name, m in cases.items():
        assert m.any(), f"the fixture holds no ray with {name}"
    # the two cases pass B exists for are handed over, never settled by pass A alone
    assert handed[cases["three or more zero-opacity candidates behind the hit"]].all()
    assert handed[cases["a zero-opacity candidate tying the hit in t"]].all()
    # a ray with a fractional candidate in front of its hit takes the exact loop on both routes; one handed over never has a miss
    assert (a[cases["a fractional candidate in front of the hit"], 6] == 1).all()
    assert (info[handed, 6] != NONE).all()
    # draws were consumed (the seed moved) exactly where draws are counted
    assert np.array_equal(a[:, 4] != seeds, a[:, 5] > 0)


def test_the_two_structures_agree(routes):
    """flat and two-level name the triangle differently in the hit record (leaf slot / world index) and walk in different orders (a ray may take
    the exact loop on one and not on the other); what a ray ends with is the same ray for ray"""
    (a0, _, i0), (a1, _, i1) = routes[0][0], routes[0][1]
    for k in (0, 2, 3, 4, 5):
        assert np.array_equal(a0[:, k], a1[:, k]), k
    assert np.array_equal(i0[:, 5], i1[:, 5]) and np.array_equal(i0[:, 6], i1[:, 6])
