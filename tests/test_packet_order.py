"""The packet stage's child order on the CPU (csrc/pt_order.h compiled for the host by tests/cpp/packet_order_host.cpp).

1. The table: one byte per direction-sign octant, the four child slots nearest first at 2 bits each, stored XOR 0xE4.  On random and degenerate
   nodes (1 to 4 children, empty slots anywhere, equal boxes, flat boxes, huge coordinates) every byte is a permutation of the slots, empty slots
   come last, the order is non-decreasing in the stated key -- the box's entry corner projected on the octant's diagonal, (x + y) + z in float32,
   recomputed here with numpy -- with ties in slot order, and a zeroed pad decodes to slot order.
2. The walk: a plain model of the 64-ray packet walk with the order policy as a parameter (sorted by first-lane entry distance / the table / slot
   order, which is what a zeroed pad gives / the table reversed), on eight fuzz scenes with opaque, MASK and BLEND triangles seen along the eight
   octants.  After the settle rule (needs_count_pass, settle_draws, the exact loop) every ray's hit record -- t, triangle, barycentrics -- and RNG
   state equal those of the per-lane machine started at the root, under every policy: the order changes how a ray is settled, never what it ends with."""
import ctypes as C

import numpy as np
import pytest

from tests import host_harness as hh
from vk_raytrace_amd import synth

NONE, LEAF = 0xFFFFFFFF, 0x80000000
_P, _I, _U = C.c_void_p, C.c_int, C.c_uint32
SIGNATURES = [
    ("po_encode", None, [_U, _P, _P, _P, _P]),
    ("po_byte", _U, [_U, _U, _U]),
    ("po_write_node", None, [_P]),
    ("po_packet_routes", _U, [_P, _I, _U] + [_P] * 7),
]
POLICIES = {"sorted": 0, "table": 1, "slot order": 2, "table reversed": 3}


@pytest.fixture(scope="module")
def lib():
    return hh.bind(hh.build_library("libpacketorder", ["packet_order_host.cpp"]), SIGNATURES)


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------------------------
def nodes():
    """lo, hi (n, 3, 4) float32 and child references (n, 4)"""
    rng = np.random.default_rng(11)
    lo, hi, cc = [], [], []

    def add(l, h, present):
        l, h = np.array(l, np.float32), np.array(h, np.float32)
        c = np.where(present, np.arange(4, dtype=np.uint32) + 7, NONE).astype(np.uint32)
        l[:, ~np.asarray(present)] = np.finfo(np.float32).max    # an empty slot's box is inverted
        h[:, ~np.asarray(present)] = -np.finfo(np.float32).max
        lo.append(l); hi.append(h); cc.append(c)

    masks = [[bool(m >> k & 1) for k in range(4)] for m in range(1, 16)]   # 1 to 4 children in every combination of slots
    for i in range(600):
        c = rng.uniform(-10, 10, (3, 4))
        e = rng.uniform(0, 3, (3, 4))
        add(c - e, c + e, masks[i % 15])
    for m in masks:
        one = rng.uniform(-5, 5, (3, 1))
        add(np.repeat(one, 4, 1), np.repeat(one + 1.5, 4, 1), m)                        # equal boxes: every key ties
        c = rng.uniform(-5, 5, (3, 4))
        add(c, c.copy(), m)                                                            # flat in every axis (points)
        e = rng.uniform(0, 2, (3, 4)); e[rng.integers(3)] = 0.0
        add(c, c + e, m)                                                               # flat in one axis
        g = np.round(rng.uniform(-2, 2, (3, 4)))                                       # lattice boxes: many partial ties
        add(g, g + 1.0, m)
        add(c * 1e30, c * 1e30 + 1e29, m)                                              # sums that overflow to infinity
    return np.stack(lo), np.stack(hi), np.stack(cc)


def test_order_table(lib):
    lo, hi, cc = nodes()
    n = len(cc)
    out = np.zeros((n, 2), np.uint32)
    lib.po_encode(n, np.ascontiguousarray(lo).ctypes.data, np.ascontiguousarray(hi).ctypes.data, np.ascontiguousarray(cc).ctypes.data, out.ctypes.data)
    stored = out.view(np.uint8).reshape(n, 8)
    assert len({bytes(r) for r in stored}) > 100, "the nodes must differ in their tables"
    for o in range(8):
        byte = stored[:, o] ^ 0xE4
        for i in range(0, n, 97):
            assert lib.po_byte(int(out[i, 0]), int(out[i, 1]), o) == byte[i]
        order = np.stack([(byte >> (2 * i)) & 3 for i in range(4)], 1).astype(np.int64)           # (n, 4): slots, nearest first
        assert (np.sort(order, 1) == np.arange(4)).all(), "a permutation of the slots"
        with np.errstate(over="ignore", invalid="ignore"):
            part = [np.where(o >> a & 1, -hi[:, a, :], lo[:, a, :]).astype(np.float32) for a in range(3)]
            key = ((part[0] + part[1]).astype(np.float32) + part[2]).astype(np.float32)           # (n, 4) by slot
        empty = np.take_along_axis(cc == NONE, order, 1)
        k = np.take_along_axis(key, order, 1)
        for i in range(3):
            a_e, b_e = empty[:, i], empty[:, i + 1]
            assert not (a_e & ~b_e).any(), "empty slots come last"
            both = ~a_e & ~b_e
            assert (k[both, i] <= k[both, i + 1]).all(), "non-decreasing in the key"
            tie = (both & (k[:, i] == k[:, i + 1])) | (a_e & b_e)
            assert (order[tie, i] < order[tie, i + 1]).all(), "ties (and the empty slots) in slot order"
    assert lib.po_byte(0, 0, 0) == 0xE4 and all(lib.po_byte(0, 0, o) == 0xE4 for o in range(8)), "a zeroed pad decodes to slot order"


def test_table_lands_in_the_first_eight_pad_bytes(lib):
    lo, hi, cc = nodes()
    for i in (0, 5, 601, len(cc) - 1):
        node = np.zeros(32, np.uint32)
        node[0:12] = lo[i].reshape(12).view(np.uint32)
        node[12:24] = hi[i].reshape(12).view(np.uint32)
        node[24:28] = cc[i]
        node[28:32] = 0xDEADBEEF
        before = node.copy()
        lib.po_write_node(node.ctypes.data)
        want = np.zeros(2, np.uint32)
        lib.po_encode(1, np.ascontiguousarray(lo[i]).ctypes.data, np.ascontiguousarray(hi[i]).ctypes.data, np.ascontiguousarray(cc[i]).ctypes.data, want.ctypes.data)
        assert np.array_equal(node[:28], before[:28]) and np.array_equal(node[28:30], want) and np.array_equal(node[30:], before[30:])


# ---- 2. the walk --------------------------------------------------------------------------------------------------------------------------------------
SIDE = 40   # 40 x 40 pixels = 25 packets of 8 x 8 per scene
OCTANTS = [(sx, sy, sz) for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)]


def packet_rays(eye, center, fov=55.0):
    """pinhole rays through the pixel centres of a SIDE x SIDE image, in packets of 8 x 8 pixels"""
    eye, center = np.asarray(eye, np.float64), np.asarray(center, np.float64)
    fwd = center - eye; fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, (0.0, 1.0, 0.0)); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    th = np.tan(np.radians(fov) / 2)
    ys, xs = np.mgrid[0:SIDE, 0:SIDE]
    d = fwd + ((2 * (xs + 0.5) / SIDE - 1) * th)[..., None] * right + ((1 - 2 * (ys + 0.5) / SIDE) * th)[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d.reshape(SIDE // 8, 8, SIDE // 8, 8, 3).transpose(0, 2, 1, 3, 4).reshape(-1, 3)   # block by block, 64 rays each
    return np.ascontiguousarray(np.broadcast_to(eye, d.shape), np.float32), np.ascontiguousarray(d, np.float32)


@pytest.fixture(scope="module")
def walks(lib):
    """per scene and policy: the route from the root, the route through the packet model, the way each ray took, the walk's statistics"""
    out = []
    for seed, octant in enumerate(OCTANTS):
        tr = hh.TracedScene(synth.fuzz_scene(seed))
        try:
            org, dirs = packet_rays(tuple(5.5 * s for s in octant), (0.3, -0.2, 0.1))
            seeds = np.random.default_rng(100 + seed).integers(0, 2 ** 32, len(org), dtype=np.uint64).astype(np.uint32)
            per = {}
            for name, policy in POLICIES.items():
                a, b = np.zeros((len(org), 7), np.uint32), np.zeros((len(org), 7), np.uint32)
                route, stats = np.zeros(len(org), np.uint32), np.zeros(4, np.uint64)
                over = lib.po_packet_routes(tr.h, policy, len(org) // 64, org.ctypes.data, dirs.ctypes.data, seeds.ctypes.data, a.ctypes.data, b.ctypes.data, route.ctypes.data,
                                            stats.ctypes.data)
                assert over == 0, "traversal stack overflow"
                per[name] = (a, b, route, stats)
            out.append((seed, per))
        finally:
            tr.close()
    return out


@pytest.mark.parametrize("policy", list(POLICIES))
def test_every_order_ends_with_the_per_lane_result(walks, policy):
    ways = np.zeros(4, np.int64)
    hits = 0
    for seed, per in walks:
        a, b, route, stats = per[policy]
        for k, name in enumerate(("hit.t", "hit.triangle", "hit.u", "hit.v", "seed afterwards")):
            bad = np.nonzero(a[:, k] != b[:, k])[0]
            assert bad.size == 0, f"fuzz scene {seed}, {policy}: {name} of {bad.size} rays differs from the per-lane result, first {bad[:5]}"
        ways += np.bincount(route, minlength=4)
        hits += int((a[:, 1] != NONE).sum())
        assert stats[2] > 0, "packets were traversed"
    print(f"{policy}: settled by the packet {ways[0]}, handed over {ways[1]}, exact loop {ways[2]}, in sign-incoherent packets {ways[3]}; rays with a hit {hits}")
    assert ways[0] > 0 and ways[1] > 0 and ways[2] > 0, "every way out of the packet stage must occur"


def test_the_orders_differ_in_work_only(walks):
    """the policies do walk differently (else the test above compares nothing): visit counts differ, and the table needs no more node visits than
    its reverse"""
    total = {name: np.sum([per[name][3][:2] for _, per in walks], 0) for name in POLICIES}
    print({k: v.tolist() for k, v in total.items()})
    assert len({tuple(v.tolist()) for v in total.values()}) == len(POLICIES)
    assert total["table"].sum() < total["table reversed"].sum()
