"""The intersection arithmetic of csrc/pt_trace.h held to an EXACT model, one function at a time -- the CPU legs.

The layer under the shading, texture, surface and display models: tri_test (trace contract T2 / T3), world_tri (T1 at a two-level leaf), make_raybox with
wide_node_step / wide_node_decide (the fused slab test), cnode_visit with cn_plane (the 80-byte nodes) and enter_instance.  VkAccelerationStructureKHR is
implementation-defined, so no reference program text lies behind it: "device == host build == oracle" only says that three copies of one formula agree, and the
box tests are otherwise seen through whole walks compared with a brute force that calls the same tri_test.  Here each function is called ON ITS OWN through
    th_trace_probe (tests/cpp: the product's headers, host build)    orc_trace_probe (the oracle's own T1 - T3; TRP_TRI and TRP_WORLD_TRI only)
    pt_debug_trace_probe (the same headers on the device, one row per lane: tests/test_trace_gpu.py)
-- row layouts in vk_raytrace_amd/csrc/pt_probe.h trace_probe -- and held to tests/golden/gen_trace_kat.py: fractions.Fraction on the fp32 inputs, so truth has
no rounding at all.  What is asserted (the derivations are in the generator's docstring, the code in tests/trace_kat_io.py):
  1  T1: every leg equals the bit model (each operation rounded once from the exact rational, signed zeros included).
  2  T2 on decided rows: the verdict is the exact one, |t - t*|, |u - u*|, |v - v*| are within the row's DERIVED forward-error bound (nothing measured, no
     tolerance file), culling follows the sign of the exact det under all four flag combinations and both windings; on the exact lattice verdict and t, u, v are
     the exact values -- u == 0, v == 0, u + v == 1 and the vertices accepted, det == 0 rejected.
  3  The caps that keep 2 honest: at most 5 % of the interior set and 50 % of the sliver set are undecided; no lattice row is.
  4  Slab test, one-sided: wherever the exact ray / box interval is non-empty the child is reported, in both node forms, alphaOnly filtering by BVH_ALPHA.
  5  Slab test, tightness: a reported child has a non-empty exact interval against the box grown by the derived margin g_a.
  6  Order: the children reported are exactly the hit set, pushed farthest first, the nearest returned (ties and the margins may fall either way).
  7  cn_plane: all 2048 grid integers decode to themselves from either half of a word.
  8  enter_instance == make_raybox of the transformed ray widened by eps |idir|, within the fp32 rounding of that expression.
  Degenerate rows (Inf, NaN, denormals, repeated vertices, coordinates up to 1e30): host == oracle bits only, and a node visit reports nothing but the row's own
  children, never BVH_NONE.

First run: every assertion holds on the host build and on the oracle; the figures each test prints:
  undecided: interior 1.7 %, miss 0.8 %, sliver 32 %, flags 2.7 %, lattice 0;
  T2, 2112 accepted decided rows: largest error / bound 0.39 (t), 0.41 (u), 0.41 (v) -- the bound is tight to about 2.5 x, so an error of a few ulps would show;
  box tests: 0 of 1527 exact hits lost in either node form, no report outside the derived margin (wide 1829 reported, 302 of them inside the margin only; compact
  1842 and 315), 291 / 295 visits with more than one child to put in order, none out of order.
That the check can fail (the product mutated in a scratch copy of the host build, one line at a time; DESIGN.md section 3 has the list): a bias of 0 in make_raybox,
both decision factors at 1 and a compact bias of 0 lose exact hits; a bias of 2^-19 breaks the margin; u >= 1, v <= 0, cross(e2, d), one more rounding in t, the other
association in T1, near-to-far pushes, a wrong shift in the host cn_plane and eps without padC0 each fail the assertion written for them.  A QUARTER of either bias
(2^-23, 2e-7) loses nothing: the constants carry that much slack over the roundings they absorb, which is why tightness is asserted as well.
"""
import numpy as np
import pytest

from tests import trace_kat_io as io


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def legs(kat):
    """every row of every kind through the host build, the triangle kinds through the oracle, once"""
    return {"host": io.run_all(io.host_fn(), kat), "orc": io.run_all(io.orc_fn(), kat, kinds=(io.TRP_TRI, io.TRP_WORLD_TRI))}


def test_fixture_is_what_the_issue_asks_for(kat):
    io.check_fixture(kat)


def test_the_models_rounding_is_ieee():
    """rnd (integers, ties to even) against the hardware's float64 -> float32 conversion, which rounds once: normal, denormal and halfway cases"""
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.normal(size=500) * 10.0 ** rng.uniform(-44, 38, 500), (np.arange(1, 200) + 0.5) * 2.0 ** -149, 1.0 + (np.arange(64) + 0.5) * 2.0 ** -23,
                        [2.0 ** -126, 2.0 ** -127, 2.0 ** -150, 3.0 * 2.0 ** -150, 0.1, 1.0 / 3.0, 16777217.0]])
    x = x[np.abs(x) < 3e38]
    assert [float(io.gen.rnd(io.gen.Fr(float(v)))) for v in x] == x.astype(np.float32).astype(np.float64).tolist()
    assert io.gen.fmul(-0.0, 3.0) == 0 and np.signbit(io.gen.fmul(-0.0, 3.0)) and not np.signbit(io.gen.fadd(1.5, -1.5)) and np.signbit(io.gen.fadd(-0.0, -0.0))


@pytest.mark.parametrize("leg", ["host", "orc"])
def test_t1_equals_the_bit_model(kat, legs, leg):
    io.check_t1(legs[leg]["world_tri"], kat, leg)


@pytest.mark.parametrize("leg", ["host", "orc"])
def test_t2_decided_rows_meet_the_exact_verdict_and_the_derived_bound(kat, legs, leg):
    worst = io.check_t2(legs[leg]["tri"], kat, leg)
    assert worst > 0.01  # the bound is not vacuous: the legs use a visible part of it


@pytest.mark.parametrize("leg", ["host", "orc"])
def test_t2_lattice_rows_are_exact(kat, legs, leg):
    io.check_lattice(legs[leg]["tri"], kat, leg)


def test_host_build_equals_the_oracle_bit_for_bit(legs):
    for name in ("tri", "tri_degenerate", "world_tri"):
        bad = io.same_bits(legs["host"][name], legs["orc"][name])
        assert bad == 0, f"{name}: host build and oracle differ in {bad} words"


def test_oracle_has_no_box_arithmetic(kat):
    for kind in (io.TRP_RAYBOX, io.TRP_NODE, io.TRP_CNODE, io.TRP_CN_PLANE, io.TRP_ENTER, 7, -1):
        assert io.orc_fn()(kind, 1, kat["node_in"].ctypes.data, 36, np.zeros(12, np.float32).ctypes.data, 12) == -1


@pytest.fixture(scope="module")
def visits(kat, legs):
    return {compact: io.check_nodes(legs["host"]["cnode" if compact else "node"], kat, compact, "host, compact" if compact else "host") for compact in (False, True)}


@pytest.mark.parametrize("compact", [False, True], ids=["wide", "compact"])
def test_slab_test_never_loses_an_exact_hit(visits, compact):
    lost = visits[compact][0]
    assert not lost, f"{len(lost)} children with a non-empty exact interval were not reported: {lost[:5]}"


@pytest.mark.parametrize("compact", [False, True], ids=["wide", "compact"])
def test_slab_test_is_tight_to_the_derived_margin(visits, compact):
    loose = visits[compact][1]
    assert not loose, f"{len(loose)} children reported although the ray misses the box grown by the derived margin: {loose[:5]}"


@pytest.mark.parametrize("compact", [False, True], ids=["wide", "compact"])
def test_visit_order_is_far_to_near(visits, compact):
    order = visits[compact][2]
    assert not order, f"{len(order)} visits out of order: {order[:3]}"


def test_degenerate_nodes_report_only_their_own_children(kat, legs):
    io.check_degenerate_nodes(legs["host"]["node_degenerate"], kat, False, "host")
    io.check_degenerate_nodes(legs["host"]["cnode_degenerate"], kat, True, "host, compact")


def test_cn_plane_decodes_every_grid_integer(legs):
    io.check_cn_plane(legs["host"]["cn_plane"], "host")


def test_raybox_brackets_the_exact_parameter(kat, legs):
    io.check_raybox(legs["host"]["raybox"], io.raybox_rows(kat), "host")


def test_enter_instance_is_the_raybox_of_the_transformed_ray_widened_by_eps(kat, legs):
    io.check_enter(legs["host"]["enter"], legs["host"]["raybox"][len(kat["node_in"]):], kat, "host")


def test_probe_rejects_what_it_cannot_hold(kat):
    p = io.host_fn()
    a, o = np.zeros((4, 36), np.float32), np.zeros((4, 12), np.float32)
    assert p(io.TRP_NODE, 4, a.ctypes.data, 35, o.ctypes.data, 12) == -1 and p(io.TRP_TRI, 4, a.ctypes.data, 36, o.ctypes.data, 3) == -1
    assert p(7, 4, a.ctypes.data, 36, o.ctypes.data, 12) == -1 and p(-1, 4, a.ctypes.data, 36, o.ctypes.data, 12) == -1
    assert p(io.TRP_NODE, 4, a.ctypes.data, 36, o.ctypes.data, 12) == 0
