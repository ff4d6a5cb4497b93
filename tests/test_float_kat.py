"""The shading math held to an INDEPENDENT float64 model, function by function.

Every other float check compares the HIP code, the CPU oracle (oracle/*.h) and the reference's compiled shaders (oracle/_ref/libref.so) with each
other, bit for bit -- and all three take their GLSL built-ins (reflect, refract, mix, smoothstep, ...) from code written in this repository, so a
formula that is wrong the same way on all sides passes.  tests/golden/gen_float_kat.py is the leg that shares nothing with them: numpy, written
from the shader text, evaluated in float64.  Here each function is called ON ITS OWN through the array probes

    orc_shading_probe (oracle)   ref_shading_probe (compiled reference)   th_shading_probe (the product's headers, host build)
    pt_debug_shading_probe (the same headers on the device, one state per lane: vk_raytrace_amd/csrc/pt_probe.h)

and held to the model: within 4 x the error the compiled reference itself shows against float64 (tests/golden/float_kat_tol.json, written by
tests/golden/measure_float_kat.py; the legs are meant to be bit-identical to the reference, the factor absorbs a deliberate 1-ulp change of
include/pt_fpmath.h) on the well-conditioned ("kept") states, RNG state after a sample call exact; and to each other bit for bit on EVERY stored
state, ill-conditioned and dot(N, V) <= 0 ones included.  The kept mask is decided by the model alone (its float32 against its float64 evaluation).

Functions, every leg: DisneyEval, DisneySample, PbrEval, PbrSample, GetSphericalUv, CreateCoordinateSystem, getRangeAttenuation, getSpotAttenuation,
Environment_sample (hand-made alias table whose pdf values are all different, so the pdf returned names the texel index and the alias choice exactly; the
reference leg also hands back the u, v of its texture lookup), and the built-ins reflect, refract, mix, smoothstep, cross, normalize, column-major
mat4 * vec4, mat4x3 * vec4(p, 1), vec3 * mat4x3, mat4(M) * vec4(d, 0), mat3(c0, c1, c2) * v (hand-made rows: integer matrices against unit vectors, exact
and different for every mix-up of rows and columns).
Oracle and reference only, because the product has no such FUNCTION (the entry answers -1 / PT_ERR_INVALID and the test asserts that):
  * vec4 * mat4: no call site in the product.
  * EnvSample's sun-disk direction (env_sampling.glsl:111-125): written inline in shade_path (pt_shade.h); reached through the sun & sky frames of
    tests/test_trace_host.py / tests/test_gpu_parity.py, bit-identical to the oracle, which IS held to the model here.  (The rest of DirectLight -- pSelect, the
    light pick, the punctual lights, the environment NEE, lightPdf and the MIS weight -- has a per-pixel expectation of its own: tests/golden/gen_path_kat.py,
    tests/test_path_model.py, tests/test_path_gpu.py -- whose sky3 and sky0 configurations run with sun & sky in use and hold this inline code to the model.)
  * step, clamp, sign, fract, mod, atan(y, x), roundEven: all in ref_glue/glsl_compat.h (what the reference's shaders run on), step and clamp in
    oracle/glsl_math.h.  The oracle and the product write the others inline where the shaders call them -- floor / fract in the texture and environment
    filters (orc_scene.h sample_texture / sample_env, pt_surface.h:51-115), sign / mod / atan inside sun_and_sky and GetSphericalUv (pt_atan2) -- so their
    coverage is through the enclosing function (GetSphericalUv here, the sky and the filters by bit-identity with the reference).
  * the tonemap curves (tonemapping.glsl:29-105: linearTosRGB, sRGBToLinear, toneMapUncharted, toneMapHejlRichard, toneMapACES, toneMap's dispatch as
    post.frag compiles it): all on the reference, the three its display pass uses on the oracle.  The product's display pass lives in pt_render.hip next to
    the shipped kernels and is held to the oracle's by tests/test_gpu_parity.py; it has no host build.
The shaders use no transpose(), inverse() or mat3(mat4): no side defines them, there is nothing to probe.
The intersection arithmetic (tri_test, world_tri, the box tests, enter_instance: csrc/pt_trace.h) is not shading math and is OUT OF SCOPE here: it has an exact
rational model of its own, tests/golden/gen_trace_kat.py, held by tests/test_trace_model.py and tests/test_trace_gpu.py.
sun_and_sky.glsl has a float64 model of its own, tests/golden/gen_sky_kat.py, held by tests/test_sky_model.py and tests/test_sky_gpu.py on 23 settings rows
(every branch of the function) x sphere, horizon, sun-fan and at-the-sun directions; the bit-identity probes here (host build == oracle, device == host build,
six variants x 1508 directions) are rows of that fixture too.
"Thin-walled from inside" (dot(ffnormal, normal) < 0 -> F = 0, discriminant = 0 in DisneySample / PbrSample) is UNREACHABLE through the function-level
probes: they all set ffnormal = normal, as the existing orc_ / ref_bsdf_sample do; the edge rows of that name vary eta and the thin-walled flag only.  That
branch is covered by whole frames alone (thin-walled materials of synth.feature_box, bit-identical across the legs).

Where the shader itself is questionable the model follows it as written and the state is not kept (it is still compared bit for bit):
  * DisneySample, transmission: normalize(refract(...)) of the zero vector when k < 0 -> NaN; ior 1.0 makes the refraction lobe's denominator 0.
  * DisneySample, clearcoat lobe with clearcoatRoughness >= 1: ImportanceSampleGTR1 divides 0 by 0.
  * CreateCoordinateSystem returns Nb = cross(Nt, N): (Nt, N, Nb) is the right-handed order, (Nt, Nb, N) is left-handed.  Asserted as written.
Hand-made edge states the filter drops (named in the fixture with the reason): the mirror configuration of "total internal reflection" and
"thin-walled from inside" (half vector from a cancelling sum), and for the sample functions roughness 0.001, thin-walled (eta 1.001), ior 1.0 and
clearcoatRoughness 1 -- a sampled half vector sits on the lobe's peak, where 1 + (a^2 - 1) NdotH^2 and LdotH eta + VdotH cancel in float32 itself.

That the check can fail (done once, in a scratch copy: the MODEL broken one formula at a time and re-minted, the unchanged oracle run against it;
"error" = the measure on kept states, bounds are 4e-7 .. 3e-4):
  refract, sign inside flipped             refract 2, disney_sample 5e14, gltf_sample 1e2
  mix, arguments swapped                   mix 20, disney_eval 6e8, gltf_eval 2e6, disney_sample 6.5
  refraction pdf without 1 - F             disney_eval 0.95, disney_sample 0.6
  GTR2 where GTR1 belongs (clearcoat)      disney_eval 7e2, disney_sample 5.3
  one rand() too few, PbrSample            gltf_sample 1.5e4 and 816 RNG states (and minting refuses: a branch keeps < 50 states)
  one rand() too few, DisneySample         disney_sample 31 and 209 RNG states
  draw behind a true `discriminat < 0`     gltf_sample: 110 RNG states (floats unchanged: only the integer comparison sees it)
  tangent-frame product with x / y swapped disney_sample 2e12, gltf_sample 8e7
  reflect without the factor 2             reflect 1, disney_sample 4e19, gltf_sample 2e8
  smoothstep 2 - 3t                        smoothstep 75, spot_attenuation 51
  cross(N, Nt) in CreateCoordinateSystem   coordinate_system 2
  atan(x, z) in GetSphericalUv             spherical_uv 1e3
  DielectricFresnel without the 0.5        disney_eval 19, disney_sample 3e7
  F_Schlick exponent 4                     gltf_eval 0.3, gltf_sample 10
  range attenuation / distance             range_attenuation 1e3
  spot blend edges swapped                 spot_attenuation 4.5e2
  mat4 * vec4 read row-major               mat4_vec4 60
  mat4x3 * vec4(p, 1) read row-major       xform_point 26
  vec3 * mat4x3 computed as M * v          xform_rowvec 16
  cross with operands swapped              cross 20
  Environment_sample: xi.y not renormalised 1.8; alias keeps the texel's pdf 4; px / py from the wrong dimension 1.4; theta linear in xi.z 0.18
  toneMapUncharted input not doubled       toneMapUncharted 0.37, toneMap 0.37
  toneMapACES without the clamp            toneMapACES 0.015
  toneMapHejlRichard without the 0.004     toneMapHejlRichard 1
  linearTosRGB with gamma 2.4              linearTosRGB 0.42, toneMapUncharted 0.2, toneMapACES 0.33, toneMap 0.2
  toneMap ignoring the exposure            toneMap 0.86
and on the product side, host build only: `bend` with the sign flipped (pt_math.h) -> refract 2, disney_sample 1e13, gltf_sample 11;
disney_refraction's pdf without 1 - F (pt_bsdf.h) -> disney_eval 21, disney_sample 1.5: the th_ probe reaches the shipped functions.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import float_kat_io as io, orc, ref

GOLDEN = io.GOLDEN
NAMES = list(io.FUNCTIONS)
PROBED = [n for n in NAMES if n not in io.SCALARS and n not in io.TONEMAPS]   # the cases of *_shading_probe; scalar built-ins and tonemap curves: oracle / reference side only
PRODUCT = [n for n in PROBED if n not in io.PRODUCT_LACKS]


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def tol():
    with open(os.path.join(GOLDEN, "float_kat_tol.json")) as f:
        return json.load(f)


def host_probe():
    from tests import host_harness
    return host_harness.lib().th_shading_probe


def sky_rows(kat):
    """six sun & sky variants x the fixture's directions, as probe rows (pt_SunAndSky words, then the direction)"""
    from tests.test_oracle_vs_ref import sunsky_variants
    d = kat["sky_dirs"]
    rows = []
    for ss in sunsky_variants():
        words = np.frombuffer(bytes(ss), np.float32)
        rows.append(np.concatenate([np.broadcast_to(words, (len(d), len(words))), d], 1))
    return np.ascontiguousarray(np.concatenate(rows), np.float32)


# ---- the fixture itself -------------------------------------------------------------------------------------------------------------------------
def test_generator_is_independent_and_deterministic(tmp_path):
    src = open(os.path.join(GOLDEN, "gen_float_kat.py")).read()
    imports = re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, re.M)
    assert set(imports) <= {"io", "os", "sys", "zipfile", "numpy", "gen_kat"}, imports   # nothing of oracle/, tests/orc.py, tests/ref.py, vk_raytrace_amd/
    assert len(re.findall(r"#.*?:\d+-\d+", src)) >= 40   # shader lines cited per function
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_float_kat", os.path.join(GOLDEN, "gen_float_kat.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = str(tmp_path / "again.npz")
    gen.main(out)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "float_kat.npz"), "rb").read()
    assert os.path.getsize(out) < (1 << 20)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_meets_the_caps(kat, tol, name):
    gen, dropped = kat[f"{name}_counts"]
    assert gen >= 200 and dropped <= 0.02 * gen, (gen, dropped)
    kept, domain = kat[f"{name}_kept"], kat[f"{name}_domain"]
    assert not (kept & ~domain).any()                       # dot(N, V) <= 0 is outside the model's domain
    assert np.isfinite(kat[f"{name}_want"][kept]).all()
    # every hand-made edge state is kept or named with the reason it was dropped
    edges = kat[f"{name}_edge_names"]
    named = {s.split(": ")[0] for s in kat[f"{name}_edge_dropped"]}
    for e, k in zip(edges, kept[len(kept) - len(edges):]):
        assert k or e in named, e
    if name in io.SAMPLERS + ("env_sample",):
        per = kat[f"{name}_branch_kept"]
        assert (per >= 50).all(), dict(zip(kat[f"{name}_branch_names"], per))
        assert np.array_equal(per, [np.count_nonzero(kept & (kat[f"{name}_branch"] == b)) for b in range(len(per))])
    t = tol["functions"][name]
    assert tol["SPREAD"] == float(kat["SPREAD"]) and t["kept_incl_edges"] == int(kept.sum()) and (t["generated"], t["dropped"]) == (gen, dropped)   # measured on THIS fixture
    assert t["max_error"] <= 1e-3                           # the project's parity bar: a larger recorded maximum rejects the fixture


def test_coordinate_system_properties(kat):
    """the model's own answer, as properties: orthonormal; Nb = cross(Nt, N) as the shader writes it (so (Nt, N, Nb) is right-handed); N = +-z, +-y"""
    N, w = kat["coordinate_system_in"].astype(np.float64), kat["coordinate_system_want"]
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    T, B = w[:, :3], w[:, 3:]
    for a, b in ((T, T), (B, B)):
        assert np.allclose((a * b).sum(1), 1.0, atol=1e-6)
    for a, b in ((T, N), (B, N), (T, B)):
        assert np.allclose((a * b).sum(1), 0.0, atol=1e-6)
    assert np.allclose(np.cross(T, N), B, atol=1e-6)
    names = list(kat["coordinate_system_edge_names"])
    edge = w[len(w) - len(names):]
    assert np.allclose(edge[names.index("N = [0, 0, 1]")], [0, 1, 0, 1, 0, 0]) and np.allclose(edge[names.index("N = [0, 0, -1]")], [0, 1, 0, -1, 0, 0])
    assert np.allclose(edge[names.index("N = [0, 1, 0]")], [0, 0, 1, -1, 0, 0]) and np.allclose(edge[names.index("N = [0, -1, 0]")], [0, 0, 1, 1, 0, 0])


# ---- the three CPU legs against the model ----------------------------------------------------------------------------------------------------------
def check_against_model(name, kat, tol, got, leg):
    err, exact = io.errors(name, kat, got)
    kept = kat[f"{name}_kept"]
    bound = 4.0 * tol["functions"][name]["max_error"]
    worst = float(np.nanmax(err[kept]))
    print(f"{leg:9s} {name:18s} max error on {int(kept.sum())} kept states {worst:.3e} (bound {bound:.3e})")
    assert np.isfinite(err[kept]).all(), f"{leg} {name}: non-finite value on a kept state"
    assert worst <= bound, f"{leg} {name}: error {worst:.3e} against the float64 model exceeds {bound:.3e} (state {int(np.nanargmax(np.where(kept, err, -1)))})"
    assert exact[kept].all(), f"{leg} {name}: RNG state after the call differs from the model on {np.count_nonzero(~exact & kept)} kept states"


@pytest.mark.parametrize("name", PROBED)
def test_oracle_against_the_float64_model(kat, tol, name):
    check_against_model(name, kat, tol, io.run_side(orc.lib(), "orc", name, kat), "oracle")


@pytest.mark.skipif(not ref.available(), reason="needs /root/reference (or a prebuilt oracle/_ref/libref.so)")
@pytest.mark.parametrize("name", PROBED)
def test_compiled_reference_against_the_float64_model(kat, tol, name):
    check_against_model(name, kat, tol, io.run_side(ref.lib(), "ref", name, kat), "reference")   # (Environment_sample: with the u, v of its texture lookup)


@pytest.mark.parametrize("name", PRODUCT)
def test_host_build_against_the_float64_model_and_the_oracle(kat, tol, name):
    got = io.run(host_probe(), name, kat)
    check_against_model(name, kat, tol, got, "host")
    # ... and bit-identical to the oracle on the WHOLE grid: ill-conditioned states, dot(N, V) <= 0, NaN results included
    bad = io.same_bits(got, io.run(orc.lib().orc_shading_probe, name, kat))
    assert bad == 0, f"{name}: host build of the product's headers and oracle differ in {bad} values"


ORACLE_HAS = ("step", "clamp", "linearTosRGB", "sRGBToLinear", "toneMapUncharted")


@pytest.mark.parametrize("name", list(io.SCALARS) + list(io.TONEMAPS))
def test_scalar_builtins_and_tonemap_curves_against_the_float64_model(kat, tol, name):
    """step, clamp, sign(+-0), fract and mod with negative operands, atan(y, x) in four quadrants and on the axes, roundEven at .5 -- as ref_glue/glsl_compat.h
    defines them under the reference's shaders; the curves of tonemapping.glsl (0, small values, 1, the Uncharted white point, 1e4) and toneMap's dispatch as
    post.frag compiles it.  The oracle defines step, clamp and the three curves its display pass uses; where a side has no such function its entry says so."""
    got = io.run_side(orc.lib(), "orc", name, kat)
    assert (got is not None) == (name in ORACLE_HAS)
    if got is not None:
        check_against_model(name, kat, tol, got, "oracle")
    if ref.available():
        got = io.run_side(ref.lib(), "ref", name, kat)
        assert got is not None
        check_against_model(name, kat, tol, got, "reference")
        if name in io.SCALARS and name != "atan":   # on the hand-made rows (signed zeros, ties, negative operands) the answer is exact
            n = len(kat[f"{name}_edge_names"])
            assert np.array_equal(got[len(got) - n:, 0].astype(np.float64), kat[f"{name}_want"][len(got) - n:, 0])


def test_matrix_conventions_on_integer_matrices(kat):
    """the hand-made rows of the matrix products are exact in float32, and every mix-up of rows and columns gives different integers: each leg must hit
    them exactly (column-major mat4 * vec4, row vector * mat4, the affine point / direction / row-vector forms, mat3(c0, c1, c2) * v, cross handedness)"""
    for name in ("cross", "mat4_vec4", "vec4_mat4", "xform_point", "xform_rowvec", "xform_dir", "mat3_vec3"):
        n = len(kat[f"{name}_edge_names"])
        want = kat[f"{name}_want"][-n:]
        assert name == "cross" or np.array_equal(want, np.rint(want))
        legs = [io.run_side(orc.lib(), "orc", name, kat)] + ([io.run_side(ref.lib(), "ref", name, kat)] if ref.available() else [])
        if name in io.PRODUCT_LACKS:
            assert io.run(host_probe(), name, kat) is None
        else:
            legs.append(io.run(host_probe(), name, kat))
        for got in legs:
            assert np.array_equal(got[-n:].astype(np.float64), want), name


def test_environment_sample_picks_the_models_texel(kat):
    """the pdf values of the hand-made alias table are all different, so an exact pdf is an exact texel index AND alias choice: every leg, every stored state
    whose `xi.y < q` has a margin (the kept ones); xi.x = 0 and just below 1 land in the first and the last texel"""
    kept, want = kat["env_sample_kept"], kat["env_sample_want"]
    tab = kat["env_sample_in"][0, 8:40].reshape(8, 4)
    texel, alias = kat["env_sample_texel"], kat["env_sample_branch"]
    idx = np.minimum((kat["env_sample_in"][:, 0] * np.float32(8)).astype(np.int64), 7)   # the table entry looked at (x 8 is exact in float32)
    assert np.array_equal(want[:, 3], np.where(alias == 1, tab[idx, 3], tab[idx, 2]).astype(np.float64))   # the fixture's integers and its pdf say the same
    assert np.array_equal(texel, np.where(alias == 1, np.ascontiguousarray(tab[idx, 0]).view(np.uint32), idx))
    assert len(np.unique(tab[:, 2:4])) == 16 and {0, 7} <= set(texel[kept]) and set(alias[kept]) == {0, 1}
    legs = [io.run_side(orc.lib(), "orc", "env_sample", kat), io.run(host_probe(), "env_sample", kat)] + ([io.run_side(ref.lib(), "ref", "env_sample", kat)] if ref.available() else [])
    for got in legs:
        assert np.array_equal(got[kept, 3].astype(np.float64), want[kept, 3])


def test_host_build_sun_and_sky_is_the_oracles(kat):
    rows = sky_rows(kat)
    a = io.probe(host_probe(), io.SUN_AND_SKY, rows, 3)
    b = io.probe(orc.lib().orc_shading_probe, io.SUN_AND_SKY, rows, 3)
    assert np.isfinite(a).all() and a.max() > 0.1 and io.same_bits(a, b) == 0


def test_probe_rejects_what_it_cannot_hold():
    """rows narrower than the function reads, and unknown functions, are refused instead of read out of bounds"""
    p = host_probe()
    a, o = np.zeros((4, 40), np.float32), np.zeros((4, 8), np.float32)
    assert p(0, 4, a.ctypes.data, 39, o.ctypes.data, 8) == -1 and p(2, 4, a.ctypes.data, 40, o.ctypes.data, 7) == -1 and p(99, 4, a.ctypes.data, 40, o.ctypes.data, 8) == -1
    assert p(0, 4, a.ctypes.data, 40, o.ctypes.data, 8) == 0


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_probe_is_the_host_build_and_meets_the_model(kat, tol):
    """one context, one launch per function: the functions k_shade is made of, each on its own on the device, bit-identical to the host build of the
    same headers on every stored state (both BSDFs: eval and sample with the RNG state; the full sun & sky grid; frame, uv, attenuation, built-ins)
    and within the tolerance of the float64 model on the kept ones"""
    from vk_raytrace_amd import capi
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.pt_create(0, C.byref(ctx)) == 0
    try:
        dev = L.pt_debug_shading_probe
        for name in PRODUCT:
            got = io.run(dev, name, kat, ctx)
            bad = io.same_bits(got, io.run(host_probe(), name, kat))
            assert bad == 0, f"{name}: device and host build differ in {bad} values"
            check_against_model(name, kat, tol, got, "device")
        rows = sky_rows(kat)
        a = io.probe(dev, io.SUN_AND_SKY, rows, 3, ctx)
        assert io.same_bits(a, io.probe(host_probe(), io.SUN_AND_SKY, rows, 3)) == 0, "sun_and_sky: device and host build differ"
        # bad arguments are refused before anything is launched
        z, o = np.zeros((4, 40), np.float32), np.zeros((4, 8), np.float32)
        assert dev(ctx, 0, 4, z.ctypes.data, 39, o.ctypes.data, 8) == capi.PT_ERR_INVALID and dev(ctx, 99, 4, z.ctypes.data, 40, o.ctypes.data, 8) == capi.PT_ERR_INVALID
        assert dev(ctx, 17, 4, z.ctypes.data, 40, o.ctypes.data, 8) == capi.PT_ERR_INVALID   # vec4 * mat4: no such function in the product
    finally:
        L.pt_destroy(ctx)
