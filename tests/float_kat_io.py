"""Shared by tests/test_float_kat.py and tests/golden/measure_float_kat.py: the fixture of tests/golden/gen_float_kat.py, the probe rows
(vk_raytrace_amd/csrc/pt_probe.h) and the error measure.  Every probe -- orc_shading_probe, ref_shading_probe, th_shading_probe,
pt_debug_shading_probe -- takes (fn, n, in, in_stride, out, out_stride) and sees the states as one array."""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (probe function number, fixture key of the input rows, output words, leading columns compared by absolute error)
FUNCTIONS = {
    "disney_eval": (0, "bsdf_eval_in", 4, 0), "gltf_eval": (1, "bsdf_eval_in", 4, 0),
    "disney_sample": (2, "bsdf_sample_in", 8, 3), "gltf_sample": (3, "bsdf_sample_in", 8, 3),
    "spherical_uv": (5, "spherical_uv_in", 2, 0), "coordinate_system": (6, "coordinate_system_in", 6, 6),
    "range_attenuation": (7, "range_attenuation_in", 1, 0), "spot_attenuation": (8, "spot_attenuation_in", 1, 0),
    "reflect": (9, "reflect_in", 3, 3), "refract": (10, "refract_in", 3, 3), "mix": (11, "mix_in", 3, 0), "smoothstep": (12, "smoothstep_in", 1, 0),
}
# vectors, matrices and Environment_sample: further cases of the same probes
FUNCTIONS.update({
    "env_sample": (13, "env_sample_in", 4, 3), "cross": (14, "cross_in", 3, 3), "normalize": (15, "normalize_in", 3, 3), "mat4_vec4": (16, "mat4_vec4_in", 4, 4),
    "vec4_mat4": (17, "vec4_mat4_in", 4, 4), "xform_point": (18, "xform_point_in", 3, 3), "xform_rowvec": (19, "xform_rowvec_in", 3, 3),
    "xform_dir": (20, "xform_dir_in", 3, 3), "mat3_vec3": (21, "mat3_vec3_in", 3, 3), "sun_disk": (22, "sun_disk_in", 5, 3),
})
# pt_math.h / pt_shade.h have no row-vector times mat4; the sun-disk direction is written inline in shade_path (pt_shade.h), not a function: it is
# reached through whole frames only (tests/test_trace_host.py, tests/test_gpu_parity.py: sun & sky frames bit-identical to the oracle)
PRODUCT_LACKS = ("vec4_mat4", "sun_disk")
# the scalar built-ins go through *_glsl_builtin, the tonemap curves through *_tonemap_curve: (fn, n, in, in_stride, out, out_stride) -> 0, or -1 where
# that side has no such function
SCALARS = {"step": 0, "clamp": 1, "sign": 2, "fract": 3, "mod": 4, "atan": 5, "roundEven": 6}
TONEMAPS = {"linearTosRGB": 0, "sRGBToLinear": 1, "toneMapUncharted": 2, "toneMapHejlRichard": 3, "toneMapACES": 4, "toneMap": 5}
for _k in SCALARS:
    FUNCTIONS[_k] = (SCALARS[_k], _k + "_in", 1, 0)
for _k in TONEMAPS:
    FUNCTIONS[_k] = (TONEMAPS[_k], "tonemap_in", 3, 0)
SUN_AND_SKY = 4
SAMPLERS = ("disney_sample", "gltf_sample")
SEED_COLUMN = {"disney_sample": 7, "gltf_sample": 7, "sun_disk": 4}   # output word that holds the RNG state after the call


def load():
    with np.load(os.path.join(GOLDEN, "float_kat.npz")) as z:
        return {k: z[k] for k in z.files}


def probe(fn_ptr, fn, rows, out_words, ctx=None):
    """rows (n, w) float32 through one call of a probe (signatures: tests/orc.py, tests/ref.py, tests/host_harness.py, vk_raytrace_amd/capi.py
    DEBUG_API); returns (n, out_words) float32, or None where that side answers -1 (no such function)"""
    rows = np.ascontiguousarray(rows, np.float32)
    out = np.zeros((len(rows), out_words), np.float32)
    args = (fn, len(rows), rows.ctypes.data, rows.shape[1], out.ctypes.data, out_words)
    if ctx is None:
        return None if fn_ptr(*args) == -1 else out
    rc = fn_ptr(ctx, *args)
    assert rc == 0, f"probe {fn} failed with {rc}"
    return out


def run(fn_ptr, name, kat, ctx=None):
    fn, key, words, _ = FUNCTIONS[name]
    return probe(fn_ptr, fn, kat[key], words, ctx)


def run_side(L, prefix, name, kat):
    """function `name` on the oracle (prefix "orc") or the compiled reference ("ref") through the entry point that has it; None: not defined on that side.
    The reference's Environment_sample also hands back the (u, v) of its texture lookup (columns 4, 5)."""
    if name == "env_sample" and prefix == "ref":
        rows = np.ascontiguousarray(kat["env_sample_in"], np.float32)
        out, uv = np.zeros((len(rows), 4), np.float32), np.zeros((len(rows), 2), np.float32)
        L.ref_env_sample_uv(len(rows), rows.ctypes.data, rows.shape[1], out.ctypes.data, uv.ctypes.data)
        return np.concatenate([out, uv], 1)
    entry = "glsl_builtin" if name in SCALARS else "tonemap_curve" if name in TONEMAPS else "shading_probe"
    return run(getattr(L, f"{prefix}_{entry}"), name, kat)


def errors(name, kat, got):
    """per state: the error measure of `got` against the float64 expectation (NaN where either side is not finite), and whether the integer
    outputs (the RNG state after a sample call) are exact"""
    n_abs = FUNCTIONS[name][3]
    want = kat[f"{name}_want"][:, :got.shape[1]]   # (Environment_sample: u, v only where the side exposes them)
    g = got[:, :want.shape[1]].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(g - want) / (np.abs(want) + 1e-6)
        e[:, :n_abs] = np.abs(g - want)[:, :n_abs]
    fin = np.isfinite(g) & np.isfinite(want)
    err = np.where(fin.all(1), np.where(fin, e, 0).max(1), np.nan)
    exact = np.ones(len(got), bool)
    if name in SEED_COLUMN:
        exact = np.ascontiguousarray(got[:, SEED_COLUMN[name]]).view(np.uint32) == kat[f"{name}_seed_after"]
    return err, exact


def same_bits(a, b):
    """the rule of tests/test_fpmath.py: NaN in the same places (payload free), every other value equal as bits; returns the number of differing values"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero(an != bn) + np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~an & ~bn))
