"""Shared by tests/test_sky_model.py, tests/test_sky_gpu.py and tests/golden/measure_sky_kat.py: the fixture of tests/golden/gen_sky_kat.py, its probe rows (the
24 words of pt_SunAndSky, then the direction: case SUN_AND_SKY of oracle/probe_rows.h and csrc/pt_probe.h) and the error measure."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np

from tests import float_kat_io

GOLDEN = float_kat_io.GOLDEN
FACTOR = 4.0   # the project's: bound = 4 x the compiled reference's recorded maximum (measure_float_kat.py gives the reason)
SUN_AND_SKY = float_kat_io.SUN_AND_SKY
same_bits = float_kat_io.same_bits


def generator():
    spec = importlib.util.spec_from_file_location("gen_sky_kat", os.path.join(GOLDEN, "gen_sky_kat.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def load(path=None):
    with np.load(path or os.path.join(GOLDEN, "sky_kat.npz")) as z:
        kat = {k: z[k] for k in z.files}
    kat["rows"] = rows(kat)
    kat["rows"].setflags(write=False)
    return kat


def tolerances():
    with open(os.path.join(GOLDEN, "sky_kat_tol.json")) as f:
        return json.load(f)


def rows(kat):
    """the probe rows in the fixture's order: per settings row the sphere directions, then that row's band, fan and sun directions"""
    out = []
    for k, words in enumerate(kat["settings"]):
        d = np.concatenate([kat["sphere"], kat["extra_dirs"][k]])
        out.append(np.concatenate([np.broadcast_to(words, (len(d), 24)), d], 1))
    out = np.ascontiguousarray(np.concatenate(out), np.float32)
    assert len(out) == len(kat["want"]) and np.array_equal(np.repeat(np.arange(len(kat["settings"])), np.bincount(kat["row_setting"])), kat["row_setting"])
    return out


def errors(kat, got):
    """the fixture's measure per row: max over the channels of |got - want| over max over the channels of |want| (0 where both are all zero); NaN where
    either side is not finite"""
    got, want = np.asarray(got, np.float64), kat["want"]
    with np.errstate(all="ignore"):
        num, den = np.abs(got - want).max(1), np.abs(want).max(1)
        e = np.where((num == 0) & (den == 0), 0.0, num / den)
    return np.where(np.isfinite(got).all(1) & np.isfinite(want).all(1), e, np.nan)


def class_maxima(kat, got):
    """class name -> (largest error on its kept rows, the row that shows it); a non-finite value on a kept row is an infinite error"""
    e = errors(kat, got)
    e = np.where(np.isnan(e), np.inf, e)
    out = {}
    for k, name in enumerate(kat["class_names"]):
        m = kat["kept"] & (kat["row_class"] == k)
        i = np.where(m)[0]
        out[str(name)] = (float(e[i].max()), int(i[e[i].argmax()])) if len(i) else (0.0, -1)
    return out


def check(kat, tol, got, leg):
    """every class within 4 x the reference's recorded maximum on its kept rows"""
    for name, (worst, row) in class_maxima(kat, got).items():
        bound = FACTOR * tol["classes"][name]["max_error"]
        print(f"{leg:10s} {name:24s} max error {worst:.3e} (bound {bound:.3e}) at row {row}")
        assert worst <= bound, f"{leg}, class {name}: error {worst:.3e} against the float64 model exceeds {bound:.3e} (row {row}: {kat['setting_names'][kat['row_setting'][row]]})"


# ---- legs: rows -> (n, 3) float32 ------------------------------------------------------------------------------------------------------------------------------
def through_probe(fn_ptr, ctx=None):
    return lambda r: float_kat_io.probe(fn_ptr, SUN_AND_SKY, r, 3, ctx)


def through_call(fn):
    """orc_sun_and_sky / ref_sun_and_sky: (const pt_SunAndSky*, const float dir[3], float out[3]), one direction per call"""
    def leg(r):
        from vk_raytrace_amd import host_device as hd
        r = np.ascontiguousarray(r, np.float32)
        out = np.zeros((len(r), 3), np.float32)
        base_in, base_out = r.ctypes.data, out.ctypes.data
        for i in range(len(r)):
            fn(C.cast(base_in + i * 108, C.POINTER(hd.SunAndSky)), base_in + i * 108 + 96, base_out + i * 12)
        return out
    return leg
