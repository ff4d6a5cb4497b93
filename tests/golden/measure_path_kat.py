"""Records what tests/test_path_model.py and tests/test_path_gpu.py take from the reference's own code.

  python tests/golden/measure_path_kat.py --table    (before gen_path_kat.py)
      the alias table of the fixture's environment from the compiled reference's createEnvironmentAccel (src/hdr_sampling.cpp) -> tests/golden/path_kat_env.npz;
      the model of gen_path_kat.py takes it as an input.
  python tests/golden/measure_path_kat.py            (after gen_path_kat.py)
      runs oracle/_ref/libref.so (pathtrace.comp / pathtrace.rgen compiled by oracle/ref_glue/; needs the reference tree) on every configuration of
      tests/golden/path_kat.npz and path_kat_sky.npz (the sun & sky configurations) and writes, per image, the maximum over the KEPT pixels of |ref - f64| / max(1, |f64|) into tests/golden/path_kat_tol.json, with
      the pixel counts and the date.  The test's bound for every leg is 4 x that maximum (the factor of the other model tests: the legs differ from the reference
      by the rounding of libm against ocml, a few ulps per call, not by a rule); an image the reference reproduces exactly is held to equality.  Guard rail (the
      project's parity bar, bench.py's per-pixel L2 of 1e-3): a recorded maximum above 1e-3 rejects the fixture.  Never taken from the product.
"""
import ctypes as C
import datetime
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import path_kat_io as io, ref  # noqa: E402


def table():
    gen = io.generator()
    env = gen.environment()
    h, w = env.shape[:2]
    acc = np.zeros((w * h, 4), np.uint32)
    i, a = C.c_float(), C.c_float()
    assert ref.lib().ref_env_accel(env.ctypes.data, w, h, acc.ctypes.data, C.byref(i), C.byref(a)) == w * h
    gen.gs.write_npz(os.path.join(HERE, "path_kat_env.npz"), dict(env=env, env_table=acc, env_integral=np.float32(i.value), env_average=np.float32(a.value)))   # the same bytes on every run
    print("recorded", w * h, "texels, integral", i.value, "average", a.value)


def main():
    if not ref.available():
        sys.exit("oracle/_ref/libref.so cannot be built here (no reference tree)")
    if "--table" in sys.argv:
        return table()
    kat = io.load()
    images = {}
    for name, img in io.render_all(kat, io.reference):
        e, kept = io.error(kat, name, img)
        assert e <= 1e-3, f"{name}: recorded maximum {e:.3g} exceeds the 1e-3 guard rail"
        print(f"{name:18s} max {e:.3e} over {kept} kept pixels")
        images[name] = {"max": e, "kept": kept, "pixels": int(img.shape[0] * img.shape[1])}
    out = {"date": datetime.date.today().isoformat(), "measure": "max over kept pixels of |ref - f64| / max(1, |f64|), per image", "images": images}
    with open(os.path.join(HERE, "path_kat_tol.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
