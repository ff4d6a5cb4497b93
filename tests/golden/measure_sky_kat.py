"""Measures the tolerance of tests/test_sky_model.py and tests/test_sky_gpu.py against the reference's own shader.

Evaluates oracle/_ref/libref.so (shaders/sun_and_sky.glsl compiled by oracle/ref_glue/; needs the reference tree, so this runs where that library can be built)
through ref_sun_and_sky on the KEPT rows of tests/golden/sky_kat.npz and writes, per class of gen_sky_kat.CLASSES, the maximum of the fixture's error measure
against the float64 expectation into tests/golden/sky_kat_tol.json, with the kept count, the dropped count, the class's spread and the date.  The tests' bound
for every leg is 4 x the maximum of the class (the project's factor, for measure_float_kat.py's reason: the legs are meant to be bit-identical to the
reference, the factor absorbs a deliberate 1-ulp change of include/pt_fpmath.h).  Per class, so that the physically scaled disc and the smoothstep's rise do
not loosen the rest.  Guard rail as in measure_float_kat.py: a recorded maximum above 1e-3 rejects the fixture -- change the inputs or the spread in
gen_sky_kat.py instead.  Nothing here is taken from the product.

Run:  python tests/golden/measure_sky_kat.py   (after gen_sky_kat.py)
"""
import datetime
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import ref, sky_kat_io as io  # noqa: E402


def main():
    if not ref.available():
        sys.exit("oracle/_ref/libref.so cannot be built here (no reference tree)")
    kat = io.load()
    got = io.through_call(ref.lib().ref_sun_and_sky)(kat["rows"])
    err = io.errors(kat, got)
    out = {"SPREAD": float(kat["SPREAD"]), "date": datetime.date.today().isoformat(), "measure": str(kat["measure"]), "rows": int(len(got)), "classes": {}}
    for k, name in enumerate(kat["class_names"]):
        m = kat["row_class"] == k
        kept = m & kat["kept"]
        assert np.isfinite(err[kept]).all(), f"{name}: non-finite value on a kept row"
        worst = float(err[kept].max())
        assert worst <= 1e-3, f"{name}: recorded maximum {worst:.3g} exceeds the 1e-3 guard rail: change the inputs or the spread"
        out["classes"][str(name)] = {"max_error": worst, "kept": int(kept.sum()), "dropped": int((m & ~kat["kept"]).sum()), "spread": float(kat["class_spread"][k])}
        print(f"{str(name):24s} max {worst:.3e}  median {np.median(err[kept]):.2e}  kept {int(kept.sum())} of {int(m.sum())}")
    with open(os.path.join(HERE, "sky_kat_tol.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
