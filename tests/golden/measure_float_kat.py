"""Measures the tolerance of tests/test_float_kat.py against the reference's own shaders.

Evaluates oracle/_ref/libref.so (the reference's GLSL compiled by oracle/ref_glue/; needs the reference tree, so this runs where that library can
be built) on the KEPT states of tests/golden/float_kat.npz and writes, per function, the maximum of the error measure against the float64
expectation into tests/golden/float_kat_tol.json, next to SPREAD, the generated / dropped counts (the 2 % cap is about these), the kept count including the hand-made edge rows and the date.  The test's bound for every leg is
4 x that maximum.  Guard rail (the project's parity bar, bench.py's per-pixel L2 of 1e-3): a recorded maximum above 1e-3 rejects the fixture --
tighten SPREAD or the inputs in gen_float_kat.py instead.  Integer outputs (RNG state after a sample call) must already be exact here.

Run:  python tests/golden/measure_float_kat.py   (after gen_float_kat.py)
"""
import datetime
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import float_kat_io as io, ref  # noqa: E402


def main():
    if not ref.available():
        sys.exit("oracle/_ref/libref.so cannot be built here (no reference tree)")
    kat = io.load()
    out = {"SPREAD": float(kat["SPREAD"]), "date": datetime.date.today().isoformat(), "measure": "max over kept states of |ref - f64| / (|f64| + 1e-6); unit vectors by absolute error",
           "functions": {}}
    for name in io.FUNCTIONS:
        got = io.run_side(ref.lib(), "ref", name, kat)
        err, seeds_ok = io.errors(name, kat, got)
        kept = kat[f"{name}_kept"]
        assert seeds_ok[kept].all(), f"{name}: the RNG state after the call differs from the model on a kept state"
        assert np.isfinite(err[kept]).all(), f"{name}: non-finite value on a kept state"
        worst = float(err[kept].max())
        assert worst <= 1e-3, f"{name}: recorded maximum {worst:.3g} exceeds the 1e-3 guard rail: tighten SPREAD or the inputs"
        gen, dropped = (int(x) for x in kat[f"{name}_counts"])
        out["functions"][name] = {"max_error": worst, "kept_incl_edges": int(kept.sum()), "edges": int(len(kat[f"{name}_edge_names"])), "generated": gen, "dropped": dropped}
        print(f"{name:18s} max {worst:.3e}  median {np.median(err[kept]):.2e}  kept {int(kept.sum())}")
    with open(os.path.join(HERE, "float_kat_tol.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
