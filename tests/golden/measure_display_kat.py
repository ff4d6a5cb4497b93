"""Measures the tolerance of tests/test_display_model.py against the reference's own display shader.

Runs oracle/_ref/libref.so (shaders/post.frag compiled by oracle/ref_glue/; needs the reference tree, so this runs where that library can be built) on every
run of tests/golden/display_kat.npz and writes, per tonemapper case, the maximum over the KEPT pixels of |ref - model| / (|model| + 1e-6) into
tests/golden/display_kat_tol.json, next to SPREAD and the pixel counts (the 5 % cap is about these).  The test's bound for every leg is 4 x that maximum.
Guard rail (the project's parity bar, 1e-3): a recorded maximum above it rejects the fixture -- tighten the inputs in gen_display_kat.py instead.  A case
whose kept pixels all come out exact (a dithered output is a multiple of 1 / 255 on every side) records the float32 resolution 2^-24 instead of 0.
The file holds no date: running this again reproduces it byte for byte.

Run:  python tests/golden/measure_display_kat.py   (after gen_display_kat.py)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import display_kat_io as io, ref  # noqa: E402


def main():
    if not ref.available():
        sys.exit("oracle/_ref/libref.so cannot be built here (no reference tree)")
    kat = io.load()
    out = {"SPREAD": float(kat["SPREAD"]), "measure": "max over kept pixels of |ref - f64| / (|f64| + 1e-6), worst channel", "cases": {}}
    for run in io.runs(kat):
        err = io.gen.measure(io.ref_tonemap(run), run.frag)
        assert np.isfinite(err[run.kept]).all(), f"{run.label}: a kept pixel is NaN or infinite on one side only"
        c = out["cases"].setdefault(run.case, {"max_error": 2.0 ** -24, "pixels": 0, "dropped": 0, "round_only": 0})
        c["max_error"] = max(c["max_error"], float(err[run.kept].max()) if run.kept.any() else 0.0)
        c["pixels"] += int(run.kept.size)
        c["dropped"] += int((~run.kept).sum())
        c["round_only"] += int(run.round_only.sum())
    for case, c in out["cases"].items():
        assert c["max_error"] <= 1e-3, f"{case}: recorded maximum {c['max_error']:.3g} exceeds the 1e-3 guard rail: tighten the inputs"
        print(f"{case:12s} max {c['max_error']:.3e}  pixels {c['pixels']}  dropped {c['dropped']}")
    with open(os.path.join(HERE, "display_kat_tol.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
