"""Measures the tolerance of tests/test_surface_model.py against the reference's own shaders.

Runs oracle/_ref/libref.so (the reference's GetShadeState and GetMaterialsAndTextures compiled by oracle/ref_glue/; needs the reference tree, so this runs
where that library can be built) on the fixture scene of tests/golden/surface_kat.npz and writes, per output group, the maximum over the KEPT rows of
|ref - f64| / max(1, |f64|) into tests/golden/surface_kat_tol.json, next to the row counts and the date.  The test's bound for every leg is 4 x that
maximum; a group the reference reproduces exactly (a copied constant) is held to equality.  Guard rail (the project's parity bar, bench.py's per-pixel L2 of
1e-3): a recorded maximum above 1e-3 rejects the fixture.  Integer outputs must already be exact here.  Never taken from the product.

Run:  python tests/golden/measure_surface_kat.py   (after gen_surface_kat.py)
"""
import datetime
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import ref, surface_kat_io as io  # noqa: E402
from vk_raytrace_amd import synth  # noqa: E402


def main():
    if not ref.available():
        sys.exit("oracle/_ref/libref.so cannot be built here (no reference tree)")
    kat = io.load()
    r = ref.Reference(io.fixture_scene(kat), synth.procedural_sky(16, 8))
    got, rc = io.reference_probe(r, io.STATE, io.probe_rows(kat))
    assert rc == 0
    kept = kat["row_kept"]
    want = kat["want"].T
    for w in io.INT_WORDS:
        assert np.array_equal(io.values(got)[kept, w], want[kept, w]), f"integer word {w} differs from the model on a kept row"
    err = io.errors(kat, got)
    for name, e in err.items():
        assert e <= 1e-3, f"{name}: recorded maximum {e:.3g} exceeds the 1e-3 guard rail"
        print(f"{name:22s} max {e:.3e}")
    out = {"date": datetime.date.today().isoformat(), "measure": "max over kept rows of |ref - f64| / max(1, |f64|), per output group", "rows": int(len(kept)), "kept": int(kept.sum()),
           "edge": int((kat["row_edge"] != 0).sum()), "groups": err}
    with open(os.path.join(HERE, "surface_kat_tol.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
