"""Measures tests/golden/accel_audit_tol.json on a GPU: cost(device structure) / cost(harness structure) per builder, scene and hierarchy
(tests/test_accel_audit_gpu.py cost_ratios), with the margin m that test_tree_quality_matches_the_emulation asserts for sahdev and sah.
m = 1e-3 is the bound tests/test_sah_cpu.py holds between the emulation and the host builder; the ratios of ploc and lbvh are recorded only.

    python tests/golden/measure_accel_audit.py [output.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.test_accel_audit_gpu import BUILDERS, TOL_FILE, cost_ratios  # noqa: E402

M = 1e-3


def main(out):
    ratios = {b: {name: cost_ratios(b, name) for name in ("soup5000", "forest")} for b in BUILDERS}
    worst = max(v for b in ("sahdev", "sah") for per in ratios[b].values() for v in per.values())
    doc = {"m": M, "asserted": ["sahdev", "sah"], "worst_asserted_ratio": worst, "ratios": ratios}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"worst asserted ratio {worst!r}, m = {M}; written to {out}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else TOL_FILE)
