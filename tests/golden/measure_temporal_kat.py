"""Writes tests/golden/temporal_kat_tol.json: what the host build of the temporal stage (tests/temporal_host.py) shows against the model of
tests/golden/gen_temporal_kat.py.

  worst_ratio        per case, the host build's largest error / bound over the kept pixels (out.rgb, Hn', fx, fy).  REPORTED: the tests apply the derived bound
                     itself (tests/test_temporal_model.py), never this figure.
  convention_spread  per move, the larger of the model's float32 and float64 residuals of "the previous camera's ray through (fx, fy) passes through P" plus their
                     difference: the spread the two runs show on that quantity.  test_conventions_through_the_previous_camera allows the host build 4 x this.
  identity_defect    worldToClip (viewInverse projInverse) against the identity over the fixture's cameras (pt_camera_world_to_clip against pt_camera_lookat):
                     relative to the size of the terms each entry sums (the test's limit is 1e-6), as it stands, and the helper against a float64 proj view.

Run from the repository root, after gen_temporal_kat.py:  python tests/golden/measure_temporal_kat.py   (needs libptmi.so for the two camera helpers)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import test_temporal_model as T   # noqa: E402

gen = T.gen


def main():
    out = {"u": gen.U, "margin": gen.MARGIN, "worst_ratio": {}, "convention_spread": {}}
    for size, move in T.CASES:
        inp, r = T.judged(size, move)
        new, pr = T.run_host(inp)
        worst, classes, exact = T.ratios(inp, r, new, pr)
        assert classes and exact
        out["worst_ratio"][f"{size[0]}x{size[1]} {move}"] = {k: round(v, 4) for k, v in worst.items()}
    for move in T.CONVENTION_MOVES:
        r32, r64 = T.convention_residual((96, 64), move, "f32"), T.convention_residual((96, 64), move, "f64")
        out["convention_spread"][move] = max(r32, r64) + abs(r32 - r64)
    out["identity_defect"] = dict(zip(("relative_to_terms", "absolute", "helper_against_float64"), T.identity_defect((96, 64))))
    with open(gen.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
