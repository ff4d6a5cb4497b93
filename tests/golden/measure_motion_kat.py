"""Writes tests/golden/motion_kat_tol.json: what the host build of the motion of moving instances (tests/motion_host.py) shows against the model of
tests/golden/gen_motion_kat.py.

  worst_ratio   per case, the host build's largest error / bound over the kept pixels (out.rgb, Hn', fx, fy).  REPORTED: the tests apply the derived bound
                itself (tests/test_motion_model.py), never this figure.
  dropped       per case, the fraction of its pixels the model's own float32 and float64 runs drop (the cap of DESIGN.md section 5.3 is 0.05)

Run from the repository root:  python tests/golden/measure_motion_kat.py   (needs no libptmi.so)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import test_motion_model as T   # noqa: E402

mk = T.mk


def main():
    out = {"u": mk.U, "margin": mk.gen.MARGIN, "worst_ratio": {}, "dropped": {}}
    for size, move in T.CASES:
        inp, r = T.judged(size, move)
        new, pr = T.run_host(inp)
        worst, classes, exact = T.tmodel.ratios(inp, r, new, pr)
        assert classes and exact
        name = f"{size[0]}x{size[1]} {move}"
        out["worst_ratio"][name] = {k: round(v, 4) for k, v in worst.items()}
        out["dropped"][name] = round(float(1 - r["kept"].mean()), 4)
    with open(mk.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
