"""Writes tests/golden/albedo_kat_tol.json: what the host build of the demodulated history (tests/albedo_host.py) shows against the model of
tests/golden/gen_albedo_kat.py.

  worst_ratio   per case, the host build's largest error / bound over the kept pixels: the step's colour, length and moments over the sequence, the moving
                step's colour and length, and the filtered and remodulated image.  It must be below 1.  REPORTED: the tests apply the derived bound itself
                (tests/test_albedo_model.py), never this figure.

Run from the repository root:  python tests/golden/measure_albedo_kat.py   (needs no libptmi.so)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import test_albedo_model as T   # noqa: E402

ak = T.ak


def main():
    out = {"u": ak.U, "margin": ak.tk.MARGIN, "worst_ratio": {}}
    for size, move in T.SEQ_CASES:
        out["worst_ratio"][f"{size[0]}x{size[1]} {move}"] = {k: round(v, 4) for k, v in T.check_step_meets_model(size, move).items()}
    for size, move in T.MOTION_CASES:
        out["worst_ratio"][f"{size[0]}x{size[1]} moving {move}"] = {k: round(v, 4) for k, v in T.check_moving_step_meets_model(size, move).items()}
    for size in T.SIZES:
        for move in ("none", "yaw", "disocclude"):
            out["worst_ratio"][f"{size[0]}x{size[1]} {move} filtered"] = {"remodulated": round(T.check_filtered_and_remodulated_meets_model(size, move), 4)}
    out["worst"] = max(v for case in out["worst_ratio"].values() for v in case.values())
    assert out["worst"] < 1.0
    with open(ak.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
