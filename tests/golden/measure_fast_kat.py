"""Writes tests/golden/fast_kat_tol.json: what the host build of the responsive history (tests/fast_host.py) shows against the model of
tests/golden/gen_fast_kat.py, and what the float64 model itself shows of the feature's purpose.

  worst_ratio   per case, the host build's largest error / bound over the kept pixels: mu, sigma, lo, hi and the clamped colour of the clamp, the colour
                and length of the long and the fast step against the imported models.  It must be below 1.  REPORTED: the tests apply the derived bound
                itself (tests/test_fast_model.py), never this figure.
  response      the float64 model's run of the switch (64 x 64, illumination 1 -> 3 after 32 calls, 25 % noise, maxHistory 32, maxFast 4, radius 2,
                sigmaScale 2): clamped RMSE / unclamped RMSE 8 calls after the switch (`ratio_after_8`: the host build has to stay below 1.25 x this
                and below 0.5), the same ratio at call 32 and the mean Hn' there.

Run from the repository root:  python tests/golden/measure_fast_kat.py   (needs no libptmi.so)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import test_fast_model as T   # noqa: E402

fk = T.fk


def main():
    out = {"u": fk.U, "margin": fk.MARGIN, "worst_ratio": {}}
    for demod in (False, True):
        tag = " demodulated" if demod else ""
        for size, move in T.SEQ_CASES:
            out["worst_ratio"][f"{size[0]}x{size[1]} {move}{tag} clamp"] = {k: round(v, 4) for k, v in T.check_clamp_meets_model(size, move, demod).items()}
        for size in T.SIZES:
            for move in ("none", "yaw"):
                out["worst_ratio"][f"{size[0]}x{size[1]} {move}{tag} steps"] = {k: round(v, 4) for k, v in T.check_fast_step_meets_model(size, move, demod).items()}
        for size, move in T.MOTION_CASES:
            out["worst_ratio"][f"{size[0]}x{size[1]} moving {move}{tag}"] = {k: round(v, 4) for k, v in T.check_moving_meets_model(size, move, demod).items()}
    out["worst"] = max(v for case in out["worst_ratio"].values() for v in case.values())
    assert out["worst"] < 1.0
    m = T.model_response()
    late, calm = m[T.SWITCH + T.AFTER - 1], m[T.SWITCH - 1]
    out["response"] = {"ratio_after_8": late[0] / late[1], "clamped_after_8": late[0], "unclamped_after_8": late[1], "ratio_at_32": calm[0] / calm[1],
                       "mean_length_at_32": calm[2]}
    with open(fk.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
