"""Writes tests/golden/svgf_kat_tol.json: what the host build of vk_raytrace_amd/csrc/pt_svgf.h (tests/svgf_host.py) measures against the float64 model of
gen_svgf_kat.py -- per output the worst error over the model's bound across every case of tests/test_svgf_model.py, the share of pixels the model drops, and
the figures of the two tests that say what the stage is for.  Reported, not used: the tests apply the bound as it stands.

Run:  python tests/golden/measure_svgf_kat.py      (from the repository root, after gen_svgf_kat.py)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import svgf_host as sh, test_svgf_model as model  # noqa: E402

gen = model.gen


def main():
    worst, dropped = {}, 0.0
    for size, move in model.CASES:
        worst["moments"] = max(worst.get("moments", 0.0), model.check_moments(size, move))
        for k, v in model.check_filter(size, move).items():
            worst[k] = max(worst.get(k, 0.0), v)
        inp, _, hist = model.run_sequence(size, move)[-1]
        guides, prm = model.guides_of(inp), gen.params()
        dropped = max(dropped, 1 - gen.judge_variance0(hist.colour, hist.length, hist.moments, guides, prm)["kept"].mean())
        rc, v0, steps = sh.filter_history(hist, guides, model.svgf_params(prm))
        c, v = hist.colour, v0
        for i, (c2, v2) in enumerate(steps):
            dropped = max(dropped, 1 - gen.judge_iteration(c, v, guides, prm, i)["kept"].mean())
            c, v = c2, v2
    estimate = {}
    for calls in (8, 4):
        offs = []
        for seed in range(4):
            rng = np.random.default_rng(100 + seed)
            hist = model.static_history([model.grey(np.ones((64, 96)), 0.1 * rng.standard_normal((64, 96))) for _ in range(calls)])
            rc, v0 = sh.variance(hist.colour, hist.length, hist.moments, None, sh.params(1, min_temporal=3.5))
            offs.append(float(v0.mean() / (0.01 * (calls - 1) / calls) - 1))
        estimate[f"N={calls}"] = offs
    out = {"comment": "host build against the float64 model: worst error / bound per output over all cases of tests/test_svgf_model.py (<= 1 passes); measured, not used",
           "worst_error_over_bound": {k: round(v, 4) for k, v in sorted(worst.items())},
           "largest_share_of_pixels_dropped_V0_and_iterations": round(float(dropped), 5),
           "mean_V0_relative_to_sigma2_(N-1)/N_minus_1_four_seeds": estimate,
           "edge_scene_worst_rmse_share_of_the_unfiltered_history_three_seeds": round(model.check_the_filter_stops_at_the_edge(), 4)}
    with open(gen.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
