"""Writes tests/golden/chain_kat_tol.json: what tests/test_chain_host.py measures on the CPU host builds -- the worst ratio of |sum t - t_mirrored| to its
derived bound on the planar-mirror pixels, and the ghosting and blur errors on the mirror's pixels with chain guides and with first-hit guides (DESIGN.md
section 5.8).  Run from the repository's root: python -m tests.golden.measure_chain_kat"""
import json

from tests import test_chain_host as t


def main():
    err, bound, n, other = t.planar_mirror_bound()
    out = {"planar_mirror": {"pixels": n, "silhouette_pixels": other, "worst_abs_difference": float(err.max()), "worst_bound": float(bound.max()),
                             "worst_ratio": float((err / bound).max())}}
    out.update(t.measure_what_it_buys())
    with open(t.TOL_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
