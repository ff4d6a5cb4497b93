"""The eight mutations of DESIGN.md section 3.3, each applied to a scratch copy of vk_raytrace_amd/csrc/pt_gather.h -- never to the tree -- and run
against tests/test_gather_host.py: every one must fail the tests section 3.3 names (CPU, about a minute):

    python tools/gather_mutations.py [name ...]

A mutant is the one-unit library tests/cpp/gather_host.cpp compiled with the scratch directory searched first (tests/host_harness.py compile_to); a
child process binds its gh_* entry points in place of the host build's and runs the test file.  Prints, per mutation, the tests that failed; exits
non-zero if a mutation failed none.

A sample's path is path_step itself (one-sample query), so two of the issue's mutations are edits around it:
  draws_after   the draws made after the path instead of before it: the first sample's path starts from the point's seed (its direction comes from a
                copy of the stream), every path is followed by the two draws -- the last one too, so they show in the record's seed
  clamp_sum     the clamp applied to the sum instead of the sample: the sample's own clamp is switched off (threshold 3e38 in the one-sample query)
                and the HEMISPHERE sum is clamped once before the division"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vk_raytrace_amd", "csrc", "pt_gather.h")
TESTS = os.path.join(ROOT, "tests", "test_gather_host.py")
LUMA_CLAMP = ("{ const float lum = dot3(m, f3{0.212671f, 0.715160f, 0.072169f}); if(lum > fp.st.fireflyClampThreshold) m *= fp.st.fireflyClampThreshold / lum; }")
MUTATIONS = {   # name: [(text in pt_gather.h, its replacement)]
    "uniform_hemisphere": [("sample_cosine_hemisphere(r1, r2)", "sample_uniform_hemisphere(r1, r2)")],
    "origin_not_offset": [("G.P.o = offset_ray(p, G.N);", "G.P.o = p;")],
    "seed_not_chained": [("gather_start_sample<KIND>(fp, G, seed, rays);\n  return false;", "gather_start_sample<KIND>(fp, G, 12345u, rays);\n  return false;")],
    "draws_after": [("const float r1 = rng_next(seed), r2 = rng_next(seed);", "uint32_t s2 = seed; const float r1 = rng_next(s2), r2 = rng_next(s2); if(G.sample != 0) seed = s2;"),
                    ("const float4 tail = gather_tail(__float_as_uint(G.P.rayD.w), 0u, G.P.closestRays);",
                     "uint32_t se = __float_as_uint(G.P.rayD.w); rng_next(se); rng_next(se); const float4 tail = gather_tail(se, 0u, G.P.closestRays);")],
    "no_pi": [("(G.sum / S) * PT_PI;", "(G.sum / S);")],
    "two_pi": [("const float fourPi = 4.0f * PT_PI;", "const float fourPi = 2.0f * PT_PI;")],
    "y4_y7_swapped": [("Y[4] = 1.092548f * (d.x * d.y);", "Y[4] = 1.092548f * (d.x * d.z);"), ("Y[7] = 1.092548f * (d.x * d.z);", "Y[7] = 1.092548f * (d.x * d.y);")],
    "clamp_sum": [("one.st.maxSamples = 1;", "one.st.maxSamples = 1; one.st.fireflyClampThreshold = 3.0e38f;"),
                  ("const f3 e = (G.sum / S) * PT_PI;", "f3 m = G.sum; " + LUMA_CLAMP + " const f3 e = (m / S) * PT_PI;")],
}


def child(scratch):
    """pytest on the host tests with gh_* taken from the mutant in `scratch`"""
    sys.path.insert(0, ROOT)
    import pytest
    from tests import gather_host as gh, host_harness
    real = gh.lib()
    mutant = host_harness.bind(host_harness.compile_to(os.path.join(scratch, "libmutant.so"), "gather_host.cpp", scratch), gh.SIGNATURES)

    class Proxy:
        def __getattr__(self, name):
            return getattr(mutant if name.startswith("gh_") else real, name)

    gh._lib = Proxy()
    return pytest.main(["-q", "--no-header", "-p", "no:cacheprovider", TESTS, "-k", "not exports", "--tb=no", "-rf"])


def main(names):
    source, survived = open(HEADER).read(), []
    for name in names or list(MUTATIONS):
        text = source
        for old, new in MUTATIONS[name]:
            assert text.count(old) == 1, f"{name}: pt_gather.h no longer holds {old!r} exactly once"
            text = text.replace(old, new)
        scratch = tempfile.mkdtemp(prefix="gather_mutant_")
        try:
            with open(os.path.join(scratch, "pt_gather.h"), "w") as f:
                f.write(text)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scratch], capture_output=True, text=True)
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
        failed = sorted({line.split("::")[1].split("[")[0].split(" ")[0] for line in out.stdout.splitlines() if line.startswith("FAILED")})
        print(f"{name}: fails {', '.join(failed) if failed else 'NOTHING'}" + ("" if failed else "\n" + out.stdout[-1500:] + out.stderr[-1500:]))
        if not failed:
            survived.append(name)
    return 1 if survived else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        sys.exit(child(sys.argv[2]))
    sys.exit(main(sys.argv[1:]))
