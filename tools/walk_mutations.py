"""The ten mutations of DESIGN.md section 3 ("What the walk promises"), each applied to a scratch copy of the product's headers -- never to the tree -- and run
against tests/test_walk_model.py: every one must fail the test named next to it (CPU only, the host build; a few minutes):

    python tools/walk_mutations.py [name ...]

A mutant is the host harness library (tests/host_harness.py: the units under tests/cpp/) compiled with the scratch directory searched before csrc/, linked like
the real one; a child process binds it in place of the harness library and runs the test file.  opaque_rule lives in pt_scene_records.cpp, which the harness
reaches through libptmi.so: the mutant compiles the mutated file into itself, where its own definition of pt_debug_scene_records is found first.  Prints, per
mutation, the tests that failed; exits non-zero if a mutation does not fail its named test."""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vk_raytrace_amd", "csrc")
TESTS = os.path.join(ROOT, "tests", "test_walk_model.py")
MUTATIONS = {   # name: (the test that must fail, [(file under csrc/, text, its replacement)])
    "ties_descending": ("test_query_host_build", [("pt_trace.h", "return ta < tb || (ta == tb && wa < wb);", "return ta < tb || (ta == tb && wa > wb);")]),
    "reject_ge": ("test_settle", [("pt_surface.h", "return !(rng_next(seed) > opacity);", "return !(rng_next(seed) >= opacity);")]),
    "mask_ge": ("test_settle", [("pt_surface.h", "(a > am.cutoff ? 1.0f : 0.0f)", "(a >= am.cutoff ? 1.0f : 0.0f)")]),
    "flip_ignored": ("test_query_host_build", [("pt_trace.h", "bool front = (flags & TRI_FLIP) ? (det < 0.0f) : (det > 0.0f);", "bool front = det > 0.0f;")]),
    "tmax_inclusive": ("test_query_host_build", [("pt_trace.h", "(MODE == TM_COUNT ? t <= tmax : t < tmax)", "(t <= tmax)")]),
    "rtx_seed_written": ("test_query_host_build", [("pt_settle.h", "  if(variant == PT_VARIANT_RTX)\n    seed = seed0;\n", ""),
                                                   ("pt_settle.h", "seed = variant == PT_VARIANT_RTX ? seed : s2;", "seed = s2;")]),
    "opaque_rule": ("test_settle", [("pt_scene_records.cpp", "if(mat.alphaMode == 0 || (mat.pbrBaseColorFactor[3] == 1.0f && mat.pbrBaseColorTexture == -1))", "if(mat.alphaMode == 0)")]),
    "opaque_draws": ("test_settle", [("pt_trace.h", "if(bslot != BVH_NONE && !((bw >> 29) & TRI_OPAQUE))\n    ++nDraw;", "if(bslot != BVH_NONE)\n    ++nDraw;")]),
    "zero_draw_ignored": ("test_settle", [("pt_trace.h", "    if(rng_next(seed) == 0.0f)\n      return false;\n", "    rng_next(seed);\n")]),
    "count_excludes_ties": ("test_settle", [("pt_trace.h", "if(t > 0.0f && key_less(t, w, tmax, wLimit))", "if(t > 0.0f && t < tmax)")]),
}


def build_mutant(scratch, extra_units):
    sys.path.insert(0, ROOT)
    from tests import host_harness as hh
    from vk_raytrace_amd import capi
    capi.lib()
    for name in os.listdir(CSRC):
        if name.endswith(".h") and not os.path.exists(os.path.join(scratch, name)):
            shutil.copy(os.path.join(CSRC, name), scratch)
    units = [os.path.join(hh.CPP, u) for u in hh.UNITS] + extra_units
    objs = []
    procs = []
    for u in units:
        o = os.path.join(scratch, os.path.basename(u) + ".o")
        objs.append(o)
        if u in extra_units:   # a host unit of the product's library: compiled as its Makefile compiles it (hipcc on a .cpp: nothing for the device in it)
            procs.append(subprocess.Popen(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "--offload-arch=gfx950", "-I" + scratch, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                                           "-c", u, "-o", o]))
        else:
            procs.append(subprocess.Popen(["g++", "-I" + scratch] + hh.COMPILE + ["-c", u, "-o", o]))
    assert all(p.wait() == 0 for p in procs), "a unit of the mutant did not compile"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    out = os.path.join(scratch, "libmutant.so")
    subprocess.check_call(["g++"] + objs + ["-shared", "-fopenmp", "-L" + lib_dir, "-l:libptmi.so", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def child(scratch):
    """pytest on the walk tests with the harness library taken from the mutant in `scratch`"""
    sys.path.insert(0, ROOT)
    import pytest
    from tests import host_harness as hh
    extra = [os.path.join(scratch, f) for f in os.listdir(scratch) if f.endswith(".cpp")]
    hh._libs[""] = hh.bind(build_mutant(scratch, extra), hh.SIGNATURES)
    return pytest.main(["-q", "--no-header", "-p", "no:cacheprovider", TESTS, "-k", "not generator and not broken_model and not oracle", "--tb=no", "-rf"])


def main(names):
    survived = []
    for name in names or list(MUTATIONS):
        must_fail, edits = MUTATIONS[name]
        scratch = tempfile.mkdtemp(prefix="walk_mutant_")
        try:
            for fname in {f for f, _, _ in edits}:
                text = open(os.path.join(CSRC, fname)).read()
                for f, old, new in edits:
                    if f == fname:
                        assert text.count(old) == 1, f"{name}: {fname} no longer holds {old!r} exactly once"
                        text = text.replace(old, new)
                with open(os.path.join(scratch, fname), "w") as out:
                    out.write(text)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scratch], capture_output=True, text=True)
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
        failed = sorted({line.split("::")[1].split("[")[0].split(" ")[0] for line in out.stdout.splitlines() if line.startswith("FAILED")})
        ok = must_fail in failed
        print(f"{name}: fails {', '.join(failed) if failed else 'NOTHING'}" + ("" if ok else f"  -- NOT {must_fail}\n" + out.stdout[-1500:] + out.stderr[-1500:]), flush=True)
        if not ok:
            survived.append(name)
    return 1 if survived else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        sys.exit(child(sys.argv[2]))
    sys.exit(main(sys.argv[1:]))
