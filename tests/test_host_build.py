"""The host builds of the four stage headers (tests/denoise_host.py, temporal_host.py, svgf_host.py, guides_host.py) go through the one build of
tests/host_harness.py: the dependency list recorded next to each library names the unit and the headers the compiler really read, a second build()
leaves the file alone, a library older than what it was made of is compiled again, and none of it needs libptmi.so."""
import os

import pytest

from tests import denoise_host, guides_host, host_harness as hh, svgf_host, temporal_host
from vk_raytrace_amd import capi

CSRC, CPP = "vk_raytrace_amd/csrc/", "tests/cpp/"
API = ["include/pt_fpmath.h", "include/pt_types.h", "include/pt_api.h"]
STAGES = {
    "denoise": (denoise_host, [CPP + "denoise_host.cpp", CPP + "stage/stage_host_common.h", CSRC + "pt_denoise.h"] + API),
    "temporal": (temporal_host, [CPP + "temporal_host.cpp", CPP + "stage/stage_host_common.h", CSRC + "pt_temporal.h", CSRC + "pt_denoise.h"] + API),
    "svgf": (svgf_host, [CPP + "svgf_host.cpp", CPP + "stage/stage_host_common.h", CSRC + "pt_svgf.h", CSRC + "pt_temporal.h", CSRC + "pt_denoise.h"] + API),
    "guides": (guides_host, [CPP + "guides_host.cpp", CPP + "th_scene.h", CSRC + "pt_guides.h", CSRC + "pt_shade.h"] + API),
}


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_the_stage_library_follows_what_it_was_made_of(stage, monkeypatch):
    module, reads = STAGES[stage]

    def no_product_library():
        raise AssertionError("a stage library asked for libptmi.so")
    monkeypatch.setattr(capi, "lib", no_product_library)
    path = module.build()
    assert os.path.dirname(path) == hh.BUILD_DIR
    deps = hh.deps(path)
    assert set(reads) <= set(deps), sorted(set(reads) - set(deps))
    assert all(os.path.isfile(os.path.join(hh.ROOT, d)) and not os.path.isabs(d) for d in deps)
    # up to date: not touched
    stamp = os.stat(path).st_mtime_ns
    assert module.build() == path and os.stat(path).st_mtime_ns == stamp
    # older than what it was made of: compiled again
    os.utime(path, (1, 1))
    assert module.build() == path
    assert os.path.getmtime(path) >= max(os.path.getmtime(os.path.join(hh.ROOT, d)) for d in deps)
    assert hh.deps(path) == deps
    module.bind(path)          # every name of the module's table resolves
