"""The host builds of the stage headers (tests/denoise_host.py, temporal_host.py, svgf_host.py, motion_host.py, albedo_host.py, fast_host.py,
guides_host.py) go through the one build of tests/host_harness.py: the dependency list recorded next to each library names the unit and the headers the
compiler really read, a second build() leaves the file alone, a library older than what it was made of is compiled again, and none of it needs
libptmi.so.  The five history libraries lay HistoryCall (tests/cpp/stage/history_step.h) out as tests/history_host.py's Call says."""
import ctypes
import os

import pytest

from tests import albedo_host, denoise_host, fast_host, guides_host, history_host, host_harness as hh, motion_host, svgf_host, temporal_host
from vk_raytrace_amd import capi

CSRC, CPP = "vk_raytrace_amd/csrc/", "tests/cpp/"
API = ["include/pt_fpmath.h", "include/pt_types.h", "include/pt_api.h"]
STEP = [CPP + "stage/history_step.h", CPP + "stage/stage_host_common.h", CSRC + "pt_temporal.h", CSRC + "pt_denoise.h"] + API   # what every history library reads
HISTORY = {"temporal": temporal_host, "svgf": svgf_host, "motion": motion_host, "albedo": albedo_host, "fast": fast_host}
STAGES = {
    "denoise": (denoise_host, [CPP + "denoise_host.cpp", CPP + "stage/stage_host_common.h", CSRC + "pt_denoise.h"] + API),
    "temporal": (temporal_host, [CPP + "temporal_host.cpp"] + STEP),
    "svgf": (svgf_host, [CPP + "svgf_host.cpp", CSRC + "pt_svgf.h"] + STEP),
    "motion": (motion_host, [CPP + "motion_host.cpp", CSRC + "pt_motion.h", CSRC + "pt_guides.h"] + STEP),
    "albedo": (albedo_host, [CPP + "albedo_host.cpp", CSRC + "pt_albedo.h"] + STEP),
    "fast": (fast_host, [CPP + "fast_host.cpp", CSRC + "pt_fast.h"] + STEP),
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


@pytest.mark.parametrize("stage", sorted(HISTORY))
def test_the_call_record_is_laid_out_as_the_binding_says(stage):
    """hs_call_layout of each history library: sizeof(HistoryCall), then the offset of every field in declaration order, against ctypes' own layout of
    history_host.Call -- a field added, dropped or moved on one side only is a difference here, not a misread pointer in a test"""
    got = history_host.layout(HISTORY[stage].lib())
    fields = [name for name, _ in history_host.Call._fields_]
    assert got == [ctypes.sizeof(history_host.Call)] + [getattr(history_host.Call, name).offset for name in fields], (stage, got)
