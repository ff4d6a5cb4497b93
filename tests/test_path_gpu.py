"""The device's path loop against the fixture of tests/golden/gen_path_kat.py (see tests/test_path_model.py): all 63 images of 46 x 30 pixels (the 24 of sky3 and sky0 with sun & sky in use) rendered by the
default launch policy (k_tail at this size) and by the staged chain k_generate -> k_closest_* -> k_shade -> k_shadow_p -> k_accumulate (PT_TUNE tail=0), flat and
two-level.  Every image is bit-identical to the product's host build on every pixel and within the model's bound (4 x the compiled reference's recorded error)
on the kept pixels.  Only the committed fixture is read here; the model does not run."""
import pytest

from tests import path_kat_io as io
from vk_raytrace_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def host_out(kat):
    out = {}
    for two in (0, 1):
        out[two] = dict(io.render_all(kat, io.host(two)))
        for v in out[two].values():
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL], ids=["flat", "two-level"])
@pytest.mark.parametrize("tune", [None, "tail=0"], ids=["default policy", "staged chain"])
def test_device_frames_equal_the_host_build_and_meet_the_model(kat, host_out, tune, accel):
    tol = io.tolerances()
    got, staged = io.device_images(kat, accel, tune)
    for cn in kat["config_names"]:
        depth = int(kat["cfg_" + str(cn)][3])
        # k_tail from bounce 0 (a sequence still counts the bounce it hands over at) against every bounce in the staged kernels.  Not asserted for maxDepth 0,
        # where neither route traces a bounce, nor per debug frame (same context, same policy: see device_images)
        if depth >= 2:
            assert staged[str(cn)] == (1 if tune is None else depth), (str(cn), tune, staged[str(cn)])
    assert set(got) == {str(n) for n in kat["image_names"]}
    want = host_out[1 if accel == capi.PT_ACCEL_TWO_LEVEL else 0]
    for name, img in got.items():
        assert io.same_bits(img, want[name]), f"{name}: the device differs from the host build"
        io.check(kat, tol, name, img)
