"""CPU tests of the frame-size fields of the C ABI (v7): lcr_config.image_width / image_height default to 0 (= 320 x 240), and every
size the frame kernel cannot draw -- not a multiple of 4, outside [16, 512], one of the two left at zero -- is refused with LCR_ERR_INVALID and
the field's name in the message BEFORE any device is touched (so these run on a box without a GPU), whatever observation_mode is."""
import ctypes

import pytest

from gym_lowcostrobot_amd import _capi

BAD_SIZES = [(12, 64), (516, 64), (64, 12), (64, 516), (66, 64), (64, 66), (64, 0), (0, 64), (-4, 64)]   # (width, height)


def test_default_config_leaves_the_frame_size_at_zero(hip_lib):
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    for tid in _capi.TASKS.values():
        for preset in _capi.PRESETS.values():
            cfg = _capi.LcrConfig()
            assert hip_lib.lcr_config_preset(ctypes.byref(cfg), tid, preset) == 0
            assert cfg.image_width == 0 and cfg.image_height == 0
        cfg = _capi.LcrConfig()
        assert hip_lib.lcr_config_default(ctypes.byref(cfg), tid) == 0
        assert cfg.image_width == 0 and cfg.image_height == 0
    assert (_capi.IMG_H, _capi.IMG_W) == (240, 320)
    assert [n for n, _ in _capi.LcrObsView._fields_][-2:] == ["image_width", "image_height"]


@pytest.mark.parametrize("obs_mode", ["both", "image", "state"])
@pytest.mark.parametrize("width,height", BAD_SIZES)
def test_bad_frame_sizes_are_refused_before_any_device_is_touched(hip_lib, width, height, obs_mode):
    cfg = _capi.LcrConfig()
    hip_lib.lcr_config_default(ctypes.byref(cfg), _capi.TASKS["reach"])
    cfg.n_envs = 4
    cfg.obs_mode = _capi.OBS_MODES[obs_mode]
    cfg.image_width, cfg.image_height = width, height
    h = ctypes.c_void_p()
    assert hip_lib.lcr_create(ctypes.byref(cfg), ctypes.byref(h)) == _capi.LCR_ERR_INVALID
    assert not h.value
    msg = hip_lib.lcr_last_error()
    # the field at fault is named: the width for a bad width, the height for a bad height, (one of) both when only one of them is zero
    if (width == 0) != (height == 0):
        assert b"image_width" in msg or b"image_height" in msg, msg
    elif width in (12, 516, 66, -4):
        assert b"image_width" in msg, msg
    else:
        assert b"image_height" in msg, msg


def test_vecsim_refuses_a_bad_image_size_before_device_use(hip_lib):
    from gym_lowcostrobot_amd import VecSim

    with pytest.raises(ValueError, match="image_width"):
        VecSim("reach", 4, image_size=(64, 66))            # (height, width): the width is not a multiple of 4
    with pytest.raises(ValueError, match="image_height"):
        VecSim("reach", 4, observation_mode="both", image_size=(600, 64))
    with pytest.raises(ValueError, match="image_size"):
        VecSim("reach", 4, image_size=64)                  # not a (height, width) pair
    with pytest.raises(ValueError, match="image_size"):
        VecSim("reach", 4, image_size=(64, 64, 3))
