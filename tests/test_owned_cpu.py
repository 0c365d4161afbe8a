"""CPU: every wrapper class that owns device buffers refuses a device that is no GPU, in one wording (countr_amd/_owned.py)."""
import pytest

from countr_amd import _lib, _owned, cam, classes, device_aug, flow, frames, match, overlay, peaks, pretrain_aug, regions, tiles, tracks, yuv

WRAPPERS = [(tiles.TileStitcher, {}), (regions.RegionSummer, {}), (frames.FramePrep, {}), (classes.ClassFolder, {}),
            (flow.FlowCounter, {"lines": ()}), (tracks.Tracker, {"max_dist": 1.0}), (yuv.YuvConverter, {}), (peaks.PeakFinder, {}),
            (match.PointMatcher, {}), (overlay.Overlay, {}), (device_aug.DeviceAug, {}), (pretrain_aug.PretrainAug, {}),
            (cam.CameraEstimator, {})]


@pytest.mark.parametrize("cls,kwargs", WRAPPERS, ids=[c.__name__ for c, _k in WRAPPERS])
def test_a_wrapper_refuses_the_cpu_in_the_one_wording(cls, kwargs):
    import torch
    for device in ("cpu", torch.device("cpu")):
        with pytest.raises(_lib.CountrError) as e:
            cls(device, **kwargs)
        assert str(e.value) == "%s needs a GPU device: the HIP path has no CPU fallback" % cls.__name__


def test_the_rule_is_one_function():
    assert len(WRAPPERS) == 13
    with pytest.raises(_lib.CountrError) as e:
        _owned.resolve("cpu", "Anything")
    assert str(e.value) == "Anything needs a GPU device: the HIP path has no CPU fallback"
