"""GPU: what the wrapper classes share (countr_amd/_owned.py) -- one instance per resolved device, buffers that only grow and their
pinned twins, and the guard of a call from another stream in its two forms."""
import types

import pytest
import torch

from countr_amd import _owned

pytestmark = pytest.mark.gpu
SLEEP = 2_000_000           # cycles of torch.cuda._sleep: milliseconds, far longer than the gap between two launches


def test_an_accessor_gives_one_object_per_resolved_device(hip):
    from countr_amd import carpk, classes, frames, match, overlay, peaks, regions, tiles
    assert torch.cuda.current_device() == 0
    accessors = [(peaks.peak_finder, peaks.PeakFinder), (match.point_matcher, match.PointMatcher),
                 (regions.region_summer, regions.RegionSummer), (classes.class_folder, classes.ClassFolder),
                 (tiles.tile_stitcher, tiles.TileStitcher), (overlay.overlay_for, overlay.Overlay), (frames.frame_prep, frames.FramePrep),
                 (carpk.carpk_prep, carpk.CarpkPrep)]
    for accessor, cls in accessors:
        a, b, c = accessor("cuda"), accessor("cuda:0"), accessor(torch.device("cuda", 0))
        assert a is b and b is c and type(a) is cls and a.device == torch.device("cuda", 0), cls.__name__
    assert frames.frame_prep("cuda") is not carpk.carpk_prep("cuda")           # (a subclass has an instance of its own)


@pytest.mark.parametrize("pinned", [True, False])
def test_grow_never_shrinks_and_makes_exactly_what_is_asked(hip, pinned):
    owner = types.SimpleNamespace(device=torch.device("cuda", 0), _buf=None, _buf_host=None)
    ptrs = lambda: (owner._buf.data_ptr(), owner._buf_host.data_ptr() if pinned else None)
    with torch.cuda.device(owner.device):
        assert _owned.grow(owner, "_buf", 100, torch.int32, pinned=pinned) is owner._buf
        first = ptrs()
        assert _owned.grow(owner, "_buf", 50, torch.int32, pinned=pinned) is owner._buf
        assert ptrs() == first and owner._buf.numel() == 100
        keep = (owner._buf, owner._buf_host)           # (alive, so that the allocator cannot hand the same addresses out again)
        assert _owned.grow(owner, "_buf", 200, torch.int32, pinned=pinned) is owner._buf
    assert owner._buf.numel() == 200 and owner._buf.dtype == torch.int32 and owner._buf.device == owner.device
    assert owner._buf.data_ptr() != first[0] and keep[0].numel() == 100
    if pinned:
        assert owner._buf_host.numel() == 200 and owner._buf_host.dtype == torch.int32 and owner._buf_host.is_pinned()
        assert owner._buf_host.data_ptr() != first[1]
    else:
        assert owner._buf_host is None


def _second_stream_reads_what_the_first_wrote(guard, buf):
    """The guard's stream holds a sleep and then the fill of buf with ones; a call on another stream waits for it and reads ones."""
    host = torch.zeros(64).pin_memory()
    second = torch.cuda.Stream()
    with torch.cuda.stream(second):
        cur = guard.enter()
        assert cur == second
        host.copy_(buf, non_blocking=True)
        guard.leave(cur)
    second.synchronize()
    assert guard.last == second and host.tolist() == [1.0] * 64


def test_guard_lazy_form(hip):
    dev = torch.device("cuda", 0)
    buf = torch.zeros(64, device=dev)
    torch.cuda.synchronize()
    guard = _owned.Guard(dev)
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(other):                     # before any leave: nothing is recorded, so nothing is waited for
        assert guard.last is None and guard.enter() == other and guard.last is None
    with torch.cuda.stream(side):
        cur = guard.enter()
        assert cur == side
        torch.cuda._sleep(SLEEP)
        buf.fill_(1)
        guard.leave(cur)
    assert guard.last == side
    _second_stream_reads_what_the_first_wrote(guard, buf)


def test_guard_recorded_at_construction(hip):
    dev = torch.device("cuda", 0)
    buf = torch.zeros(64, device=dev)
    torch.cuda.synchronize()
    made_on = torch.cuda.Stream()
    with torch.cuda.device(dev), torch.cuda.stream(made_on):
        torch.cuda._sleep(SLEEP)
        buf.fill_(1)                                   # the constructor's fill of device state
        guard = _owned.Guard(dev, recorded=True)
    assert guard.last == made_on
    _second_stream_reads_what_the_first_wrote(guard, buf)
