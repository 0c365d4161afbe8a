"""CPU: the rule of include/countr_hip_cam.h as countr_amd/cam.py restates it -- hand-built fields with known answers, and the accuracy
of flow_host(camera="translation") on pan_scene clips, whose truth is known by construction."""
import functools

import numpy as np
import pytest

from countr_amd import cam, flow

R = cam.RANGE


def textured(h=32, w=64, seed=0):
    """A luma whose every cell is far above min_texture = 128."""
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def field_of(offsets, h=32, w=64, rest=(9999, 9999)):
    """A field whose first cells (row-major) hold `offsets`; the others hold `rest`, out of range by default: they do not vote."""
    V = np.empty((h // 8, w // 8, 2), np.int16)
    V[...] = rest
    flat = V.reshape(-1, 2)
    if len(offsets):
        flat[:len(offsets)] = offsets
    return V


def test_texture_is_the_sum_of_right_and_lower_differences_with_a_clamped_edge():
    L = np.zeros((8, 16), np.uint8)
    L[:, 7] = 10                                  # the last column of cell 0: |right - here| = 10 on columns 6 and 7, eight rows each
    T = cam.texture_host(L)
    assert T.dtype == np.uint32 and T.tolist() == [[160, 0]]
    L = np.zeros((16, 8), np.uint8)
    L[15, :] = 3                                  # the last row: a lower neighbour that is the row itself; the row above sees 3 per pixel
    assert cam.texture_host(L).tolist() == [[0], [24]]
    L = np.full((8, 8), 255, np.uint8)
    L[::2, ::2] = 0
    L[1::2, 1::2] = 0
    assert cam.texture_host(L)[0, 0] == 255 * (7 * 8 + 7 * 8)                      # the clamped column and row add nothing
    with pytest.raises(ValueError):
        cam.texture_host(np.zeros((8, 12), np.uint8))


def test_lower_median_of_an_even_and_an_odd_number_of_voters():
    L = textured()
    even = [(16 * k, -16 * k) for k in (1, 2, 3, 4)]                               # rank 2: x = 32; y ascending -64 -48 -32 -16: -48
    rec, flags = cam.estimate_host(field_of(even), L, tol=16, min_voters=4)
    assert rec.tolist() == [32, -48, 4, 2, 1, 32, 0, 0] and flags.all()  # (32, -32) and (48, -48) agree on both axes
    odd = even + [(80, -80)]                                                       # rank 3: x = 48, y = -48
    rec, _ = cam.estimate_host(field_of(odd), L, tol=16, min_voters=4)
    assert rec.tolist() == [48, -48, 5, 3, 1, 32, 0, 0]
    rec, _ = cam.estimate_host(field_of([(21, -5)] * 32), L)                       # all voters equal
    assert rec.tolist() == [21, -5, 32, 32, 1, 32, 0, 0]
    rec, _ = cam.estimate_host(field_of([]), L)                                    # nobody votes
    assert rec.tolist() == [0, 0, 0, 0, 0, 32, 0, 0]


def test_validity_at_half_the_inliers_and_at_min_voters():
    L = textured()
    # 16 voters: the median (rank 8) is 0; eight lie within tol = 8 and eight do not: 2 * inliers == n is valid
    half = [(0, 0)] * 8 + [(100 + 20 * k, 0) for k in range(8)]
    rec, _ = cam.estimate_host(field_of(half), L)
    assert rec.tolist() == [0, 0, 16, 8, 1, 32, 0, 0]
    # one inlier fewer: the median is still 0 (rank 8 of 16: seven zeros and -100 below them), seven of 16 agree: invalid, g = (0, 0)
    fewer = [(0, 0)] * 7 + [(-100, 0)] + [(100 + 20 * k, 0) for k in range(8)]
    rec, _ = cam.estimate_host(field_of(fewer), L)
    assert rec.tolist() == [0, 0, 16, 7, 0, 32, 0, 0]
    fewer[0] = (40, 0)                                                             # rank 8 is now 40 -- and g is still written as 0
    rec, _ = cam.estimate_host(field_of(sorted(fewer)), L, tol=0)
    assert rec[:5].tolist() == [0, 0, 16, 1, 0]
    # n == min_voters is valid, one fewer is not
    rec, _ = cam.estimate_host(field_of([(33, 7)] * 16), L)
    assert rec.tolist() == [33, 7, 16, 16, 1, 32, 0, 0]
    rec, _ = cam.estimate_host(field_of([(33, 7)] * 15), L)
    assert rec.tolist() == [0, 0, 15, 15, 0, 32, 0, 0]


def test_offsets_at_the_range_vote_and_one_beyond_does_not():
    L = textured()
    rec, _ = cam.estimate_host(field_of([(R, -R)] * 9 + [(-R, R)] * 8), L, tol=0, min_voters=1)
    assert rec.tolist() == [R, -R, 17, 9, 1, 32, 0, 0]
    rec, _ = cam.estimate_host(field_of([(R + 1, 0), (0, -R - 1), (-R - 1, 0), (0, R + 1), (32767, -32768), (5, 5)]), L, min_voters=1)
    assert rec.tolist() == [5, 5, 1, 1, 1, 32, 0, 0]


def test_flat_cells_do_not_vote_and_compensate_keeps_them_at_rest():
    L = textured()
    L[:9, :25] = 77                               # cells (0, 0), (0, 1) and (0, 2) are flat, their right and lower neighbours included
    T = cam.texture_host(L)
    assert T[0, :3].tolist() == [0, 0, 0] and T[0, 3] > 128 and T[1, 0] > 128
    V = field_of([(0, 0), (50, 50), (0, 0)] + [(20, -4)] * 29)
    rec, flags = cam.estimate_host(V, L)
    assert flags[0, :3].tolist() == [0, 0, 0] and flags.sum() == 29 and rec.tolist() == [20, -4, 29, 29, 1, 32, 0, 0]
    out = cam.compensate_host(V, rec, flags)
    assert out[0, 0].tolist() == [0, 0]           # flat and resting: it moves with the scene
    assert out[0, 1].tolist() == [30, 54]         # flat but moving: V - g
    assert out[0, 2].tolist() == [0, 0] and out[0, 3].tolist() == [0, 0]
    V[0, 3] = (0, 0)                              # textured and resting in the image: it moves against the scene
    rec, flags = cam.estimate_host(V, L)
    assert cam.compensate_host(V, rec, flags)[0, 3].tolist() == [-20, 4]


def test_compensate_saturates_to_int16():
    flags = np.ones((1, 4), np.uint8)
    V = np.array([[(-32768, 32767), (32767, -32768), (-32600, 32600), (0, 0)]], np.int16)
    rec = np.array([R, -R, 4, 4, 1, 4, 0, 0], np.int32)
    assert cam.compensate_host(V, rec, flags).tolist() == [[[-32768, 32767], [32767 - R, -32768 + R], [-32768, 32767], [-R, R]]]


def test_path_chains_follow_the_interval_and_a_lost_frame_adds_nothing():
    L = textured()
    lumas = [L] * 9
    g = [(16 * t, -t) for t in range(9)]
    whole = lambda t: field_of([g[t]] * 32)
    for s in (1, 4):
        fields = [None if t < s else whole(t) for t in range(9)]
        fields[6] = field_of([(g[6][0] + 40 * k, 0) for k in range(32)])             # frame 6 agrees on nothing: lost
        rec, path, comp = cam.camera_host(lumas, fields, interval=s)
        want = np.zeros((9, 2), np.int64)
        for t in range(s, 9):
            want[t] = want[t - s] + (g[t] if t != 6 else (0, 0))
        assert path.dtype == np.int64 and path.tolist() == want.tolist()
        assert rec[:s].tolist() == [[0] * 8] * s and rec[6, 4] == 0 and rec[6, :2].tolist() == [0, 0] and cam.lost_frames(rec) == 1
        assert comp[:s] == [None] * s and not comp[5].any() and (comp[6] == fields[6]).all()
    assert path[8].tolist() == [16 * (4 + 8), -(4 + 8)]                            # interval 4: the chain 0, 4, 8
    P = cam.CameraPath(path, cam.lost_frames(rec), rec)
    assert P.lost == 1 and P.position(8, (2.5, 0.75, 3.0, 1.0)).tolist() == [2.5 * 192 / 16, 3.0 * -12 / 16]
    assert cam.shifted_placement(path[8], (2.5, 0.75, 3.0, 1.0)) == (2.5, 0.75 + 2.5 * 192 / 16, 3.0, 1.0 + 3.0 * -12 / 16)


def test_settings_are_checked():
    assert cam.settings("translation") == (128, 8, 16) and cam.settings(None, 0, 0, 1) == (0, 0, 1)
    for bad in (dict(camera="affine"), dict(camera="translation", min_texture=-1), dict(camera=None, tol=1.5), dict(camera=None, min_voters=0)):
        with pytest.raises(ValueError):
            cam.settings(**bad)
    with pytest.raises(ValueError):
        flow.flow_host([], [], lines=(), camera="zoom")


# ---- accuracy on pan_scene: the issue's settings.  60 frames, speeds 1 .. 3 px/frame, search 6, band 8, three seeds
PANS = (((1.3, 0.4), 0.3), ((-2.2, 0.7), 0.5))
SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def clip(pan, jitter, seed, frames=60, interval=1, speed=(1.0, 3.0)):
    lumas, maps, lines, truth, c = cam.pan_scene(frames=frames, seed=seed, pan=pan, jitter=jitter, interval=interval, speed=speed)
    fields = [None if t < interval else flow.motion_host(lumas[t], lumas[t - interval], 6, 256) for t in range(frames)]
    kw = dict(lines=lines, search=6, interval=interval, band=8.0, fields=fields)
    _out, on, path = flow.flow_host(lumas, maps, camera="translation", **kw)
    _out, off = flow.flow_host(lumas, maps, **kw)
    return on.line_counts, off.line_counts, truth, np.abs(path.path / 16.0 - c).max(), path.lost


def off_by(counts, truth):
    """The worst entry's |count - truth| / truth."""
    return float((np.abs(counts - truth) / truth).max())


def test_panned_clips_are_counted_and_the_uncompensated_rule_loses_them():
    """Measured with the committed camera_host (worst entry off, as a fraction of its true count; every truth is [1, 2] x 3 lines):
        pan (1.3, 0.4) +- 0.3    seeds 0, 1, 2: 5.1 %, 6.5 %, 5.9 %       path drift 1.06, 0.60, 0.95 px      camera=None: 49.9 %, 61 %, 100 %
        pan (-2.2, 0.7) +- 0.5   seeds 0, 1, 2: 4.5 %, 6.3 %, 2.7 %       path drift 0.81, 0.54, 0.50 px      camera=None: 100 %, 100 %, 100 %
    The worst is 6.5 %, under the 10 % that would have meant a fault, so the bound is 1.5 x 6.5 % = 9.75 %.  (Before pan_scene kept
    objects from resting in the image -- its docstring, item 3 -- the worst was 15.6 %: a fault of the scene, found with the TRUE camera
    motion in place of the estimate.)  No estimate is lost, and the path stays within 2 px of the true one.  Without the camera every
    clip loses a count of 1 or 2 whole; the assertion is that each pan's clips miss some entry by more than 50 % (one clip of the six
    loses 0.998 of 2, a hair under)."""
    worst = 0.0
    for pan, jitter in PANS:
        missed = 0.0
        for seed in SEEDS:
            on, off, truth, drift, lost = clip(pan, jitter, seed)
            print("pan %r seed %d: on off by %.4f, camera=None off by %.4f, drift %.2f px, lost %d" % (pan, seed, off_by(on, truth), off_by(off, truth), drift, lost))
            worst = max(worst, off_by(on, truth))
            missed = max(missed, off_by(off, truth))
            assert off_by(off, truth) > 5 * 0.0975 and lost == 0 and drift < 2.0
        assert missed > 0.5                       # the evidence that the feature does something
    assert worst <= 0.0975, worst


def test_at_pan_zero_camera_on_and_off_give_identical_flux_sums():
    """Worst entry off at pan 0, seeds 0, 1, 2: 1.0 %, 1.2 %, 1.7 % -- with the camera on and off alike, because the sums are the same."""
    for seed in SEEDS:
        on, off, truth, drift, lost = clip((0.0, 0.0), 0.0, seed)
        assert (on == off).all() and drift == 0 and lost == 0
        assert off_by(on, truth) <= 0.0255                                         # 1.5 x 1.7 %


def test_slow_pan_at_interval_four():
    """Pan (0.3, -0.15), 120 frames, interval 4, object speeds 0.3 .. 1 px/frame (1 .. 3 would leave a search of 6 at interval 4).
    Measured, seeds 0, 1, 2: 10.8 %, 13.8 %, 4.3 % with the camera on.  That is over 10 %, and it is not the camera's: on the entries the
    pan leaves alone, camera=None misses by the same 6 .. 9 % on the same clips (slow objects at interval 4 are the flow rule's own
    error), and on the others it loses half of the count.  Bound: 1.5 x 13.8 % = 20.7 %."""
    for seed in SEEDS:
        on, off, truth, drift, lost = clip((0.3, -0.15), 0.0, seed, frames=120, interval=4, speed=(0.3, 1.0))
        print("slow pan seed %d: on off by %.4f, camera=None off by %.4f, drift %.2f px" % (seed, off_by(on, truth), off_by(off, truth), drift))
        assert off_by(on, truth) <= 0.207 and off_by(off, truth) > 0.3 and lost == 0
