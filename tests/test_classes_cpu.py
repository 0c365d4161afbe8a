"""CPU: the fold rule restated in numpy (countr_amd.classes_host) and the forward batches that count_classes shares between classes
(inference.image_chunks, inference.class_batches)."""
import numpy as np

import countr_amd
from countr_amd import inference
from countr_amd.classes import NONE, classes_host


def maps_of(nc, h, w, seed):
    return [m for m in np.random.RandomState(seed).uniform(-0.5, 1.0, (nc, h, w)).astype(np.float32)]


def test_exports():
    assert countr_amd.classes_host is classes_host and NONE == 255
    assert countr_amd.ClassCounts._fields == ("names", "counts", "maps", "labels", "won", "total", "area")


def test_ties_go_to_the_lowest_index():
    m = maps_of(4, 6, 9, 1)
    m[3][2, :] = 2.0
    m[1][2, :] = 2.0               # classes 1 and 3 tie on row 2: 1 owns it
    m[2][4, :5] = 4.0
    m[0][4, :5] = 2.0              # scaled by 2: a tie of v, not of the maps
    labels, won, total, area = classes_host(m, [2.0, 1.0, 1.0, 1.0], floor=0.0)
    assert (labels[2] == 1).all() and (labels[4, :5] == 0).all()
    same = [np.full((3, 3), 0.25, np.float32)] * 5
    labels, won, total, area = classes_host(same, [1.0] * 5)
    assert (labels == 0).all() and area.tolist() == [9, 0, 0, 0, 0] and won.tolist() == [2.25, 0, 0, 0, 0] and total.tolist() == [2.25] * 5


def test_at_or_below_the_floor_is_nobody_and_the_areas_partition_the_map():
    m = maps_of(3, 7, 11, 2)
    floor = 0.375                  # (exact in float32)
    for k in range(3):
        m[k][:2] = np.minimum(m[k][:2], 0.375)
    m[1][0, 0] = 0.375             # the maximum equals the floor: still nobody
    labels, won, total, area = classes_host(m, [1.0, 1.0, 1.0], floor)
    v = np.stack(m)
    assert (labels[:2] == NONE).all() and labels[0, 0] == NONE
    assert ((labels == NONE) == (v.max(axis=0) <= np.float32(floor))).all() and (labels != NONE).any()
    assert area.sum() + (labels == NONE).sum() == 7 * 11
    assert labels.dtype == np.uint8 and area.dtype == np.int64 and won.dtype == total.dtype == np.float64
    # everything below the floor: nobody anywhere, nothing won, the totals stay
    labels, won, total, area = classes_host(m, [1.0, 1.0, 1.0], floor=5.0)
    assert (labels == NONE).all() and not won.any() and not area.any() and np.allclose(total, v.reshape(3, -1).astype(np.float64).sum(1))


def test_one_class_above_the_floor_wins_everything():
    m = maps_of(1, 5, 7, 3)
    labels, won, total, area, won_abs, total_abs = classes_host(m, [0.5], floor=-1.0, members=True)
    assert (labels == 0).all() and area.tolist() == [35] and won[0] == total[0] and won_abs[0] == total_abs[0]
    assert total[0] == (np.float32(0.5) * m[0]).astype(np.float64).sum()


def test_the_product_is_rounded_to_float32_before_it_is_compared():
    # 3 * (1/3 rounded) rounds to 1.0 in float32 but not in float64: a tie with a plain 1.0, so class 0 owns the pixel
    third = np.float32(1.0) / np.float32(3.0)
    labels, _won, _total, _area = classes_host([np.full((1, 1), 1.0, np.float32), np.full((1, 1), third, np.float32)], [1.0, 3.0])
    assert np.float32(3.0) * third == np.float32(1.0) and 3.0 * float(third) != 1.0 and labels[0, 0] == 0


def test_chunks_of_count_images():
    """Derived by hand from window_starts: a 384-wide image has 1 window, 576 -> 3 (0, 128, 192), 672 -> 4 (0, 128, 256, 288: a 1080p
    frame), 960 -> 6 (0, 128, ..., 512, 576), 192 -> none.  A chunk takes images while their windows fit max_batch; an image with more
    windows than that is a chunk of its own."""
    assert [len(inference.window_starts(w)) for w in (384, 576, 672, 960, 192)] == [1, 3, 4, 6, 0]
    assert inference.window_starts(576) == [0, 128, 192] and inference.window_starts(672) == [0, 128, 256, 288]
    assert inference.image_chunks([672] * 9, 32) == [[0, 1, 2, 3, 4, 5, 6, 7], [8]]          # 8 x 4 = 32 windows, then one frame
    assert inference.image_chunks([576, 960], 32) == [[0, 1]]                                # 9 windows
    assert inference.image_chunks([576, 960, 384], 8) == [[0], [1, 2]]                       # 3 + 6 > 8; 6 + 1 <= 8
    assert inference.image_chunks([192, 672, 192], 4) == [[0, 1, 2]]                         # images without windows cost nothing
    assert inference.image_chunks([960, 384, 960], 4) == [[0], [1], [2]]                     # 6 > 4: on its own; 1 + 6 > 4
    assert inference.image_chunks([], 32) == []


def test_classes_with_the_same_paths_share_their_window_lists():
    widths = [576, 960]            # the two frames of the GPU test: 3 and 6 windows
    a = inference.class_batches(widths, [3, 3], [False, False], 32)
    b = inference.class_batches(widths, [3, 3], [False, False], 32)
    one = inference.class_batches(widths, [1, 1], [False, False], 32)
    zero = inference.class_batches(widths, [0, 0], [False, False], 32)
    key = lambda batches: [(w, nb) for _S, _v, w, nb in batches]
    assert key(a) == key(b) == key(one) == key(zero)                     # the shot count is not part of a forward batch's identity
    (S, variants, windows, nb), = a
    assert S == 3 and variants == [(0, -1), (1, -1)] and nb == 16
    assert windows == [((0, -1), s) for s in (0, 128, 192)] + [((1, -1), s) for s in (0, 128, 256, 384, 512, 576)]
    # frame 0 on the 3 x 3 split: nine crops of its own width in a batch of 32, and frame 1 alone in a batch of 8
    split = inference.class_batches(widths, [3, 3], [True, False], 32)
    assert [(S, nb, len(w)) for S, _v, w, nb in split] == [(3, 32, 27), (3, 8, 6)]
    assert split[0][1] == [(0, k) for k in range(9)] and split[0][2][:4] == [((0, 0), 0), ((0, 0), 128), ((0, 0), 192), ((0, 1), 0)]
    assert split[1][2] == [((1, -1), s) for s in (0, 128, 256, 384, 512, 576)]
    assert not set(map(str, key(split))) & set(map(str, key(a)))
    # frames of different shot counts of one class are different batches; what does not fit one forward has no bucket
    mixed = inference.class_batches(widths, [3, 0], [False, False], 32)
    assert [(S, v, nb) for S, v, _w, nb in mixed] == [(3, [(0, -1)], 4), (0, [(1, -1)], 8)]
    assert [nb for _S, _v, _w, nb in inference.class_batches([192, 960], [0, 0], [False, True], 32)] == [None, None]      # 54 windows; none
