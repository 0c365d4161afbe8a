"""What counting a 4K frame from its own pixels costs: mae_vit_base_patch16 in bf16 (randomly initialised), one synthetic 3840 x 2160
uint8 frame on the device, three exemplar boxes, zoom 1 / 2 / 3, every call synchronised; the median wall time per call of

  1  count_frames(zoom=k)            resize to height 384 k, exemplars, tiles gathered into the forward's batch, forwards, the stitch
                                     with its sums (csrc_tiles/tiles.hip)
  2  the composition                 the same result from existing functions: FramePrep at that height, the band images sliced and
                                     made contiguous, inference.density_maps over them, inference.blend_windows over the transposed
                                     band maps, the sums as torch ops with one .item() each (inference._normalise)
  3  gather + stitch alone           the frame's countr_tile_gather launches and TileStitcher.stitch on the tile maps of the last call

in this process and this run.  Before anything is timed the maps of 1 and 2 must be equal bit for bit.  At zoom 1 row 1 is the existing
path and there is nothing to compose or stitch.  No threshold: the file records what was measured.

    python tools/bench_zoom.py [--calls 30] [--warmup 5] [--out profiles/zoom.txt] [--head <commit>]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import models_mae_cross
from bench_report import head, median_ms
from countr_amd import count_frames, frames as FR, inference, tile_starts
from countr_amd.tiles import tile_stitcher

H, W = 2160, 3840
BOXES = [(400, 300, 549, 449), (1800, 900, 1949, 1049), (3000, 1500, 3149, 1649)]      # 150 px: 26 px at zoom 1, the plain path


def composed(model, frame, k, max_batch=32):
    """(count, map) at zoom k from existing functions."""
    im = FR.frame_prep("cuda").prepare([frame], 384 * k)[0]
    hk, wk = im.shape[-2:]
    ex, rects = FR.exemplars(im, BOXES, W, H, 384 * k)
    rows = tile_starts(hk, 128)
    bands = [im[:, :, r:r + 384, :].contiguous() for r in rows]
    maps = inference.density_maps(model, bands, [ex] * len(rows), 3, max_batch)
    dm = inference.blend_windows(torch.stack(maps).transpose(1, 2), rows, hk, wk).t().contiguous()
    return inference._normalise((dm.sum() / 60).item(), dm, rects, True), dm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    model = models_mae_cross.__dict__["mae_vit_base_patch16"](norm_pix_loss="store_true", precision="bf16").to("cuda").eval()
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
    lines = ["zoom: HEAD %s, %s" % (args.head or head(root), torch.cuda.get_device_name(0)),
             "mae_vit_base_patch16 bf16, one frame of %d x %d on the device, 3-shot, band_stride 128, max_batch 32; ms per call, median "
             "(min .. max) of %d synchronised calls after %d warm-ups" % (W, H, args.calls, args.warmup)]

    def synced(fn):
        def run():
            fn()
            torch.cuda.synchronize()
        return run

    for k in (1, 2, 3):
        (cnt, dm), = count_frames(model, [frame], [BOXES], zoom=k)
        hk, wk = dm.shape
        a = median_ms(synced(lambda: count_frames(model, [frame], [BOXES], zoom=k)), args.calls, args.warmup)
        if k == 1:
            lines.append("zoom 1: map %d x %d, %d windows in one row (the existing path)" % (hk, wk, len(inference.window_starts(wk))))
            lines.append("  1  %-28s %9.3f  (%.3f .. %.3f)" % (("count_frames(zoom=1)",) + a))
            continue
        want_cnt, want = composed(model, frame, k)
        if not torch.equal(dm, want):
            raise SystemExit("bench_zoom: count_frames(zoom=%d) and the composition differ on the map" % k)
        rows, cols = tile_starts(hk, 128), tile_starts(wk, 128)
        tiles = [(r, c) for r in rows for c in cols]
        b = median_ms(synced(lambda: composed(model, frame, k)), args.calls, args.warmup)
        # the tile kernels alone: this frame's gathers into a batch buffer, and the stitch of the tile maps the last call left
        st = tile_stitcher("cuda")
        im = FR.frame_prep("cuda").prepare([frame], 384 * k)[0]
        rects = FR.scale_boxes(BOXES, W, H, 384 * k)
        batch = torch.empty(32, 3, 384, 384, device="cuda")

        def kernels():
            for t0 in range(0, len(tiles), 32):
                st.gather(im, tiles[t0:t0 + 32], batch)
            st.stitch(rows, cols, hk, wk, rects)

        c = median_ms(synced(kernels), args.calls, args.warmup)
        moved = 2 * len(tiles) * 3 * 384 * 384 * 4 + (len(tiles) * 384 * 384 + hk * wk) * 4
        lines.append("zoom %d: map %d x %d, %d x %d = %d tiles in %d forwards (the two paths agree bit for bit on the map; counts %.6f and %.6f)"
                     % (k, hk, wk, len(rows), len(cols), len(tiles), -(-len(tiles) // 32), cnt, want_cnt))
        lines.append("  1  %-28s %9.3f  (%.3f .. %.3f)" % (("count_frames(zoom=%d)" % k,) + a))
        lines.append("  2  %-28s %9.3f  (%.3f .. %.3f)" % (("the composition",) + b))
        lines.append("  3  %-28s %9.3f  (%.3f .. %.3f)" % (("gather + stitch alone",) + c))
        lines.append("  2 / 1 = %.2f, 3 / 1 = %.1f %% of the call; row 3 moves at least %.1f MB (tiles read and written once, tile maps read once, "
                     "the map written once), launches, download and wait included" % (b[0] / a[0], 100 * c[0] / a[0], moved / 1e6))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
