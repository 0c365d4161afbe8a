"""Sliding-window inference around SupervisedMAE.forward.

Reference behaviour: FSC_test_cross(few-shot).py:264-359 and demo_zero.py:41-74 -- images are resized to height 384,
the width is covered by 384-px windows with stride 128 (last window snapped to w-384), overlapping columns are blended
sequentially (previously covered columns: 1/2 old + 1/2 new), count = sum/60, optional 3x3 crop-and-upscale for tiny
exemplars and test-time normalisation by the mean exemplar-box count.  Images narrower than 384 give an all-zero map
(the reference's loop never runs).  Every window is an independent forward, so all windows (of all crops) go through
the engine as ONE batch -- the stitching itself is a few elementwise ops on [384, w].
"""
import torch
import torch.nn.functional as F

from . import _lib


def window_starts(width):
    """Start columns produced by the reference loop (FSC_test_cross(few-shot).py:326-349)."""
    starts, start = [], 0
    while start + 383 < width:
        starts.append(start)
        start += 128
        if start + 383 >= width:
            if start == width - 384 + 128:
                break
            start = width - 384
    return starts


def blend_windows(outputs, starts, width, height=384):
    """Sequential blend of per-window densities [n, height, 384] exactly as the reference does it."""
    dm = torch.zeros(height, width, device=outputs.device, dtype=outputs.dtype)
    prev = -1
    for out, start in zip(outputs, starts):
        ov = prev - start + 1
        if ov > 0:
            dm[:, start:prev + 1] = dm[:, start:prev + 1] / 2 + out[:, :ov] / 2
        dm[:, prev + 1:start + 384] = out[:, max(ov, 0):]
        prev = start + 383
    return dm


def _bucket(n, max_batch):
    """Forward batch sizes come from {1, 2, 4, ..., max_batch}: the engine keeps one static plan (buffers + launch lists) per
    batch size, so arbitrary window counts would build arbitrarily many plans.  A chunk is padded up to its bucket."""
    b = 1
    while b < n and b < max_batch:
        b *= 2
    return min(b, max_batch)


def blend_windows_batched(outputs, starts, width, height=384):
    """blend_windows for n images of the SAME width at once: outputs [n, len(starts), height, 384] -> [n, height, width].  The
    same sequential arithmetic per image (previously covered columns: old / 2 + new / 2), one set of launches for all of them."""
    n = outputs.shape[0]
    dm = torch.zeros(n, height, width, device=outputs.device, dtype=outputs.dtype)
    prev = -1
    for k, start in enumerate(starts):
        out = outputs[:, k]
        ov = prev - start + 1
        if ov > 0:
            dm[:, :, start:prev + 1] = dm[:, :, start:prev + 1] / 2 + out[:, :, :ov] / 2
        dm[:, :, prev + 1:start + 384] = out[:, :, max(ov, 0):]
        prev = start + 383
    return dm


MAX_BLEND_WINDOWS = _lib.WINDOW_MAX_STARTS


def _native_plan(model, images, max_batch):
    """The window list [(image index, start column)] of a call that fits ONE forward of the native path -- fp32 device images of the
    model's height whose windows number <= max_batch -- or None (the torch path then runs)."""
    if not images or not hasattr(model, "_engine"):
        return None
    h = images[0].shape[-2]
    plan = [(i, s) for i, im in enumerate(images) for s in window_starts(im.shape[-1])]
    # (countr_window_blend takes at most MAX_BLEND_WINDOWS window positions per image: wider panoramas go to the torch path below)
    if (not plan or len(plan) > min(max_batch, 64) or h != getattr(model, "img_size", 384)
            or any(len(window_starts(im.shape[-1])) > MAX_BLEND_WINDOWS for im in images)
            or any((not im.is_cuda) or im.dtype != torch.float32 or im.dim() != 4 or im.shape[0] != 1 or im.shape[1] != 3 or im.shape[-2] != h
                   or not im.is_contiguous() for im in images)):
        return None
    return plan


def _gather_windows(L, images, plan, h, dst, nb, st):
    """The windows of `plan` cut straight into the batch buffer dst [nb, 3, h, 384] (countr_window_gather); padding rows zeroed."""
    import ctypes as C
    nw = len(plan)
    frames = (C.c_void_p * nw)(*[images[i].data_ptr() for i, _s in plan])
    widths = (C.c_int * nw)(*[images[i].shape[-1] for i, _s in plan])
    starts = (C.c_int * nw)(*[s0 for _i, s0 in plan])
    _lib.check(L.countr_window_gather(frames, widths, starts, nw, h, dst.data_ptr(), st), "countr_window_gather")
    if nb > nw:
        dst[nw:].zero_()                       # padding rows only need defined values


def _width_runs(images):
    """Runs of consecutive images of one width: [(first image, count, width), ...]."""
    runs, i = [], 0
    while i < len(images):
        j = i
        while j + 1 < len(images) and images[j + 1].shape[-1] == images[i].shape[-1]:
            j += 1
        runs.append((i, j - i + 1, images[i].shape[-1]))
        i = j + 1
    return runs


def _blend_outputs(L, out, images, want_sums, st):
    """The forward's per-window densities out [>= windows, h, 384], in the order of _native_plan(images), stitched per image
    (countr_window_blend: one launch per run of consecutive images of one width) -> maps, or (maps, sums)."""
    import ctypes as C
    h = images[0].shape[-2]
    dev = images[0].device
    res, sums = [None] * len(images), [None] * len(images)
    row = 0
    for i, n, w in _width_runs(images):         # one blend launch each
        stw = window_starts(w)
        if not stw:
            for k in range(i, i + n):
                res[k] = torch.zeros(h, w, device=dev)          # narrower than a window: the reference's loop never runs
                sums[k] = torch.zeros((), device=dev)
        else:
            dm = torch.empty(n, h, w, device=dev, dtype=torch.float32)
            sm = torch.empty(n, device=dev, dtype=torch.float32) if want_sums else None
            ws = torch.empty(n * int(L.countr_window_blend_blocks(h, w)), device=dev, dtype=torch.float32) if want_sums else None
            arr = (C.c_int * len(stw))(*stw)
            _lib.check(L.countr_window_blend(out[row:].data_ptr(), n, len(stw), arr, h, w, dm.data_ptr(), sm.data_ptr() if want_sums else None,
                                             ws.data_ptr() if want_sums else None, st), "countr_window_blend")
            for k in range(n):
                res[i + k] = dm[k]
                if want_sums:
                    sums[i + k] = sm[k]
            row += n * len(stw)
    return (res, sums) if want_sums else res


def _native_front(model, images, max_batch):
    """What every native one-forward call starts with: (window list, engine, forward batch size, stream pointer) after check_ln_fold on
    the first window, or None where _native_plan refuses the images."""
    import ctypes as C
    plan = _native_plan(model, images, max_batch)
    if plan is None:
        return None
    eng = model._engine()
    eng.check_ln_fold(images[plan[0][0]][:, :, :, plan[0][1]:plan[0][1] + 384])     # (first use of a weight set only: may rebuild the plans)
    return plan, eng, _bucket(len(plan), max_batch), C.c_void_p(torch.cuda.current_stream(images[0].device).cuda_stream)


def forward_ahead(eng, p, nb, S, fill, fill_next=None, load_boxes=None, have=None):
    """One forward batch of plan p = eng.plan(nb, S, False) with the optional encoder look-ahead -> (out [nb, h, 384], valid until the next
    forward of this plan, token).  fill(dst) writes this batch's images into dst [nb, 3, h, 384], padding rows included; it is skipped
    when `have` is the engine's token for this batch's latent (an earlier call ran its encoder ahead).  fill_next(dst), given where the
    caller found that the NEXT batch qualifies, does the same for that batch: its encoder forward then runs beside this batch's decoder /
    density head, and token (engine.pipe_claim) is the next call's `have`; None otherwise.  load_boxes(view [nb, S, 3, 64, 64]) writes the
    exemplars, padding rows included, when S > 0."""
    img = p.buf["img"]
    mine = p.enc_pipe is not None and eng.pipe_owner(have)
    if not mine:
        fill(img)
    ahead = p.enc_pipe is not None and fill_next is not None
    if ahead:
        fill_next(p.pipe_img[:img.numel()].view(img.shape))
    token = eng.pipe_claim() if ahead else None
    if S > 0:
        load_boxes(p.buf["boxes"].view(nb, S, 3, 64, 64))
    if mine or ahead:
        return eng.forward_loaded_pipelined(nb, S, mine, ahead), token
    return eng.forward_loaded(nb, S), token


@torch.no_grad()
def _native_maps(model, images, boxes, shot_num, max_batch, want_sums, have=None, ahead=None, flags=None):
    """density_maps through the two window kernels of the C ABI (countr_window_gather / countr_window_blend: windows cut straight into
    the engine's input batch, stitched + summed by one launch per image width) when the call fits ONE forward: fp32 device images of
    the model's height whose windows number <= max_batch.  Returns None when it does not apply (the torch path below then runs).
    Pipelined encoder (density_maps_stream): `ahead` = the images of the NEXT call -- if that call takes this path with the same forward
    batch size, their windows are gathered now and their frozen-encoder forward runs beside this call's decoder / density head
    (flags["ahead"] = the engine's ownership token if it did); `have` = the token of the call that ran THIS call's encoder forward."""
    front = _native_front(model, images, max_batch)
    if front is None:
        return None
    plan, eng, nb, st = front
    h = images[0].shape[-2]
    p = eng.plan(nb, shot_num, False)
    plan_next = _native_plan(model, ahead, max_batch) if (ahead is not None and p.enc_pipe is not None) else None
    if plan_next is not None and (_bucket(len(plan_next), max_batch) != nb or ahead[0].shape[-2] != h or ahead[0].device != images[0].device):
        plan_next = None

    def load_boxes(bx):
        for j, (i, _s) in enumerate(plan):
            bx[j].copy_(boxes[i][0, :shot_num])
        if nb > len(plan):
            bx[len(plan):].zero_()

    out, token = forward_ahead(eng, p, nb, shot_num, lambda dst: _gather_windows(eng.L, images, plan, h, dst, nb, st),
                               (lambda dst: _gather_windows(eng.L, ahead, plan_next, h, dst, nb, st)) if plan_next is not None else None,
                               load_boxes, have)
    if flags is not None:
        flags["ahead"] = token
    return _blend_outputs(eng.L, out, images, want_sums, st)


@torch.no_grad()
def density_maps(model, images, boxes, shot_num, max_batch=32, return_sums=False):
    """Stitched densities of SEVERAL images in as few forwards as possible: images = [[1, 3, 384, w_i], ...], boxes = per image
    [1, >= shot_num, 3, 64, 64] (anything when shot_num == 0) -> [[384, w_i], ...].  Every 384-px window of every image is an
    independent forward of the reference (FSC_test_cross(few-shot).py:326-349, demo_zero.py:49-72), so the windows of all images
    are concatenated and run in chunks of up to max_batch (zero-shot 1920x1080 frames: 8 images x 4 windows = one batch of 32).
    Images of equal width (video frames) are cut into windows and blended together: one strided copy per window position and one
    blend pass for the whole group instead of one per image (the per-image torch launches were ~10 % of the 8-frame call)."""
    shot_num = int(shot_num)
    native = _native_maps(model, images, boxes, shot_num, max_batch, return_sums)
    if native is not None:
        return native
    dev = images[0].device
    h = images[0].shape[-2]
    plan = [(i, s) for i, im in enumerate(images) for s in window_starts(im.shape[-1])]
    # runs of consecutive images with one width: (first image, count, width).  Their windows are consecutive rows of the plan
    # (image-major), so window position k of the whole run is the strided slice rows[k::nwin] -- no index tensors, no host sync
    runs = _width_runs(images)
    first_row, r = {}, 0
    for i, im in enumerate(images):
        first_row[i] = r
        r += len(window_starts(im.shape[-1]))
    stacked = {i0: torch.cat(images[i0:i0 + n], 0) for i0, n, w in runs if n > 1 and window_starts(w)}
    outs = []
    for c0 in range(0, len(plan), max_batch):
        chunk = plan[c0:c0 + max_batch]
        nb = _bucket(len(chunk), max_batch)
        wins = (torch.empty if nb == len(chunk) else torch.zeros)(nb, 3, h, 384, device=dev, dtype=torch.float32)   # padding rows only need defined values
        done = set()
        for i0, n, w in runs:                    # whole runs that lie inside this chunk: one strided copy per window position
            st = window_starts(w)
            r0 = first_row[i0] - c0
            if i0 not in stacked or r0 < 0 or r0 + n * len(st) > len(chunk):
                continue
            for k, s0 in enumerate(st):
                wins[r0 + k:r0 + n * len(st):len(st)] = stacked[i0][:, :, :, s0:s0 + 384]
            done.update(range(r0, r0 + n * len(st)))
        for j, (i, s0) in enumerate(chunk):
            if j not in done:
                wins[j] = images[i][0, :, :, s0:s0 + 384]
        if shot_num > 0:
            bx = torch.zeros(nb, shot_num, 3, 64, 64, device=dev, dtype=torch.float32)
            for j, (i, _s) in enumerate(chunk):
                bx[j] = boxes[i][0, :shot_num]
        else:
            bx = torch.zeros(nb, 0, device=dev)
        o = model(wins, bx, shot_num)[:len(chunk)]
        outs.append(o.clone() if c0 + max_batch < len(plan) else o)    # the engine's output buffer lives until the next forward
    outs = torch.cat(outs, 0) if len(outs) > 1 else (outs[0] if outs else None)
    res = [None] * len(images)
    for i0, n, w in runs:
        starts = window_starts(w)
        if not starts:
            for i in range(i0, i0 + n):
                res[i] = torch.zeros(h, w, device=dev)      # narrower than a window: the reference's loop never runs
            continue
        k0 = first_row[i0]
        if n > 1:
            dm = blend_windows_batched(outs[k0:k0 + n * len(starts)].view(n, len(starts), h, 384), starts, w, h)
            for k in range(n):
                res[i0 + k] = dm[k]
        else:
            res[i0] = blend_windows(outs[k0:k0 + len(starts)], starts, w, h)
    return (res, [d.sum() for d in res]) if return_sums else res


@torch.no_grad()
def density_maps_stream(model, groups, shot_num, max_batch=32, return_sums=False):
    """density_maps over a SEQUENCE of calls -- groups = iterable of (images, boxes), e.g. eight video frames each -- with the frozen
    encoder pipelined across them: nothing in a forward depends on another forward (models_mae_cross.py:201-207 under no_grad), so
    while group k's decoder and density head run, group k + 1's windows are already cut and their encoder forward runs on a lane of its
    own (engine.forward_loaded_pipelined); group k + 1 then starts at decoder_embed.  Yields, per group and in order, exactly what
    density_maps returns -- bit-identical maps; 7.70 -> 7.25 ms per 32 windows.  One group of look-ahead: the generator reads group
    k + 1 before it yields group k.  Groups that do not fit the native one-forward path (or whose neighbour needs another forward batch
    size) simply run on their own."""
    shot_num = int(shot_num)
    it = iter(groups)
    cur = next(it, None)
    have = None      # the engine's token for the encoder output computed ahead for `cur` (engine.pipe_claim), or None
    while cur is not None:
        nxt = next(it, None)
        images, boxes = cur
        flags = {}
        res = _native_maps(model, images, boxes, shot_num, max_batch, return_sums, have=have,
                           ahead=(nxt[0] if nxt is not None else None), flags=flags)
        if res is None:
            res = density_maps(model, images, boxes, shot_num, max_batch, return_sums)
        have = flags.get("ahead")
        yield res
        cur = nxt


@torch.no_grad()
def density_map(model, samples, boxes, shot_num, max_batch=32):
    """samples [1, 3, 384, w] -> stitched density [384, w]; all windows run as batched forwards."""
    return density_maps(model, [samples], [boxes], shot_num, max_batch)[0]


def _small_exemplars(pos):
    s_cnt = 0
    for rect in (pos or [])[:3]:
        if rect[2] - rect[0] < 10 and rect[3] - rect[1] < 10:
            s_cnt += 1
    return s_cnt


def _normalise(pred, dm, pos, normalization):
    """Test-time normalisation (FSC_test_cross(few-shot).py:353-359): divide by the mean count inside the exemplar boxes if > 1.8."""
    if normalization and pos:
        e_cnt = sum((dm[r[0]:r[2] + 1, r[1]:r[3] + 1].sum() / 60).item() for r in pos) / 3
        if e_cnt > 1.8:
            pred /= e_cnt
    return pred


def split_count(dms, pos, normalization):
    """The count rule of the 3 x 3 split (FSC_test_cross(few-shot).py:273-320, 353-359): dms = the nine crops' maps in the reference's
    list order -> (pred_cnt, density_map).  The count is the sum of the nine maps' counts, added in list order (the order decides the
    last bits); the map, which the normalisation reads, is the LAST crop's (the reference reuses its variable)."""
    pred = sum((d.sum() / 60).item() for d in dms)
    dm = dms[-1]
    return _normalise(pred, dm, pos, normalization), dm


@torch.no_grad()
def count_image(model, samples, boxes, shot_num, pos=None, normalization=True, max_s_cnt=1, max_batch=32, return_crops=False):
    """Full per-image test path: returns (pred_cnt, density_map).  pos: exemplar rectangles [(y1, x1, y2, x2), ...].
    return_crops=True: (pred_cnt, density_map, crops) -- crops = the nine maps of the 3x3 path in the reference's list order (the report's
    misc.make_grid tiles them; density_map is the last of them), or None when the image did not take that path."""
    _, _, h, w = samples.shape
    dms = None
    if pos is not None and _small_exemplars(pos) >= max_s_cnt:
        # 3x3 split: each crop is upscaled back to (h, w) and counted on its own (FSC_test_cross(few-shot).py:273-320); the nine
        # upscaled crops are nine independent images for the stitcher, so all their windows share forwards
        crops = []
        for (top, left) in ((0, 0), (h // 3, 0), (0, w // 3), (h // 3, w // 3), (h * 2 // 3, 0), (h * 2 // 3, w // 3),
                            (0, w * 2 // 3), (h // 3, w * 2 // 3), (h * 2 // 3, w * 2 // 3)):
            crop = samples[:, :, top:top + h // 3, left:left + w // 3]
            crops.append(F.interpolate(crop, size=(h, w), mode="bilinear", align_corners=False))
        dms = density_maps(model, crops, [boxes] * 9, shot_num, max_batch)
        pred, dm = split_count(dms, pos, normalization)
    else:
        dm = density_map(model, samples, boxes, shot_num, max_batch)
        pred = _normalise((dm.sum() / 60).item(), dm, pos, normalization)
    return (pred, dm, dms) if return_crops else (pred, dm)


def image_chunks(widths, max_batch=32):
    """Positions of consecutive images (given by their widths) grouped into forward batches: as many images as fill one batch of
    max_batch windows, an image with more windows than that on its own -> [[0, 1, ...], ...]."""
    g0, chunks = 0, []
    while g0 < len(widths):                             # as many images as fill one forward batch
        g1, nwin = g0, 0
        while g1 < len(widths) and (g1 == g0 or nwin + len(window_starts(widths[g1])) <= max_batch):
            nwin += len(window_starts(widths[g1]))
            g1 += 1
        chunks.append(list(range(g0, g1)))
        g0 = g1
    return chunks


def class_batches(widths, shots, split, max_batch=32):
    """The forward batches count_items / count_images form for the frames of ONE exemplar set (a class), from sizes alone: widths [F] of
    the prepared frames, shots [F] exemplars per frame, split [F] whether the frame takes the 3 x 3 split -> [(shot count, variants,
    windows, bucket), ...].  A variant is an image that is cut into windows: (frame, -1) = the prepared frame, (frame, k) = crop k of
    its split, upscaled to the frame's size.  windows = [(variant, start column), ...] in forward order, bucket = the forward batch
    size.  A split frame is a batch of its own; the others are grouped by shot count and chunked by image_chunks.  Two batches run the
    same encoder forward iff their windows and buckets are equal: the kernels choose split-K by batch size, so a row is reproducible
    only inside the same forward batch.  bucket is None where the batch does not fit one native forward (no windows, or more than
    max_batch of them): density_maps then runs it as before."""
    out, groups = [], {}

    def batch(S, variants):
        windows = [(v, s0) for v in variants for s0 in window_starts(widths[v[0]])]
        fits = (0 < len(windows) <= min(max_batch, 64)
                and all(len(window_starts(widths[f])) <= MAX_BLEND_WINDOWS for f, _k in variants))
        out.append((S, variants, windows, _bucket(len(windows), max_batch) if fits else None))

    for f in range(len(widths)):
        if split[f]:
            batch(shots[f], [(f, k) for k in range(9)])
        else:
            groups.setdefault(shots[f], []).append(f)
    for S, idxs in groups.items():
        for sel in image_chunks([widths[f] for f in idxs], max_batch):
            batch(S, [(idxs[k], -1) for k in sel])
    return out


@torch.no_grad()
def density_maps_shared(model, images, jobs, max_batch=32):
    """density_maps of the SAME images for several exemplar sets with one encoder forward: jobs = [(boxes, shot_num), ...], boxes as
    density_maps takes them -> one list of maps per job, each bit-identical to density_maps(model, images, boxes, shot_num, max_batch).
    Where the images fit one native forward the windows are gathered once; the first job runs the ordinary forward, every further job
    of its shot count only the class-dependent tail (engine.forward_loaded_tail), and the first job of another shot count the decoder
    side on a copy of the latent (engine.forward_loaded_from).  A job's exemplars enter its plan by one indexed copy.  Images that do
    not fit run through density_maps job by job."""
    front = _native_front(model, images, max_batch)
    if front is None:
        return [density_maps(model, images, bx, int(S), max_batch) for bx, S in jobs]
    plan, eng, nb, st = front
    dev = images[0].device
    nw = len(plan)
    shots = list(dict.fromkeys(int(S) for _bx, S in jobs))
    for _ in range(2):          # every plan exists before the first forward: building one may grow the shared scratch and drop the others
        for S in shots:
            eng.plan(nb, S, False)
    if any((nb, S, False) not in eng.plans for S in shots):
        raise _lib.CountrError("density_maps_shared: the engine could not hold the plans of %d shot counts at once" % len(shots))
    _gather_windows(eng.L, images, plan, images[0].shape[-2], eng.plan(nb, shots[0], False).buf["img"], nb, st)
    rows = torch.tensor([i for i, _s in plan], device=dev) if any(shots) else None          # window -> its image
    res = [None] * len(jobs)
    for S in shots:
        p = eng.plan(nb, S, False)
        first = True
        for j, (boxes, Sj) in enumerate(jobs):
            if int(Sj) != S:
                continue
            if S > 0:
                bx = p.buf["boxes"].view(nb, S, 3, 64, 64)
                torch.index_select(torch.cat([b[:, :S] for b in boxes], 0), 0, rows, out=bx[:nw])
                if nb > nw:
                    bx[nw:].zero_()
            if not first:
                out = eng.forward_loaded_tail(nb, S)
            elif S == shots[0]:
                out = eng.forward_loaded(nb, S)     # [nb, h, 384], valid until the next forward of this plan
            else:
                out = eng.forward_loaded_from(nb, S, shots[0])
            first = False
            res[j] = _blend_outputs(eng.L, out, images, False, st)
    return res


@torch.no_grad()
def count_images(model, items, normalization=True, max_s_cnt=1, max_batch=32, return_crops=False):
    """Test path over MANY images with windows batched across images: items = [(samples [1,3,384,w], boxes [1,S,3,64,64] or
    empty, pos or None), ...] -> [(pred_cnt, density_map), ...] in input order.  Images are grouped by shot count (one forward
    has one shot_num, models_mae_cross.py:201); images that take the 3x3 split path already fill batches on their own.
    return_crops=True: (pred_cnt, density_map, crops) per image, crops as count_image returns them."""
    res = [None] * len(items)
    groups = {}
    for idx, (samples, boxes, pos) in enumerate(items):
        S = boxes.shape[1] if boxes.nelement() > 0 else 0
        if pos is not None and _small_exemplars(pos) >= max_s_cnt:
            res[idx] = count_image(model, samples, boxes, S, pos, normalization, max_s_cnt, max_batch, return_crops)
        else:
            groups.setdefault(S, []).append(idx)
    for S, idxs in groups.items():
        chunks = [[idxs[k] for k in sel] for sel in image_chunks([items[i][0].shape[-1] for i in idxs], max_batch)]
        # consecutive forwards of one shot count: the next chunk's encoder forward runs beside this chunk's decoder / head
        stream = density_maps_stream(model, (([items[i][0] for i in sel], [items[i][1] for i in sel]) for sel in chunks), S, max_batch)
        for sel, dms in zip(chunks, stream):
            for i, dm in zip(sel, dms):
                pred = _normalise((dm.sum() / 60).item(), dm, items[i][2], normalization)
                res[i] = (pred, dm, None) if return_crops else (pred, dm)
    return res
