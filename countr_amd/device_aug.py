"""Training batches from recipes: the train-time augmentation of countr_amd/data/fsc147.py on the device.

A loader built with TrainData(..., device_aug=True) hands over recipes (fsc147.recipe_train): the decoded uint8 frame, the draws and
the final dot cells.  DeviceAug.batch turns a list of them into the three tensors FinetuneStep.load() takes -- imgs [B, 3, 384, 384],
boxes [B, 3, 3, 64, 64], gt [B, 384, 384], fp32 -- with HIP kernels on the current stream (csrc/frames.hip, csrc/augment.hip):

    frame --countr_frame_resize_u8--> clean --countr_aug_jitter (noise + colour jitter)--> --countr_aug_blur--> --countr_aug_window
    (affine warp + flip + crop)--> imgs[b];   clean --countr_aug_exemplars--> boxes[b];   dot cells --countr_aug_density--> gt[b]

Plain recipes (--no_do_aug) skip the middle (the window is cut from the clean frame), mosaic recipes upload the image the host's
mosaic() finished.  One host-to-device copy and seven launches per batch plus two per distinct frame size for the resize (batches
above 32 images go in groups of 32).  There is no host fallback.

"mosaic_dev" recipes (TrainData(..., device_mosaic=True)) bring the decoded frames of their four pieces and the draws instead of a
finished image: every frame is uploaded and resized with the others (frames of one size share a launch pair), and one more launch,
countr_aug_mosaic (csrc/mosaic.hip), crops, resizes and cross-fades the pieces straight into imgs[b].  The window launch still writes
such a row first (a plain crop of the sample's own clean frame, so that its table stays one entry per batch row); the mosaic launch
follows it on the same stream and overwrites the row."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _owned
from .data import fsc147
from .frames import FramePrep, MAX_BATCHED

OUT = fsc147.MAX_HW
BOX = 64


def blur_weights(sigma):
    """The two normalised 1-D kernels of fsc147.gaussian_blur(img, (7, 9), sigma), computed as it computes them (fp32)."""
    def k1d(n):
        x = torch.linspace(-(n - 1) * 0.5, (n - 1) * 0.5, n, dtype=torch.float32)
        k = torch.exp(-0.5 * (x / sigma) ** 2)
        return (k / k.sum()).tolist()
    return k1d(7), k1d(9)


def affine_coeffs(h, w, pr):
    """The six doubles of countr_aug_image.affine for AugParams pr on an h x w image: what fsc147.warp_affine hands to scipy."""
    Mi = np.linalg.inv(fsc147.affine_matrix(h, w, pr.rotate, pr.scale, pr.shear, pr.tx, pr.ty))
    return [Mi[1, 1], Mi[1, 0], Mi[1, 2], Mi[0, 1], Mi[0, 0], Mi[0, 2]]


def fill_params(d, h, w, pr):
    """Jitter / blur / affine fields of a countr_aug_image from AugParams."""
    d.brightness, d.contrast, d.saturation, d.hue = pr.brightness, pr.contrast, pr.saturation, pr.hue
    d.nops = len(pr.order)
    for k, op in enumerate(pr.order):
        d.order[k] = int(op)
    kx, ky = blur_weights(pr.sigma)
    d.kx[:] = kx
    d.ky[:] = ky
    d.affine[:] = affine_coeffs(h, w, pr)


def _pad4(n):
    return (n + 3) & ~3


def _pad16(n):
    return (n + 15) & ~15


class _Stage:
    """One pinned host arena and its device copy: everything a batch uploads (frames, mosaic images, dot cells) in ONE copy."""

    def __init__(self, device):
        self.device = device
        self.host = self.dev = None
        self.copied = None

    def reserve(self, nbytes):
        if self.copied is not None:
            self.copied.synchronize()          # the previous upload from this arena must have left it
        if self.host is None or self.host.numel() < nbytes:
            self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def upload(self, nbytes):
        self.dev[:nbytes].copy_(self.host[:nbytes], non_blocking=True)
        if self.copied is None:
            self.copied = torch.cuda.Event()
        self.copied.record(torch.cuda.current_stream(self.device))


class DeviceAug:
    """Owns what must not be allocated per batch: the resize tap tables (a FramePrep's), two upload arenas used in turn (so that
    filling one does not wait for the previous batch's copy), and the device workspaces -- the uint8 intermediate of the resize, the
    clean resized frames, two ping-pong images, the partial sums of the contrast mean.  All grow on demand and never shrink.  Only
    the three returned tensors are new in every call: FinetuneStep.load() keeps references to them until the following step() and
    matches next_imgs by identity."""

    def __init__(self, device="cuda", batch=8, noise_seed=0):
        self.device = _owned.resolve(device, "DeviceAug")
        self.L = _lib.lib()
        self.batch_hint = int(batch)
        self.noise_seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
        self.prep = FramePrep(self.device)             # tap tables per (in, out) size
        self._stages = [_Stage(self.device), _Stage(self.device)]
        self._turn = 0
        self._clean = self._ping = self._pong = self._tmp = None
        self._partials = torch.empty(self.L.countr_aug_partials_floats(_lib.AUG_MAX_IMAGES), dtype=torch.float32, device=self.device)
        self._last = None                              # (stream, event) of the previous batch, for a call from another stream
        self.launches = 0                              # kernel launches of the last batch() call

    def workspace_bytes(self):
        ts = [self._clean, self._ping, self._pong, self._tmp, self._partials] + [t for s in self._stages for t in (s.host, s.dev)]
        ts += [t for pair in self.prep._tables.values() for t in pair]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    @staticmethod
    def _frame(fr):
        fr = fr.numpy() if isinstance(fr, torch.Tensor) else np.asarray(fr)
        if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
            raise ValueError("DeviceAug.batch: frames are uint8 [H, W, 3]")
        return fr

    @staticmethod
    def _mosaic_entry(row, r, clean_of):
        """countr_mosaic_image of mosaic_dev recipe r for batch row `row`; clean_of(k) -> (device address, (h, w)) of its frame k."""
        m = _lib.MosaicImage()
        m.bl, m.row = int(r["bl"]), row
        if len(r["pieces"]) != 4:
            raise ValueError("DeviceAug.batch: a mosaic_dev recipe has four pieces")
        for q, (k, nh, nw, start_h, start_w, length) in zip(m.piece, r["pieces"]):
            ptr, (h, w) = clean_of(int(k))
            if (h, w) != (int(nh), int(nw)):
                raise ValueError("DeviceAug.batch: piece of %s drawn on %d x %d, its frame resizes to %d x %d" % (r["im_id"], nh, nw, h, w))
            q.src, q.h, q.w, q.start_h, q.start_w, q.length = ptr, h, w, int(start_h), int(start_w), int(length)
        return m

    def batch(self, recipes, noise=None):
        """recipes: a list of fsc147.recipe_train results -> (imgs [B, 3, 384, 384], boxes [B, 3, 3, 64, 64], gt [B, 384, 384],
        m_flags [B] (a host list)).  noise: None (the generator: Philox stream (noise_seed, recipe counter)) or a list with, per
        recipe, an explicit [3, new_h, new_w] noise image (already scaled; None entries fall back to the generator) -- the tests and a
        user's own stream."""
        B = len(recipes)
        if B < 1:
            raise ValueError("DeviceAug.batch: empty batch")
        for r in recipes:
            if len(r["rects"]) != 3:
                raise ValueError("DeviceAug.batch: %s has %d exemplar boxes, the batch layout needs 3" % (r["im_id"], len(r["rects"])))
        dev = self.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            st = C.c_void_p(cur.cuda_stream)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])
            self.launches = 0
            # ---- one upload: frames (16-byte aligned each), mosaic images, explicit noise, dot cells
            # frames: slot i < B is recipe i's own frame, the foreign frames of the mosaic_dev recipes follow
            frames = [self._frame(r["frames"][0] if r["kind"] == "mosaic_dev" else r["frame"]) for r in recipes]
            shapes = [(r["new_h"], r["new_w"]) for r in recipes]
            slot_of = {}                                   # (recipe, index in its frames) -> slot
            for i, r in enumerate(recipes):
                if r["kind"] == "mosaic_dev":
                    slot_of[(i, 0)] = i
                    for k in range(1, len(r["frames"])):
                        slot_of[(i, k)] = len(frames)
                        frames.append(self._frame(r["frames"][k]))
                        shapes.append(fsc147.flex_resize(frames[-1].shape[0], frames[-1].shape[1]))
            off, f_off, m_off, n_off = 0, [], {}, {}
            for fr in frames:
                f_off.append(off)
                off += _pad16(fr.size)
            for i, r in enumerate(recipes):
                if r["kind"] == "mosaic":
                    m_off[i] = off
                    off += 3 * OUT * OUT * 4
                elif noise is not None and noise[i] is not None and r["kind"] == "aug":
                    n_off[i] = off
                    off += _pad16(3 * r["new_h"] * r["new_w"] * 4)
            c_off, ncells = off, sum(len(r["cells"]) for r in recipes)
            off += _pad16(max(ncells, 1) * 4)
            stage = self._stages[self._turn]
            self._turn ^= 1
            stage.reserve(off)
            hb = stage.host.numpy()
            cell_rng, k = [], 0
            for s, fr in enumerate(frames):
                hb[f_off[s]:f_off[s] + fr.size] = fr.reshape(-1)
            for i, r in enumerate(recipes):
                if i in m_off:
                    hb[m_off[i]:m_off[i] + 3 * OUT * OUT * 4].view(np.float32)[:] = r["image"].numpy().reshape(-1)
                if i in n_off:
                    nz = np.asarray(noise[i], dtype=np.float32).reshape(-1)
                    if nz.size != 3 * r["new_h"] * r["new_w"]:
                        raise ValueError("DeviceAug.batch: explicit noise of recipe %d is not [3, new_h, new_w]" % i)
                    hb[n_off[i]:n_off[i] + nz.size * 4].view(np.float32)[:] = nz
                cl = np.asarray(r["cells"], dtype=np.int64).reshape(-1, 2)
                if len(cl) and (cl.min() < 0 or cl.max() >= OUT):
                    raise ValueError("DeviceAug.batch: dot cell outside the 384 x 384 target")
                hb[c_off + 4 * k:c_off + 4 * (k + len(cl))].view(np.int32)[:] = (cl[:, 0] << 16 | cl[:, 1]).astype(np.int32)
                cell_rng.append((k, len(cl)))
                k += len(cl)
            stage.upload(off)
            base = stage.dev.data_ptr()
            # ---- workspaces: clean / ping / pong hold every image of the batch back to back (sizes padded to 16 bytes)
            # (only the B own frames can go through the chain: ping / pong end where the foreign frames begin)
            sizes = [_pad4(3 * nh * nw) for nh, nw in shapes]
            w_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            clean = _owned.grow(self, "_clean", int(w_off[-1]), torch.float32)
            ping = _owned.grow(self, "_ping", int(w_off[B]), torch.float32)
            pong = _owned.grow(self, "_pong", int(w_off[B]), torch.float32)
            # ---- resize + ToTensor: frames of one (H, W) share a launch pair
            by_shape = {}
            for s, fr in enumerate(frames):
                by_shape.setdefault((int(fr.shape[0]), int(fr.shape[1])) + tuple(shapes[s]), []).append(s)
            need = max(min(len(ix), MAX_BATCHED) * H * nw * 3 for (H, W, nh, nw), ix in by_shape.items())
            tmp = _owned.grow(self, "_tmp", need, torch.uint8)
            for (H, W, nh, nw), idxs in by_shape.items():
                hbt, hwt = self.prep.tables(W, nw)
                vbt, vwt = self.prep.tables(H, nh)
                for g0 in range(0, len(idxs), MAX_BATCHED):
                    sel = idxs[g0:g0 + MAX_BATCHED]
                    fp = (C.c_void_p * len(sel))(*[base + f_off[i] for i in sel])
                    op = (C.c_void_p * len(sel))(*[clean.data_ptr() + 4 * int(w_off[i]) for i in sel])
                    _lib.check(self.L.countr_frame_resize_u8(fp, op, len(sel), H, W, nh, nw, hbt.data_ptr(), hwt.data_ptr(), vbt.data_ptr(),
                                                             vwt.data_ptr(), tmp.data_ptr(), st), "countr_frame_resize_u8")
                    self.launches += 2
            # ---- descriptors
            imgs = torch.empty(B, 3, OUT, OUT, device=dev, dtype=torch.float32)
            boxes = torch.empty(B, 3, 3, BOX, BOX, device=dev, dtype=torch.float32)
            gt = torch.empty(B, OUT, OUT, device=dev, dtype=torch.float32)
            table = (_lib.AugImage * B)()
            chain, mosaics = [], []
            for i, r in enumerate(recipes):
                d, h, w = table[i], r["new_h"], r["new_w"]
                d.src = clean.data_ptr() + 4 * int(w_off[i])
                d.jit = ping.data_ptr() + 4 * int(w_off[i])
                d.blr = pong.data_ptr() + 4 * int(w_off[i])
                d.h, d.w = h, w
                d.rects[:] = [int(v) for rect in r["rects"] for v in rect]
                d.cell_off, d.cell_cnt = cell_rng[i]
                if r["kind"] == "aug":
                    fill_params(d, h, w, r["params"])
                    d.counter = int(r["noise_counter"]) & 0xFFFFFFFFFFFFFFFF
                    if i in n_off:
                        d.noise, d.noise_mode = base + n_off[i], 2
                    else:
                        d.noise_mode = 1
                    d.win, d.win_h, d.win_w, d.win_mode = d.blr, h, w, 1
                    d.flip, d.start_h, d.start_w = int(r["flip"]), r["start_h"], r["start_w"]
                    chain.append(i)
                elif r["kind"] == "plain":
                    d.win, d.win_h, d.win_w, d.win_mode = d.src, h, w, 0
                    d.start_h, d.start_w = r["start_h"], r["start_w"]
                elif r["kind"] == "mosaic":
                    d.win, d.win_h, d.win_w, d.win_mode = base + m_off[i], OUT, OUT, 0
                elif r["kind"] == "mosaic_dev":
                    d.win, d.win_h, d.win_w, d.win_mode = d.src, h, w, 0      # a valid window; countr_aug_mosaic overwrites the row
                    mosaics.append(self._mosaic_entry(i, r, lambda k, i=i: (clean.data_ptr() + 4 * int(w_off[slot_of[(i, k)]]),
                                                                            shapes[slot_of[(i, k)]])))
                else:
                    raise ValueError("DeviceAug.batch: unknown recipe kind %r" % (r["kind"],))
            # ---- the chain on the augmented images, then the three outputs for every image
            G = _lib.AUG_MAX_IMAGES
            if chain:
                sub = (_lib.AugImage * len(chain))(*[table[i] for i in chain])
                for g0 in range(0, len(chain), G):
                    n = min(G, len(chain) - g0)
                    part = C.byref(sub[g0])
                    _lib.check(self.L.countr_aug_jitter(part, n, self.noise_seed, self._partials.data_ptr(), st), "countr_aug_jitter")
                    _lib.check(self.L.countr_aug_blur(part, n, st), "countr_aug_blur")
                    self.launches += 3
            for g0 in range(0, B, G):
                n = min(G, B - g0)
                part = C.byref(table[g0])
                _lib.check(self.L.countr_aug_window(part, n, imgs[g0:].data_ptr(), st), "countr_aug_window")
                _lib.check(self.L.countr_aug_exemplars(part, n, boxes[g0:].data_ptr(), st), "countr_aug_exemplars")
                _lib.check(self.L.countr_aug_density(part, n, base + c_off, max(ncells, 1), gt[g0:].data_ptr(), st), "countr_aug_density")
                self.launches += 3
            for g0 in range(0, len(mosaics), G):       # after the window launches: the rows of the mosaic_dev recipes
                sub = (_lib.MosaicImage * len(mosaics[g0:g0 + G]))(*mosaics[g0:g0 + G])
                _lib.check(self.L.countr_aug_mosaic(sub, len(sub), imgs.data_ptr(), B, st), "countr_aug_mosaic")
                self.launches += 1
            if self._last is None or self._last[0] != cur:
                self._last = (cur, torch.cuda.Event())
            self._last[1].record(cur)
        return imgs, boxes, gt, [int(r["m_flag"]) for r in recipes]
