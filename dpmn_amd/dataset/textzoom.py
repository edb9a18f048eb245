"""TextZoom data path of the SR trainer: the parts of dataset/dataset.py that
interfaces/base.py:85-125 wires into the training / evaluation loaders, restricted to what the SR path consumes.

  lmdbDataset_real          dataset.py:565-686   LMDB reader: keys image_hr-%09d / image_lr-%09d / label-%09d / num-samples
  resizeNormalize           dataset.py:1266-1319 PIL bicubic resize -> ToTensor -> optional mask channel (gray > mean ? 0 : 255)
  alignCollate_realWTLAMask dataset.py:1966-2076 batch of (HR, LR, label) -> the tuple TextSR.train unpacks (super_resolution.py:142)

Host code by nature (JPEG / PNG decode and PIL resampling are what the reference does too); PIL is the same library the
reference calls, so `resizeNormalize` is not a restatement of an algorithm but the same calls.  Left out, with the positions
kept in the collated tuple: the YUV copies (cv2.cvtColor, read by nothing on the SR path), imgaug augmenters (constructed but
never applied by these classes).  Manmade degradation and cutblur (dataset.py:422-489, 622-637; main.py --manmade_degrade / --cutblur)
do not run per image on the host here: the dataset hands out the HR image in the LR position, the collate function packs the HR pixels
once and `sr_batches` synthesises the LR batch on the GPU (ops.degrade_ragged_u8, then the ragged resize).  The JPEG stage the reference
left commented out on the resized image (dataset.py:559 JPEG_compress, :1298-1300; main.py --jpeg_degrade) runs there too, on the resized
uint8 LR batch (ops.jpeg_roundtrip_u8), with a quality drawn per image.  `lmdb` itself is imported lazily:
it is not installed in the build image, so the reader is exercised in tests/ through an injected environment object with the
same `begin().get(key)` protocol, over images encoded the way TextZoom stores them.
"""
import io

import numpy as np
import torch

from ..utils.util import str_filt


def buf2PIL(txn, key, mode='RGB'):
    """dataset.py:54-60."""
    from PIL import Image
    buf = txn.get(key)
    if buf is None:
        raise IOError("missing key %r" % key)
    return Image.open(io.BytesIO(buf)).convert(mode)


def _to_tensor(img):
    """torchvision.transforms.ToTensor for a PIL image of mode RGB / L: uint8 HWC -> float CHW / 255."""
    a = np.asarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float().div(255.0)


class lmdbDataset_real(torch.utils.data.Dataset):
    def __init__(self, root=None, voc_type='upper', max_len=100, test=False, cutblur=False, manmade_degrade=False, rotate=None,
                 env=None):
        super().__init__()
        if cutblur and not manmade_degrade:
            raise ValueError("dpmn_amd lmdbDataset_real: cutblur needs manmade_degrade (the reference's cutblur mixes LR and HR pixels "
                             "column by column, which needs equal native sizes; paired TextZoom crops do not have them)")
        if env is None:
            try:
                import lmdb
            except ImportError as e:
                raise RuntimeError("dpmn_amd: reading TextZoom needs the `lmdb` package (not installed here); "
                                   "main.py falls back to synthetic batches with --synthetic_steps") from e
            env = lmdb.open(root, max_readers=1, readonly=True, lock=False, readahead=False, meminit=False)
        self.env = env
        with self.env.begin(write=False) as txn:
            self.nSamples = int(txn.get(b'num-samples'))
        self.voc_type, self.max_len, self.test = voc_type, max_len, test
        # manmade_degrade: image_lr-* is not read, the HR image stands in the LR position (degraded on the GPU by sr_batches)
        self.manmade_degrade, self.cb_flag = bool(manmade_degrade), bool(cutblur)

    def __len__(self):
        return self.nSamples

    def __getitem__(self, index):
        assert index <= len(self), 'index range error'
        index += 1
        with self.env.begin(write=False) as txn:
            try:
                img_HR = buf2PIL(txn, b'image_hr-%09d' % index, 'RGB')
                img_lr = img_HR if self.manmade_degrade else buf2PIL(txn, b'image_lr-%09d' % index, 'RGB')
                word = txn.get(b'label-%09d' % index)
                word = " " if word is None else str(word.decode())
            except IOError:
                return self[index % len(self)]          # dataset.py:680-681: skip to the next sample (index is already +1)
        return img_HR, img_lr, None, None, str_filt(word, self.voc_type)


class resizeNormalize(object):
    def __init__(self, size, mask=False, interpolation=None):
        from PIL import Image
        self.size, self.mask = size, mask
        self.interpolation = Image.BICUBIC if interpolation is None else interpolation

    def __call__(self, img):
        img = img.resize(self.size, self.interpolation)
        t = _to_tensor(img)
        if self.mask:
            m = img.convert('L')
            thres = np.array(m).mean()
            m = m.point(lambda x: 0 if x > thres else 255)
            t = torch.cat((t, _to_tensor(m)), 0)
        return t


class resizeU8(object):
    """Host half of the GPU collate: the same PIL bicubic resize as resizeNormalize, returned as the raw uint8 HWC pixels --
    ToTensor and the mask channel run on the GPU (csrc/misc.hip k_collate_u8 through finish_on_gpu)."""

    def __init__(self, size, interpolation=None):
        from PIL import Image
        self.size = size
        self.interpolation = Image.BICUBIC if interpolation is None else interpolation

    def __call__(self, img):
        return torch.from_numpy(np.asarray(img.resize(self.size, self.interpolation), dtype=np.uint8).copy())


def finish_on_gpu(images_u8, mask, device):
    """(B, H, W, 3) uint8 from a gpu_finish collate -> (B, 3 + mask, H, W) float on `device` (one 3-byte-per-pixel upload and one
    kernel per batch instead of B x (ToTensor + convert('L') + point + cat) on the host and a 16-byte-per-pixel upload)."""
    from .. import ops
    return ops.collate_u8(images_u8.to(device, non_blocking=True), mask)


class alignCollate_realWTLAMask(object):
    """collate_fn of the training loader (base.py:99-102); returns the 9-tuple of dataset.py:2076 with None in the positions of
    the YUV copies and the pseudo-LR batch.  gpu_finish=True (ours): positions 0 and 2 hold the resized uint8 (B, H, W, 3) pixels
    and `sr_batches(loader, device)` finishes them on the GPU -- same values, bit for bit (tests/test_gpu_dataset.py).
    gpu_resize=True (ours, opt-in): no PIL resize here either; positions 0 and 2 hold the utils.resize.pack_ragged pair (packed uint8
    pixels of the decoded images, (B, 3) meta) and `sr_batches` resizes them on the GPU (ops.resize_ragged_u8, the same bytes as PIL's
    bicubic resize; tests/test_gpu_resize.py) before it finishes them.
    degrade=True (ours, needs gpu_resize): the LR images are synthesised from the HR images -- the HR pixels are packed ONCE, position
    2 carries the same pair as position 0 and `sr_batches` degrades them on the GPU (ops.degrade_ragged_u8; cutblur=True: with the
    reference's cutblur).  The random draws happen in sr_batches, in the main process, not in the loader's workers.
    jpeg=(lo, hi, prob) (ours, needs degrade): with probability prob a synthesised LR image, after its resize, goes through a JPEG of a
    quality drawn from lo .. hi (ops.jpeg_roundtrip_u8; the reference's JPEG_compress, dataset.py:559, fixes 40).
    psf=(kinds, prob, frac) (ours, needs degrade; main.py --psf_blur): with probability prob the HR pixels an LR image is synthesised
    from are first blurred by a random point-spread function of one of `kinds` (motion, disk, aniso; utils/psf.py) whose radius is
    drawn up to frac of the image's height (ops.psf_blur_ragged_u8); the HR batch stays sharp.
    render=(words, atlases) (ours, needs degrade; main.py --train_words, dataset/words.py WordsHR): the batch holds no image at all --
    positions 0 and 2 are None and `sr_batches` renders the HR images on the GPU (ops.render_words_u8) from the words and parameters
    it draws per batch; `render` is then True and `words` / `atlases` carry the pair.  render_fx (ours, needs render; main.py
    --train_words_fx): the utils.render.RenderFx of the run -- `sr_batches` then draws with draw_render_fx and renders with
    ops.render_words_fx_u8 (outline, drop shadow, photo background).  render_warp (ours, needs render; main.py --train_words_warp):
    the utils.render.RenderWarp of the run -- `sr_batches` then draws with draw_render_warp and renders with ops.render_words_warp_u8
    (projective distortion, rotation, curved baseline; with or without render_fx)."""

    def __init__(self, imgH=64, imgW=256, down_sample_scale=4, keep_ratio=False, min_ratio=1, mask=False, alphabet=53, train=True,
                 y_domain=False, gpu_finish=False, gpu_resize=False, degrade=False, cutblur=False, jpeg=None, render=None,
                 psf=None, render_fx=None, render_warp=None):
        if degrade and not gpu_resize:
            raise ValueError("alignCollate_realWTLAMask: degrade=True needs gpu_resize=True (the LR images are made on the GPU from the "
                             "packed HR pixels)")
        if cutblur and not degrade:
            raise ValueError("alignCollate_realWTLAMask: cutblur=True needs degrade=True (cutblur replaces columns of the LR image by the "
                             "HR image's, which needs equal native sizes; paired TextZoom crops do not have them)")
        if jpeg is not None and not degrade:
            raise ValueError("alignCollate_realWTLAMask: jpeg=(lo, hi, prob) needs degrade=True (the JPEG artefacts are put on the LR "
                             "images that are synthesised on the GPU; paired TextZoom LR crops are used as they are)")
        if jpeg is not None:
            lo, hi, prob = jpeg
            if not (1 <= int(lo) <= int(hi) <= 100 and 0.0 <= float(prob) <= 1.0):
                raise ValueError("alignCollate_realWTLAMask: jpeg=(lo, hi, prob) needs 1 <= lo <= hi <= 100 and 0 <= prob <= 1, got %r"
                                 % (jpeg,))
            jpeg = (int(lo), int(hi), float(prob))
        self.jpeg = jpeg
        if psf is not None and not degrade:
            raise ValueError("alignCollate_realWTLAMask: psf=(kinds, prob, frac) needs degrade=True (the point-spread function blurs the "
                             "HR pixels that the LR images are synthesised from on the GPU; paired TextZoom LR crops are used as they are)")
        if psf is not None:
            from ..utils.psf import KINDS
            kinds, prob, frac = psf
            kinds = tuple(kinds)
            if not (kinds and all(k in KINDS for k in kinds) and len(set(kinds)) == len(kinds) and 0.0 <= float(prob) <= 1.0
                    and 0.0 < float(frac) <= 1.0):
                raise ValueError("alignCollate_realWTLAMask: psf=(kinds, prob, frac) needs distinct kinds of %s, 0 <= prob <= 1 and "
                                 "0 < frac <= 1, got %r" % (", ".join(KINDS), psf))
            psf = (kinds, float(prob), float(frac))
        self.psf = psf
        if render is not None and not degrade:
            raise ValueError("alignCollate_realWTLAMask: render=(words, atlases) needs degrade=True (the rendered HR images have no LR "
                             "partner: it is synthesised on the GPU)")
        self.render = render is not None
        self.words, self.atlases = (list(render[0]), render[1]) if self.render else (None, None)
        if render_fx and not self.render:
            raise ValueError("alignCollate_realWTLAMask: render_fx needs render=(words, atlases) (the effects are drawn on rendered words)")
        self.render_fx = render_fx or None
        if render_warp and not self.render:
            raise ValueError("alignCollate_realWTLAMask: render_warp needs render=(words, atlases) (the warp is drawn on rendered words)")
        self.render_warp = render_warp or None
        self.imgH, self.imgW, self.down_sample_scale, self.mask = imgH, imgW, down_sample_scale, mask
        self.gpu_finish, self.gpu_resize, self.degrade, self.cutblur = gpu_finish, gpu_resize, bool(degrade), bool(cutblur)
        self.alphabet = "0123456789abcdefghijklmnopqrstuvwxyz"
        self.d2a = "-" + self.alphabet
        self.alsize = len(self.d2a)
        self.a2d = {ch: i for i, ch in enumerate(self.d2a)}
        if gpu_resize:
            self.transform = self.transform2 = None
        elif gpu_finish:
            self.transform = resizeU8((imgW, imgH))
            self.transform2 = resizeU8((imgW // down_sample_scale, imgH // down_sample_scale))
        else:
            self.transform = resizeNormalize((imgW, imgH), mask)
            self.transform2 = resizeNormalize((imgW // down_sample_scale, imgH // down_sample_scale), mask)

    def __call__(self, batch):
        images_HR, images_lr, _, _, label_strs = zip(*batch)
        if self.render:          # (nothing to pack: sr_batches renders the batch on the GPU)
            images_HR = images_lr = None
        elif self.gpu_resize:      # (pin=False: a loader with pin_memory pins its batches itself, and workers must not open the GPU)
            from ..utils.resize import pack_ragged
            rgb = lambda im: np.asarray(im if im.mode == 'RGB' else im.convert('RGB'), dtype=np.uint8)
            images_HR = pack_ragged([rgb(im) for im in images_HR], pin=False)
            images_lr = images_HR if self.degrade else pack_ragged([rgb(im) for im in images_lr], pin=False)
        else:
            images_HR = torch.stack([self.transform(im) for im in images_HR], 0)
            images_lr = torch.stack([self.transform2(im) for im in images_lr], 0)
        max_len = 26
        label_batches, weighted_masks, weighted_tics = [], [], []
        for word in label_strs:
            word = word.lower()
            if 1 < len(word) < 26:                       # spread the characters over 26 slots (dataset.py:2019-2027)
                padding = int((26 - len(word)) / (len(word) - 1))
                word = word[0] + "".join("-" * padding + ch for ch in word[1:])
            elif len(word) >= 26:
                word = word[:26]
            label_list = [self.a2d[ch] for ch in word if ch in self.a2d]
            if len(label_list) <= 0:
                weighted_masks.append(0)
            else:
                weighted_masks.extend(label_list)
            labels = torch.tensor(label_list, dtype=torch.long)[:, None]
            if labels.shape[0] > 0:
                label_batches.append(torch.zeros((labels.shape[0], self.alsize)).scatter_(-1, labels, 1))
                weighted_tics.append(1)
            else:
                vec = torch.zeros((1, self.alsize))
                vec[0, 0] = 1.
                label_batches.append(vec)
                weighted_tics.append(0)
        label_rebatches = torch.zeros((len(label_strs), max_len, self.alsize))
        for idx, lb in enumerate(label_batches):
            label_rebatches[idx][:lb.shape[0]] = lb
        label_rebatches = label_rebatches.unsqueeze(1).float().permute(0, 3, 1, 2)
        return images_HR, None, images_lr, None, None, label_strs, label_rebatches, torch.tensor(weighted_masks).long(), torch.tensor(weighted_tics)


def resize_on_gpu(pair, size, mask, device):
    """(packed, meta) of a gpu_resize collate -> (B, 3 + mask, H, W) float on `device`, size = (H, W): one upload of the decoded
    pixels, the ragged bicubic resize and the collate kernel."""
    from .. import ops
    packed, meta = pair
    return ops.collate_u8(ops.resize_ragged_u8(packed.to(device, non_blocking=True), meta, size[0], size[1]), mask)


def degrade_on_gpu(pair, size, scale, mask, device, cutblur=False, rng=None, jpeg=None, psf=None):
    """(packed, meta) of a degrade collate (the HR pixels; packed on the host, or already on `device`: a rendered batch of
    ops.render_words_u8) -> (images_hr (B, 3 + mask, H, W), images_lr (B, 3 + mask, H / scale,
    W / scale)) float on `device`, size = (H, W): one upload, the degradation of the ragged batch at the images' own sizes
    (ops.degrade_ragged_u8: the parameters of utils.degrade.draw_params and one 63-bit noise seed, both drawn from `rng`, Python's
    `random` by default), the two ragged resizes and the collate kernel.  jpeg = (lo, hi, prob): the resized LR batch, and only it,
    goes through ops.jpeg_roundtrip_u8 with the qualities of utils.jpeg.draw_jpeg, drawn from `rng` AFTER the draws above; with
    jpeg=None not one more draw is made.  psf = (kinds, prob, frac) (main.py --psf_blur): the PSFs of utils.psf.draw_psf are drawn
    from `rng` after the noise seed and BEFORE the JPEG qualities; the HR pack is blurred (ops.psf_blur_ragged_u8), the blurred pack
    is degraded with cut_x and cut_side zeroed, and cutblur then copies its columns from the UNBLURRED pack (ops.cutblur_ragged_u8):
    they stay the true HR pixels and the blur never reaches across the cut through the later filters' taps.  images_hr always comes
    from the unblurred pack; with psf=None the draws and launches are exactly those without it."""
    import random
    from .. import ops
    from ..utils.degrade import draw_params, CUT_X, CUT_SIDE
    rng = random if rng is None else rng
    packed, meta = pair
    params = draw_params(meta.shape[0], cutblur=cutblur, hr_widths=[int(w) for w in meta[:, 2]], rng=rng)
    seed = rng.getrandbits(63)
    packed = packed.to(device, non_blocking=True)
    if psf is None:
        low = ops.degrade_ragged_u8(packed, meta, params, seed=seed)
    else:
        from ..utils.psf import draw_psf
        taps = draw_psf(meta.shape[0], psf[0], psf[1], psf[2], [int(h) for h in meta[:, 1]], rng=rng)
        uncut = params.copy()
        uncut[:, [CUT_X, CUT_SIDE]] = 0
        low = ops.degrade_ragged_u8(ops.psf_blur_ragged_u8(packed, meta, taps), meta, uncut, seed=seed)
        low = ops.cutblur_ragged_u8(low, packed, meta, params)
    H, W = size
    low = ops.resize_ragged_u8(low, meta, H // scale, W // scale)
    if jpeg is not None:
        from ..utils.jpeg import draw_jpeg
        ops.jpeg_roundtrip_u8(low, draw_jpeg(meta.shape[0], jpeg[0], jpeg[1], jpeg[2], rng=rng), out=low)
    return ops.collate_u8(ops.resize_ragged_u8(packed, meta, H, W), mask), ops.collate_u8(low, mask)


def sr_batches(loader, device=None, mask=None, size=None):
    """Adapter for TextSR.train / eval / test: (images_hr, images_lr, label_vecs, label_strs) per batch.  label_vecs is None: for
    --arch tatt the reference derives them from a CRNN on the LR image (super_resolution.py:165-169), not from the dataset.
    Batches of a gpu_finish collate (uint8 pixels) are finished on `device` here (default: the current GPU); mask=None takes the
    collate function's own setting.  Batches of a gpu_resize collate (packed pixels of the decoded images) are resized here first;
    size = (imgH, imgW, down_sample_scale), None takes the collate function's own.  Batches of a degrade collate (the HR pixels in both
    positions) get their LR images here (degrade_on_gpu).  The randomness of a pass comes from ONE 63-bit draw from Python's `random`
    when the pass starts, in the main process; batch j then draws from random.Random(that key + j).  TextSR.train fetches a batch
    before it writes the training state of the step before it, so per-batch draws from the global stream would be repeated after a
    continuation; keyed by (pass, batch) a continued run (--train_state restores the stream the key came from) sees exactly the LR
    images the uninterrupted run saw.  Batches of a render collate (main.py --train_words) hold no image: from the batch's stream come
    FIRST the words and render parameters (utils.render.draw_render, one sample per item of the batch), THEN exactly the draws of
    degrade_on_gpu; the HR images are rendered on the GPU (ops.render_words_u8) and the yielded labels are the drawn words.  With the
    collate's render_fx (main.py --train_words_fx) the draws are utils.render.draw_render_fx's (every sample's fx draws follow its
    render draws, still before the degradation's) and the render is ops.render_words_fx_u8; without it nothing changes.  With the
    collate's render_warp (main.py --train_words_warp) the draws are utils.render.draw_render_warp's (every sample's warp draws follow
    its fx draws) and the render is ops.render_words_warp_u8; without it nothing changes either."""
    import random
    col = getattr(loader, "collate_fn", None)
    if mask is None:
        mask = bool(getattr(col, "mask", True))
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    degrade = bool(getattr(col, "degrade", False))
    pass_key = random.getrandbits(63) if degrade else None
    render = degrade and bool(getattr(col, "render", False))
    for j, data in enumerate(loader):
        hr, lr = data[0], data[2]
        labels = list(data[5])
        if render:
            from .. import ops
            from ..utils.render import draw_render
            if size is None:
                size = (col.imgH, col.imgW, col.down_sample_scale)
            H, W, scale = size
            rng = random.Random(pass_key + j)
            fx, warp = getattr(col, "render_fx", None), getattr(col, "render_warp", None)
            if warp:
                from ..utils.render import draw_render_warp
                labels, cls, lens, params, rows, wrows = draw_render_warp(col.words, col.atlases.n_fonts, rng, len(labels), fx, warp)
                pair = ops.render_words_warp_u8(cls, lens, params, rows, wrows, col.atlases, fx.pool if fx else None, device=device)
            elif fx:
                from ..utils.render import draw_render_fx
                labels, cls, lens, params, rows = draw_render_fx(col.words, col.atlases.n_fonts, rng, len(labels), fx)
                pair = ops.render_words_fx_u8(cls, lens, params, rows, col.atlases, fx.pool, device=device)
            else:
                labels, cls, lens, params = draw_render(col.words, col.atlases.n_fonts, rng, n=len(labels))
                pair = ops.render_words_u8(cls, lens, params, col.atlases, device=device)
            hr, lr = degrade_on_gpu(pair, (H, W), scale, mask, device,
                                    cutblur=col.cutblur, rng=rng, jpeg=getattr(col, "jpeg", None), psf=getattr(col, "psf", None))
        elif isinstance(hr, (tuple, list)):
            if size is None:
                if not hasattr(col, "imgH"):
                    raise ValueError("sr_batches: a gpu_resize batch needs size=(imgH, imgW, down_sample_scale) or a loader whose "
                                     "collate_fn carries them")
                size = (col.imgH, col.imgW, col.down_sample_scale)
            H, W, scale = size
            if degrade:
                hr, lr = degrade_on_gpu(hr, (H, W), scale, mask, device, cutblur=col.cutblur, rng=random.Random(pass_key + j),
                                            jpeg=getattr(col, "jpeg", None), psf=getattr(col, "psf", None))
            else:
                hr, lr = resize_on_gpu(hr, (H, W), mask, device), resize_on_gpu(lr, (H // scale, W // scale), mask, device)
        elif hr.dtype == torch.uint8:
            hr, lr = finish_on_gpu(hr, mask, device), finish_on_gpu(lr, mask, device)
        yield hr, lr, None, labels
