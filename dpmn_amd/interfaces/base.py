"""Mirror of ``interfaces/base.py::TextBase`` restricted to the SR hot path.

Keeps the attribute names, the per-PGRM hyper-parameter string parsing (base.py:64-82, with a safe
parser instead of eval()), ``generator_init`` (base.py:127-198) and the checkpoint format
(base.py:328-373), and the CRNN recogniser of the word accuracy (``CRNN_init`` / ``parse_crnn_data``, base.py:411-425) on the
native NativeCRNN, the ASTER recogniser (``Aster_init`` / ``parse_aster_data``, base.py:427-450) on the native NativeASTER, the MORAN
recogniser (``MORAN_init`` / ``parse_moran_data`` / ``converter_moran``, base.py:60-61, 375-409) on the native NativeMORAN, and the
comparison images (``tripple_display`` / ``test_display``, base.py:275-326) on one ``ops.display_triple`` launch.  Ours: the
training-state file that lets an interrupted run continue (``write_train_state`` / ``read_train_state``, the structure fingerprint,
``rng_capture`` / ``rng_restore``; used by ``TextSR.train(state_path=...)``).  Out of scope here: the pygame
renderer.
"""
import os

import torch

from ..model import pgrm, cmm, tsrn, tatt, tbsrn
from ..model.native import frozen as _frozen
from ..utils import ssim_psnr
from ..utils.jpeg import jpeg_setting
from ..utils.psf import psf_setting


def parse_list(s):
    """'2,4,8,' -> [2, 4, 8]; replaces eval() of base.py:64-82."""
    out = []
    for tok in str(s).split(','):
        tok = tok.strip()
        if tok:
            out.append(float(tok) if ('.' in tok or 'e' in tok.lower()) else int(tok))
    return out


def _val_weights(config, key, path, what):
    """The weights file of a recogniser: `path`, or config.TRAIN.VAL.<key> when it is None.  A missing or empty path raises: an
    untrained recogniser never produces an accuracy."""
    val = getattr(config.TRAIN, "VAL", None)
    model_path = (getattr(val, key, None) if val is not None else None) if path is None else path
    if not model_path or not os.path.isfile(model_path):
        raise FileNotFoundError("dpmn_amd: the %s recogniser needs its weights: config TRAIN.VAL.%s (or the path "
                                "argument) names no file (%r)" % (what, key, model_path))
    return model_path


# --------------------------------------------------------------------------------------------------- training state (ours)
# One file that lets an interrupted run continue bit for bit (TextSR.train(state_path=...), main.py --train_state): every model's and
# DistillModule's state_dict, the trainer's Adam state, the loop's bookkeeping and the random streams a step draws from.  The file
# holds tensors and plain Python values only, so it loads with torch.load(weights_only=True).
TRAIN_STATE_VERSION = 1
FINGERPRINT_FIELDS = ("arch", "stu_iter_b1", "stu_iter_b2", "sr_share", "patch_size", "embed_dim", "depths", "num_heads", "window_size",
                      "window_num", "mlp_ratio", "height", "width", "manmade_degrade", "cutblur", "train_hr_dir", "jpeg_degrade", "ema", "train_words",
                      "psf_blur")
# booleans, jpeg_degrade: None or [lo, hi, prob], psf_blur: None or [kinds, prob, frac] of utils.psf.psf_setting, ema: None or the decay
# of the averaged weights, and train_words: None or the dict of
# utils.render.words_setting (crc32 of the word list, sorted font names, epoch size; with --train_words_fx, and only then, its kinds, its
# probability and the crc32 of the background pool: a state written without them loads into a run without them, any difference is
# refused); a state written before they existed has them off
DATA_FIELDS = ("manmade_degrade", "cutblur", "train_hr_dir", "jpeg_degrade", "ema", "train_words", "psf_blur")


def state_fingerprint(args, config, ema=None, train_words=None):
    """What decides the structure of the trained models: a state is only ever loaded into a run with the same values.
    ema: the decay TextSR.train(ema_decay=...) averages the weights with (main.py --ema), None = off.
    train_words: the setting TextSR.train(train_words=...) renders its HR images from (main.py --train_words), None = off."""
    fp = {k: getattr(args, k) for k in ("arch", "stu_iter_b1", "stu_iter_b2", "window_num")}
    fp["sr_share"] = bool(args.sr_share)
    for k in ("patch_size", "embed_dim", "depths", "num_heads", "window_size", "mlp_ratio"):
        fp[k] = parse_list(getattr(args, k))
    fp["height"], fp["width"] = int(config.TRAIN.height), int(config.TRAIN.width)
    # where the LR images come from: a run with synthesised LR images only continues a run of the same kind
    fp["manmade_degrade"], fp["cutblur"] = degrade_flags(args)
    fp["train_hr_dir"] = bool(getattr(args, "train_hr_dir", None))
    jpeg = jpeg_setting(args)
    fp["jpeg_degrade"] = None if jpeg is None else list(jpeg)
    psf = psf_setting(args)
    fp["psf_blur"] = None if psf is None else [list(psf[0]), psf[1], psf[2]]
    # the averaged weights are part of the trainer's state: a run with them only continues a run that kept them, at the same decay
    fp["ema"] = None if ema is None else float(ema)
    # the word list, fonts and epoch size decide which HR images a step sees: a run rendered from words only continues its like
    fp["train_words"] = None if not train_words else {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in dict(train_words).items()}
    return fp


def degrade_flags(args):
    """(manmade_degrade, cutblur) of the training loader: --train_hr_dir and --train_words imply --manmade_degrade."""
    return (bool(getattr(args, "manmade_degrade", False) or getattr(args, "train_hr_dir", None) or getattr(args, "train_words", None)),
            bool(getattr(args, "cutblur", False)))


def _data_field(v):
    """A DATA_FIELDS value as it is compared: off (absent, None, False) -> None, a flag -> True, a setting -> its values."""
    if not v:
        return None
    if isinstance(v, dict):
        return sorted((k, list(x) if isinstance(x, (list, tuple)) else x) for k, x in v.items())
    return v if isinstance(v, (bool, float)) else [list(x) if isinstance(x, (list, tuple)) else x for x in v]


def check_fingerprint(saved, current, path=""):
    for k in FINGERPRINT_FIELDS:
        if (_data_field(saved.get(k)) != _data_field(current.get(k))) if k in DATA_FIELDS else (saved.get(k) != current.get(k)):
            raise ValueError("dpmn_amd: training state %s was written by a run with %s = %r, this run has %s = %r"
                             % (path, k, saved.get(k), k, current.get(k)))


def write_train_state(path, obj):
    """Atomic: the bytes go to PATH.tmp in the same directory, are flushed and fsync'ed, and only then take PATH's name -- a save
    that dies part-way leaves the previous file in place."""
    tmp = path + ".tmp"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(tmp, "wb") as f:
        torch.save(obj, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def read_train_state(path, fingerprint=None):
    """The state at `path` (never PATH.tmp: a leftover of a save that died), on the CPU.  The format version and, when given, the
    structure fingerprint are checked before the caller loads anything."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict) or state.get("version") != TRAIN_STATE_VERSION:
        raise ValueError("dpmn_amd: %s is not a training state of format version %d (found %r)"
                         % (path, TRAIN_STATE_VERSION, state.get("version") if isinstance(state, dict) else type(state).__name__))
    if fingerprint is not None:
        check_fingerprint(state["fingerprint"], fingerprint, path)
    return state


def rng_capture(device=None):
    """The random streams a training step draws from: torch's CPU generator (train/pgrm_train.py draw_seeds: the Dropout / DropPath
    seeds), numpy's global state (rotate_pair), Python's random, torch's device generator."""
    import random
    import numpy as np
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    ver, internal, gauss_next = random.getstate()
    return {"torch": torch.get_rng_state(), "numpy": (kind, torch.from_numpy(keys.astype("int64")), int(pos), int(has_gauss), float(gauss)),
            "python": (ver, tuple(internal), gauss_next),
            "device": torch.cuda.get_rng_state(device) if device is not None and device.type == "cuda" else None}


def rng_restore(state, device=None):
    import random
    import numpy as np
    torch.set_rng_state(state["torch"])
    kind, keys, pos, has_gauss, gauss = state["numpy"]
    np.random.set_state((kind, keys.numpy().astype("uint32"), pos, has_gauss, gauss))
    ver, internal, gauss_next = state["python"]
    random.setstate((ver, tuple(internal), gauss_next))
    if state.get("device") is not None and device is not None and device.type == "cuda":
        torch.cuda.set_rng_state(state["device"], device)


class TextBase(object):
    def __init__(self, config, args, opt_TPG=None):
        self.config = config
        self.args = args
        self.scale_factor = self.config.TRAIN.down_sample_scale
        self.rec_path = getattr(args, "rec_path", None)
        self.resume = args.resume if getattr(args, "resume", None) is not None else config.TRAIN.resume
        self.batch_size = args.batch_size if args.batch_size is not None else self.config.TRAIN.batch_size
        val = getattr(config.TRAIN, "VAL", None)     # base.py:56
        self.vis_dir = args.vis_dir if getattr(args, "vis_dir", None) is not None else (getattr(val, "vis_dir", None) or "./vis")
        self.voc_type = getattr(config.TRAIN, "voc_type", None)
        if not torch.cuda.is_available():
            raise RuntimeError("dpmn_amd: the DPMN hot path needs a MI355X (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device())
        from ..utils.labelmaps import MoranLabelConverter
        self.converter_moran = MoranLabelConverter()       # base.py:60-61: digits + lowercase + '$'
        self.cal_psnr = ssim_psnr.calculate_psnr
        self.cal_ssim = ssim_psnr.SSIM()
        self.mask = self.args.mask
        self.depths = parse_list(self.args.depths)
        self.patch_size = parse_list(self.args.patch_size)
        self.embed_dim = parse_list(self.args.embed_dim)
        ws = parse_list(self.args.window_size)
        nh = parse_list(self.args.num_heads)
        self.window_size, self.num_heads = [], []
        pre = 0
        for _ in self.depths:
            self.window_size.append(ws[pre:pre + self.args.window_num])
            pre += self.args.window_num
        pre = 0
        for layer_num in self.depths:
            self.num_heads.append(nh[pre:pre + layer_num])
            pre += layer_num
        self.mlp_ratio = parse_list(self.args.mlp_ratio)
        self.drop_rate = parse_list(self.args.drop_rate)
        self.attn_drop_rate = parse_list(self.args.attn_drop_rate)
        self.drop_path_rate = parse_list(self.args.drop_path_rate)

    # ------------------------------------------------------------------ data (base.py:85-125)
    def _loader(self, dirs, test, shuffle, drop_last, shard=False, gpu_finish=True, gpu_resize=False, degrade=False, cutblur=False,
                hr_dir=None, jpeg=None, words=None, psf=None):
        """shard=True (training under torch.distributed): every rank walks its own 1/world of a per-epoch permutation
        (DistributedSampler, call `self.train_sampler.set_epoch(epoch)`) with batch_size // world samples per step, so the
        GLOBAL batch stays config.TRAIN.batch_size at the configured learning rate -- nn.DataParallel's scatter of one batch
        over the GPUs (base.py:160-162), not world x batch_size.
        gpu_resize=True (or main.py --gpu_resize; needs gpu_finish): the collate packs the decoded pixels and the bicubic resize runs on
        the GPU too (ops.resize_ragged_u8 in sr_batches), same bytes as PIL's.
        degrade=True (get_train_data with main.py --manmade_degrade; never for validation or test data): the LR images are synthesised
        from the HR images on the GPU (ops.degrade_ragged_u8 in sr_batches; cutblur=True: with cutblur), which needs gpu_finish and
        turns gpu_resize on.  hr_dir (--train_hr_dir): a folder of HR images instead of the LMDBs of `dirs` (dataset/folder.py
        FolderHR), always degraded.  jpeg=(lo, hi, prob) (--jpeg_degrade / --jpeg_prob; with degrade, training data only): JPEG
        artefacts on the synthesised LR images (ops.jpeg_roundtrip_u8 in sr_batches).  psf=(kinds, prob, frac) (--psf_blur / --psf_prob /
        --psf_radius; with degrade, training data only): a random point-spread function on the HR pixels that the LR images are synthesised
        from (ops.psf_blur_ragged_u8 in sr_batches).  words=(words, atlases, epoch size)
        (--train_words): no image data at all -- dataset/words.py WordsHR, the HR images are rendered on the GPU by sr_batches
        (ops.render_words_u8), always degraded; a fourth item, the utils.render.RenderFx of --train_words_fx (or None), makes that
        ops.render_words_fx_u8: outline, drop shadow, photo background; a fifth item, the utils.render.RenderWarp of
        --train_words_warp (or None), makes it ops.render_words_warp_u8: projective distortion, rotation, curved baseline."""
        from ..dataset import textzoom as tz
        cfg = self.config.TRAIN
        degrade = bool(degrade or hr_dir or words)
        if degrade and not gpu_finish:
            raise ValueError("dpmn_amd: manmade_degrade makes the LR images on the GPU: it needs gpu_finish=True")
        if words:
            from ..dataset.words import WordsHR
            sets = [WordsHR(words[0], words[2])]
        elif hr_dir:
            from ..dataset.folder import FolderHR
            sets = [FolderHR(hr_dir, voc_type=cfg.voc_type)]
        else:
            sets = [tz.lmdbDataset_real(root=d, voc_type=cfg.voc_type, max_len=cfg.max_len, test=test, cutblur=cutblur,
                                        manmade_degrade=degrade) for d in dirs]
        ds = torch.utils.data.ConcatDataset(sets)
        dist = torch.distributed
        world = dist.get_world_size() if (shard and dist.is_initialized()) else 1
        sampler, bs = None, self.batch_size
        if world > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=dist.get_rank(), shuffle=shuffle,
                                                                      drop_last=drop_last)
            bs = max(self.batch_size // world, 2)       # B_local = 1 changes SKConv's squeeze() semantics (quirk Q3)
        loader = torch.utils.data.DataLoader(
            ds, batch_size=bs, shuffle=shuffle and sampler is None, sampler=sampler, num_workers=int(cfg.workers), pin_memory=True,
            drop_last=drop_last,
            collate_fn=tz.alignCollate_realWTLAMask(imgH=cfg.height, imgW=cfg.width, down_sample_scale=cfg.down_sample_scale, mask=self.mask,
                                                    gpu_finish=gpu_finish,      # True: ToTensor + mask channel on the GPU by sr_batches
                                                    gpu_resize=gpu_finish and (gpu_resize or degrade or bool(getattr(self.args, "gpu_resize", False))),
                                                    degrade=degrade, cutblur=cutblur, jpeg=jpeg, psf=psf,
                                                    render=(words[0], words[1]) if words else None,
                                                    render_fx=words[3] if words and len(words) > 3 else None,
                                                    render_warp=words[4] if words and len(words) > 4 else None))
        # (dataset/textzoom.py; uint8 pixels in the batch); False: the reference's float (B, 3 + mask, H, W) tensors for consumers that
        # iterate the loader themselves
        if shard:
            self.train_sampler = sampler
        return ds, loader

    def get_train_data(self, train_words=None):
        """train_words (main.py --train_words): (words, atlases, epoch size[, fx[, warp]]) -- the filtered word list,
        utils.render.build_atlases of the fonts, the number of samples that counts as one epoch and, optionally, the
        utils.render.RenderFx of --train_words_fx (or None) and the utils.render.RenderWarp of --train_words_warp; the training set is
        then rendered from it."""
        cfg = self.config.TRAIN
        degrade, cutblur = degrade_flags(self.args)
        hr_dir = getattr(self.args, "train_hr_dir", None)
        jpeg, psf = jpeg_setting(self.args), psf_setting(self.args)
        if train_words is not None:
            if hr_dir:
                raise ValueError("dpmn_amd: train_words and train_hr_dir are two sources of the HR images; give one")
            return self._loader([], False, True, True, shard=True, degrade=True, cutblur=cutblur, jpeg=jpeg, words=tuple(train_words),
                                psf=psf)
        if hr_dir:
            return self._loader([], False, True, True, shard=True, degrade=True, cutblur=cutblur, hr_dir=hr_dir, jpeg=jpeg, psf=psf)
        if not isinstance(cfg.train_data_dir, list):
            raise TypeError('check trainRoot')
        return self._loader(cfg.train_data_dir, False, True, True, shard=True, degrade=degrade, cutblur=cutblur, jpeg=jpeg,
                            psf=psf)

    def get_val_data(self):
        pairs = [self.get_test_data(d) for d in self.config.TRAIN.VAL.val_data_dir]
        return [p[0] for p in pairs], [p[1] for p in pairs]

    def get_test_data(self, dir_):
        return self._loader([dir_], True, True, False)

    def generator_init(self, iter=0, mode=True, psn=False, hidden_size=64, testing=False):
        cfg = self.config.TRAIN
        kw = dict(scale_factor=self.scale_factor, width=cfg.width, height=cfg.height, STN=self.args.STN, mask=self.mask,
                  srb_nums=self.args.srb, hidden_units=self.args.hd_u)
        if psn and self.args.arch in ('tsrn', 'tg'):
            model = tsrn.TSRN(**kw)
        elif psn and self.args.arch == 'tatt':
            model = tatt.TSRN_TL_TRANS(**kw)
        elif psn and self.args.arch == 'tbsrn':
            model = tbsrn.TBSRN(**kw)
        elif psn and self.args.arch == 'tpgsr':       # base.py:141-144
            model = tsrn.TSRN_TL(**kw)
        elif psn:
            raise NotImplementedError("dpmn_amd: PSN arch %r is not built (built: tsrn, tg, tatt, tbsrn, tpgsr)" % self.args.arch)
        else:
            # base.py:151 never passes img_size, so the reference PGRM is hard-wired to 32x128 outputs (weight_list_i is
            # (1, hidden, 32, 128), pgrm.py:497, quirk Q7).  Here the size follows the config (height x width), which is the
            # identical call for the 32x128 recipe and lets the 64x256 stress configuration run at all.
            model = pgrm.PGRM(img_size=[cfg.height, cfg.width],
                              patch_size=self.patch_size, embed_dim=self.embed_dim, depths=self.depths,
                              num_heads=self.num_heads, window_size=self.window_size, mlp_ratio=self.mlp_ratio,
                              drop_rate=self.drop_rate, attn_drop_rate=self.attn_drop_rate,
                              drop_path_rate=self.drop_path_rate, iter=iter, mode=mode, hidden_size=hidden_size)
        from ..loss.image_loss import ImageLoss
        image_crit = ImageLoss(gradient=self.args.gradient, loss_weight=[1, 1])
        model = model.to(self.device)
        if self.resume and (psn or testing):
            if os.path.isdir(self.resume):
                name = "model_{}.pth".format(self.args.arch) if psn else "model_best_" + str(iter) + ".pth"
                path = os.path.join(self.resume, name)
            else:
                path = self.resume
            print('loading pre-trained model from %s ' % path)
            model.load_state_dict(torch.load(path, map_location=self.device)['state_dict_G'])
        return {'model': model, 'crit': image_crit}

    def CRNN_init(self, path=None):
        """base.py:411-417: CRNN(32, 1, 37, 256) from config.TRAIN.VAL.crnn_pretrained (or `path`), here the native NativeCRNN,
        frozen and in eval mode.  A missing or empty path raises: an untrained recogniser never produces an accuracy."""
        from ..model.crnn import NativeCRNN
        model_path = _val_weights(self.config, "crnn_pretrained", path, "CRNN")
        model = NativeCRNN(32, 1, 37, 256).to(self.device)
        print('loading pretrained crnn model from %s' % model_path)
        model.load_state_dict(torch.load(model_path, map_location=self.device))
        return _frozen(model)

    def MORAN_init(self, path=None):
        """base.py:375-394: MORAN(1, 37, 256, 32, 100, BidirDecoder=True) from config.TRAIN.VAL.moran_pretrained (or `path`; a plain
        state dict, a DataParallel `module.` key prefix is stripped), here the native NativeMORAN, frozen and in eval mode.  A missing
        or empty path raises: an untrained recogniser never produces an accuracy."""
        from ..model.moran import NativeMORAN
        model_path = _val_weights(self.config, "moran_pretrained", path, "MORAN")
        model = NativeMORAN(1, 37, 256, 32, 100, BidirDecoder=True)
        print('loading pre-trained moran model from %s' % model_path)
        state_dict = torch.load(model_path, map_location='cpu')
        model.load_state_dict({k.replace("module.", ""): v for k, v in state_dict.items()})
        return _frozen(model.to(self.device))

    def parse_moran_data(self, imgs_input):
        """base.py:396-409: bicubic resize to 32x100 and ITU-601 luma (no normalisation) -> (tensor (B, 1, 32, 100), length (B) int32
        = 20 decode steps per image, text, text): text is the encoding of '0' * 20 per image (B * 20 zeros, int64)."""
        from ..model.moran import MAX_ITER, MORAN
        batch_size = imgs_input.shape[0]
        if imgs_input.is_cuda:
            from .. import ops
            tensor = ops.moran_prep(imgs_input.float(), 32, 100)[0]
        else:
            tensor = MORAN.parse_moran_data(imgs_input)
        text, lens = self.converter_moran.encode(['0' * MAX_ITER] * batch_size)
        return tensor, lens.to(torch.int32), text, text

    def Aster_init(self, path=None):
        """base.py:427-439: the ASTER recogniser from config.TRAIN.VAL.rec_pretrained (or `path`; the checkpoint's 'state_dict'),
        here the native NativeASTER, frozen and in eval mode -> (aster, aster_info).  A missing or empty path raises."""
        from ..model.aster import NativeASTER
        from ..utils.labelmaps import AsterInfo
        model_path = _val_weights(self.config, "rec_pretrained", path, "ASTER")
        aster_info = AsterInfo(getattr(self.config.TRAIN, "voc_type", None) or 'all')
        aster = NativeASTER(arch='ResNet_ASTER', rec_num_classes=aster_info.rec_num_classes, sDim=512, attDim=512,
                            max_len_labels=aster_info.max_len, eos=aster_info.char2id[aster_info.EOS], STN_ON=True)
        aster.load_state_dict(torch.load(model_path, map_location='cpu')['state_dict'])
        print('load pre_trained aster model from %s' % model_path)
        aster = aster.to(self.device)
        aster.info = aster_info
        return _frozen(aster), aster_info

    def parse_aster_data(self, imgs_input):
        """base.py:441-450: images in [0, 1] -> the recogniser's input dict (images in [-1, 1], targets filled with ones)."""
        from ..utils.labelmaps import AsterInfo
        aster_info = AsterInfo(getattr(self.config.TRAIN, "voc_type", None) or 'all')
        images_input = imgs_input.to(self.device)
        batch_size = images_input.shape[0]
        return {'images': images_input * 2 - 1, 'rec_targets': torch.IntTensor(batch_size, aster_info.max_len).fill_(1),
                'rec_lengths': [aster_info.max_len] * batch_size}

    def parse_crnn_data(self, imgs_input):
        """base.py:419-425: bicubic resize to 32x100 and ITU-601 luma -> (B, 1, 32, 100), a view of the NHWC buffer NativeCRNN's
        first conv reads (dpmn_gray_prep_f32; channels 0..2 of the input are read)."""
        from .. import ops
        return ops.crnn_prep(imgs_input.float(), 32, 100)[..., 0:1].permute(0, 3, 1, 2)

    # ------------------------------------------------------------------ comparison images (base.py:275-326)
    def _write_triples(self, out_dir, image_in, image_out, image_target, sel, names):
        """The PNGs of the images `sel` under out_dir: ONE ops.display_triple launch, ONE device-to-host copy, PIL only encodes
        (Image.fromarray(arr).save(path) is what torchvision's save_image ends in).  A later equal name overwrites an earlier one."""
        if not sel:
            return
        from PIL import Image
        from .. import ops
        arr = ops.display_triple(image_in, image_out, image_target, sel).cpu().numpy()
        os.makedirs(out_dir, exist_ok=True)
        for a, name in zip(arr, names):
            Image.fromarray(a).save(os.path.join(out_dir, name))

    def tripple_display(self, image_in, image_out, image_target, pred_str_lr, pred_str_sr, label_strs, index):
        """base.py:275-298: the first min(B, TRAIN.VAL.n_vis) images of the batch as <vis_dir>/<index>/<LR string>_<SR string>_
        <label>_.png, each the bicubically enlarged LR input over the SR output over the HR target (channels 0..2)."""
        from ..utils.display import image_name
        val = getattr(self.config.TRAIN, "VAL", None)
        n_vis = getattr(val, "n_vis", None) if val is not None else None
        n = min(image_in.shape[0], 10 if n_vis is None else int(n_vis))      # (10: config/super_resolution.yaml)
        names = [image_name(pred_str_lr[i], pred_str_sr[i], label_strs[i]) for i in range(n)]
        self._write_triples(os.path.join(self.vis_dir, str(index)), image_in, image_out, image_target, list(range(n)), names)

    def test_display(self, image_in, image_out, image_target, pred_str_lr, pred_str_sr, label_strs, str_filt):
        """base.py:300-326: the images whose filtered SR string differs from the filtered label, as <vis_dir>/display/<filtered LR
        string>_<filtered SR string>_<filtered label>_.png -> their number."""
        from ..utils.display import image_name
        sel = [i for i in range(image_in.shape[0]) if str_filt(pred_str_sr[i], 'lower') != str_filt(label_strs[i], 'lower')]
        names = [image_name(str_filt(pred_str_lr[i], 'lower'), str_filt(pred_str_sr[i], 'lower'), str_filt(label_strs[i], 'lower'))
                 for i in sel]
        self._write_triples(os.path.join(self.vis_dir, 'display'), image_in, image_out, image_target, sel, names)
        return len(sel)

    def save_checkpoint(self, netG_list, epoch, iters, best_acc_dict, best_model_info, is_best, converge_list,
                        recognizer=None, metric="sum", trainer=None):
        """Same files and dict keys as base.py:328-358: model_best_{metric}_{epoch}_{i}.pth when is_best, otherwise every
        model overwrites checkpoint.pth (the reference's behaviour, line 358).  Recogniser files (base.py:360-373) are written
        when a recogniser list is passed.  trainer (ours): the train/optim.py Trainer that owns the parameters -- its pending
        ZeRO-1 parameter all-gathers are awaited before any state_dict is cloned (they write the flat parameter arena from
        RCCL's stream; a clone racing them would store step t-1 values for the shards other ranks own)."""
        if trainer is not None:
            trainer.sync_params()
        ckpt_path = os.path.join(self.vis_dir, 'ckpt')
        os.makedirs(ckpt_path, exist_ok=True)
        for i, netG in enumerate(netG_list):
            # parameters may be views into the trainer's flat buckets: store compact, storage-independent copies
            save_dict = {'state_dict_G': {k: v.detach().clone() for k, v in netG.state_dict().items()},
                         'info': {'arch': self.args.arch, 'iters': iters, 'epochs': epoch, 'batch_size': self.batch_size,
                                  'voc_type': getattr(self, "voc_type", None), 'up_scale_factor': self.scale_factor},
                         'best_history_res': best_acc_dict, 'best_model_info': best_model_info,
                         'param_num': sum(p.numel() for p in netG.parameters()), 'converge': converge_list}
            fname = 'model_best_{}_{}_{}.pth'.format(metric, epoch, i) if is_best else 'checkpoint.pth'
            torch.save(save_dict, os.path.join(ckpt_path, fname))
        if recognizer is not None:
            recs = recognizer if isinstance(recognizer, list) else [recognizer]
            for i, r in enumerate(recs):
                if isinstance(recognizer, list):
                    fname = ('recognizer_best_{}_{}_{}.pth' if is_best else 'recognizer_{}_{}_{}.pth').format(metric, epoch, i)
                else:
                    fname = 'recognizer_best.pth' if is_best else 'recognizer.pth'
                torch.save(r.state_dict(), os.path.join(ckpt_path, fname))
        return ckpt_path
