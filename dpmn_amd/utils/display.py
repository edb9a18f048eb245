"""Host side of the LR / SR / HR comparison images (``tripple_display`` / ``test_display``, interfaces/base.py:275-326 of the
reference): the two quantisations, a numpy restatement of the whole triple (the CPU
reference of ``ops.display_triple``, csrc/display.hip) and the file-name rule.  No torch, no GPU: importable on any machine.

The LR rows are PIL's fixed-point bicubic resize of ``utils/resize.py`` (``pil_resize_u8``), enlarging only.
"""
import numpy as np

from .resize import pil_resize_u8


def quantize_lr(x):
    """ToPILImage on a float tensor: x.mul(255).byte() -- one float32 multiply, then truncation.  Values outside [0, 1] (undefined in
    the reference: a float -> uint8 cast out of range) are clamped to [0, 255] first; NaN gives 0."""
    v = np.asarray(x, np.float32) * np.float32(255.0)
    return np.clip(np.nan_to_num(v, nan=0.0), 0.0, 255.0).astype(np.uint8)


def quantize_sr(x):
    """torchvision save_image: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- two separately rounded float32 operations (no FMA),
    then truncation.  NaN gives 0."""
    v = np.asarray(x, np.float32) * np.float32(255.0)
    v = v + np.float32(0.5)
    return np.clip(np.nan_to_num(v, nan=0.0), 0.0, 255.0).astype(np.uint8)


def triple_reference(image_in, image_out, image_target, sel):
    """The CPU restatement of ops.display_triple on numpy arrays: (B, >=3, h, w), (B, >=3, H, W) x 2, indices -> (n, 3 H, W, 3)
    uint8.  The enlarged LR passes ToTensor (/ 255) and save_image's quantisation again in the reference: the identity on 0..255."""
    image_in, image_out, image_target = (np.asarray(a, np.float32) for a in (image_in, image_out, image_target))
    H, W = image_target.shape[-2:]
    out = np.empty((len(sel), 3 * H, W, 3), np.uint8)
    for j, b in enumerate(sel):
        out[j, :H] = pil_resize_u8(quantize_lr(image_in[b, :3]).transpose(1, 2, 0), H, W)
        out[j, H:2 * H] = quantize_sr(image_out[b, :3]).transpose(1, 2, 0)
        out[j, 2 * H:] = quantize_sr(image_target[b, :3]).transpose(1, 2, 0)
    return out


def image_name(pred_lr, pred_sr, label):
    """base.py:296-297 / 323-324: '<LR string>_<SR string>_<label>_.png' with every '/' removed (the strings come from a
    recogniser and from the data set: a '/' would name a directory)."""
    return (str(pred_lr) + '_' + str(pred_sr) + '_' + str(label) + '_.png').replace('/', '')
