"""Host side of the ragged-batch resize (dpmn_amd/utils/resize.py, dpmn_amd/dataset/folder.py) against PIL itself: the general
coefficient tables, the numpy restatement of the two passes for enlarging and shrinking, the packing of a ragged batch and the host
half of the folder reader.  No GPU."""
import numpy as np
import pytest
import torch
from PIL import Image

from dpmn_amd.utils import resize
from helpers import pil_bicubic_tables

# (h, w) -> (H, W): shrinking and enlarging on either axis, mixed, extreme aspect ratios, one pixel, equal sizes
PAIRS = [((43, 157), (32, 128)), ((19, 73), (16, 64)), ((55, 185), (32, 128)), ((23, 85), (16, 64)), ((7, 300), (16, 64)),
         ((120, 9), (16, 64)), ((33, 64), (16, 64)), ((16, 700), (32, 128)), ((200, 900), (16, 64)), ((1, 1), (16, 64)),
         ((5, 5), (32, 128)), ((16, 64), (16, 64))]


def images(shape, seed):
    """A random image and a 0 / 255 image (the overshoot of the cubic is largest at hard edges) of one shape."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 256, shape + (3,)).astype(np.uint8), (rng.randint(0, 2, shape + (3,)) * 255).astype(np.uint8))


def pil_resize(img, H, W):
    return np.asarray(Image.fromarray(img).resize((W, H), Image.BICUBIC))


@pytest.mark.parametrize("src,dst", PAIRS)
def test_pil_resize_u8_equals_pil(src, dst):
    for img in images(src, 11 + src[0]):
        got = resize.pil_resize_u8(img, *dst)
        assert got.dtype == np.uint8 and got.shape == dst + (3,)
        assert int((got != pil_resize(img, *dst)).sum()) == 0


def test_tables_equal_the_enlarging_tables_and_are_monotone_and_bounded():
    """The vectorised tables against the per-index restatement of Resample.c (helpers.pil_bicubic_tables), then their invariants."""
    for insz, outsz in [(1, 1), (1, 16), (5, 32), (16, 16), (16, 32), (19, 64), (64, 64), (64, 128), (73, 128), (157, 128), (8192, 1)]:
        assert np.array_equal(resize.pil_resample_tables(insz, outsz), pil_bicubic_tables(insz, outsz))
    sizes = sorted({s for pair in PAIRS for s in pair[0]} | {2, 3, 8192})      # 8192 -> 1: the widest kernel pack_ragged admits
    for insz in sizes:
        for outsz in ((1, 128) if insz == 8192 else (1, 16, 32, 64, 128)):
            tab = resize.pil_resample_tables(insz, outsz)
            scale = max(insz / outsz, 1.0)
            assert tab.dtype == np.int32 and tab.shape == (outsz, 2 + 2 * int(np.ceil(2 * scale)) + 1) and not tab.flags.writeable
            xmin, n = tab[:, 0].astype(np.int64), tab[:, 1].astype(np.int64)
            assert xmin.min() >= 0 and n.min() >= 1 and (xmin + n).max() <= insz and n.max() <= tab.shape[1] - 2
            assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all()
            k = tab[:, 2:].astype(np.int64)
            assert all((k[i, n[i]:] == 0).all() for i in range(outsz))
            assert abs(k.sum(1) - (1 << 22)).max() <= tab.shape[1]      # normalised weights, one rounding of half a unit per tap
            assert 255 * int(np.abs(k).sum(1).max()) + (1 << 21) < 2 ** 31      # int32 accumulation holds
    assert resize.pil_resample_tables(157, 128) is resize.pil_resample_tables(157, 128)
    with pytest.raises(ValueError):
        resize.pil_resample_tables(0, 16)


def test_pack_ragged_round_trip_and_rejections():
    imgs = [images(src, 5)[0] for src, _ in PAIRS]
    packed, meta = resize.pack_ragged(imgs)
    assert packed.dtype == torch.uint8 and packed.dim() == 1 and packed.numel() == sum(a.size for a in imgs)
    assert tuple(meta.shape) == (len(imgs), 3) and meta.dtype in (torch.int32, torch.int64)
    flat = packed.numpy()
    for (off, h, w), a in zip(meta.tolist(), imgs):
        assert (h, w) == a.shape[:2] and np.array_equal(flat[off:off + h * w * 3].reshape(h, w, 3), a)
    assert meta[:, 0].tolist() == np.concatenate(([0], np.cumsum([a.size for a in imgs])[:-1])).tolist()
    ok = np.zeros((4, 4, 3), np.uint8)
    big = np.broadcast_to(np.zeros((1, 1, 3), np.uint8), (8192, 8192, 3))      # 192 MiB of pixels without the memory
    for bad in ([ok, np.zeros((0, 4, 3), np.uint8)], [np.zeros((4, 0, 3), np.uint8)], [ok, np.broadcast_to(ok[:1, :1], (8193, 1, 3))],
                [np.broadcast_to(ok[:1, :1], (1, 8193, 3))], [big] * 11, [], [np.zeros((4, 4), np.uint8)], [np.zeros((4, 4, 3), np.float32)]):
        with pytest.raises(ValueError):
            resize.pack_ragged(bad)
    assert 10 * big.size <= resize.MAX_PACKED_BYTES < 11 * big.size


def test_folder_host_batches_decode_order_and_skipping(tmp_path, capsys):
    from dpmn_amd.dataset import folder
    rng = np.random.RandomState(3)
    rgb = rng.randint(0, 256, (9, 31, 3)).astype(np.uint8)
    gray = rng.randint(0, 256, (12, 20)).astype(np.uint8)
    rgba = rng.randint(0, 256, (7, 15, 4)).astype(np.uint8)
    pal = Image.fromarray(rgb).convert("P", palette=Image.ADAPTIVE, colors=16)
    Image.fromarray(rgb).save(tmp_path / "d_rgb.png")
    Image.fromarray(gray).save(tmp_path / "b_gray.png")
    Image.fromarray(rgba).save(tmp_path / "c_rgba.png")
    pal.save(tmp_path / "a_pal.png")
    (tmp_path / "notes.txt").write_text("not an image")
    (tmp_path / "broken.png").write_bytes(b"\x89PNG\r\n\x1a\n" + b"\0" * 16)
    (tmp_path / "sub").mkdir()
    Image.fromarray(rgb).save(tmp_path / "sub" / "inside.png")      # directories are not walked
    batches = list(folder.host_batches(str(tmp_path), 3))
    printed = capsys.readouterr().out.splitlines()
    assert [b[0] for b in batches] == [["a_pal.png", "b_gray.png", "c_rgba.png"], ["d_rgb.png"]]
    assert len(printed) == 2 and "broken.png" in printed[0] and "notes.txt" in printed[1]
    expected = {"a_pal.png": np.asarray(pal.convert("RGB")), "b_gray.png": np.stack([gray] * 3, -1), "c_rgba.png": rgba[..., :3],
                "d_rgb.png": rgb}
    for names, packed, meta in batches:
        for name, (off, h, w) in zip(names, meta.tolist()):
            assert np.array_equal(packed.numpy()[off:off + h * w * 3].reshape(h, w, 3), expected[name]), name
    empty = tmp_path / "sub" / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError):
        next(folder.host_batches(str(empty), 2))
