"""HR text crops from a word list on the CPU (utils/render.py, dataset/words.py, main.py --train_words): the draws of a sample, the
NumPy restatement against PIL, the word-file reader and the flag conflicts, the --train_state fingerprint, and sr_batches over a WordsHR
loader with the device ops replaced by their NumPy restatements."""
import importlib.util
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dpmn_amd.utils import render as rd
from dpmn_amd.utils.resize import MAX_SIDE, pack_ragged, pil_resize_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = ["hello", "World", "a", "x" * 25, "it's", "42nd"]
_ATLASES = {}


def _atlases():
    """PIL's built-in font at the base heights 64 and 40 as two atlases: made once, never changed"""
    if not _ATLASES:
        _ATLASES["a"] = rd.build_atlases(None, [64, 40])
    return _ATLASES["a"]


class Counting(random.Random):
    """a random.Random that counts the calls draw_render may make"""

    def __init__(self, seed):
        super().__init__(seed)
        self.n_random = self.n_bits = 0

    def random(self):
        self.n_random += 1
        return super().random()

    def getrandbits(self, k):
        self.n_bits += 1
        return super().getrandbits(k)


# -------------------------------------------------------------------------------------------------------------------------- draws
def test_draw_render_is_deterministic_counts_its_draws_and_stays_in_range():
    at = _atlases()
    a = rd.draw_render(WORDS, 2, random.Random(7), n=300)
    b = rd.draw_render(WORDS, 2, random.Random(7), n=300)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    c = rd.draw_render(WORDS, 2, random.Random(8), n=300)
    assert not np.array_equal(a[3], c[3])
    labels, cls, lens, p = a
    assert cls.shape == (300, 25) and cls.dtype == np.int32 and lens.dtype == np.int32 and p.shape == (300, rd.N_PARAMS) and p.dtype == np.int64
    assert set(labels) <= set(WORDS) and [WORDS[i] for i in p[:, rd.WORD]] == labels and set(p[:, rd.WORD]) == set(range(len(WORDS)))
    assert [len(w) for w in labels] == lens.tolist()
    # every column in its documented range, and the ranges are reached
    assert set(p[:, rd.FONT]) == {0, 1} and set(p[:, rd.CASE]) == {0, 1, 2} and set(p[:, rd.STYLE]) == {0, 1, 2}
    assert p[:, rd.GH].min() >= 24 and p[:, rd.GH].max() <= 64 and (p[:, rd.GH] % 2 == 0).all() and {24, 64} <= set(p[:, rd.GH])
    assert set(p[:, rd.SPACING]) == {-1, 0, 1, 2, 3, 4}
    m = p[:, rd.M_LEFT:rd.M_BOTTOM + 1]
    assert m.min() == 0 and (m <= p[:, rd.GH, None] // 4).all() and m.max() == 16
    assert np.abs(p[:, rd.SHEAR]).max() <= int(0.3 * 65536) and p[:, rd.SHEAR].min() < -15000 and p[:, rd.SHEAR].max() > 15000
    assert p[:, rd.FG:rd.FG + 6].min() >= 0 and p[:, rd.FG:rd.FG + 6].max() <= 255 and p[:, rd.BG2:rd.BG2 + 3].max() <= 255
    assert all(abs(rd.luma(r[rd.FG:rd.FG + 3]) - rd.luma(r[rd.BG:rd.BG + 3])) >= 64 for r in p)
    assert p[:, rd.SEED].min() >= 0 and p[:, rd.SEED].max() < 2 ** 63 and len(set(p[:, rd.SEED])) == 300
    # a fixed number of draws per sample beside the contrast redraw: 14 + 6 per colour attempt random(), one getrandbits
    for n in (1, 5, 40):
        rng = Counting(3)
        rd.draw_render(WORDS, 2, rng, n=n)
        assert rng.n_bits == n and rng.n_random >= (rd.FIXED_DRAWS + 6) * n and (rng.n_random - rd.FIXED_DRAWS * n) % 6 == 0
    one = Counting(11)
    rd.draw_render(WORDS, 2, one, n=1)
    many = Counting(11)
    rd.draw_render(WORDS, 2, many, n=2)
    first = rd.draw_render(WORDS, 2, random.Random(11), n=1)[3]
    assert np.array_equal(rd.draw_render(WORDS, 2, random.Random(11), n=2)[3][:1], first) and many.n_random > one.n_random
    # sizes: the images of the draws, and the clamp at absurd margins
    meta = rd.render_meta(cls, lens, p, at)
    assert meta[:, 1:].min() >= 1 and meta[:, 1:].max() <= MAX_SIDE and meta[0, 0] == 0
    assert np.array_equal(meta[1:, 0], np.cumsum(meta[:-1, 1] * meta[:-1, 2] * 3))
    assert np.array_equal(meta[:, 1], p[:, rd.GH] + p[:, rd.M_TOP] + p[:, rd.M_BOTTOM])
    big = p[:1].copy()
    big[0, rd.M_LEFT] = big[0, rd.M_TOP] = MAX_SIDE
    assert tuple(rd.render_meta(cls[:1], lens[:1], big, at)[0, 1:]) == (MAX_SIDE, MAX_SIDE)
    with pytest.raises(ValueError):
        rd.draw_render([], 1, random.Random(1))
    bad = p[:1].copy()
    bad[0, rd.FONT] = 2
    with pytest.raises(ValueError, match="font"):
        rd.render_meta(cls[:1], lens[:1], bad, at)


# ----------------------------------------------------------------------------------------------------------------- against PIL
def _row(font, gh, fg=(200, 30, 90), bg=(10, 220, 130), **kw):
    row = np.zeros(rd.N_PARAMS, np.int64)
    row[rd.FONT], row[rd.GH] = font, gh
    row[rd.FG:rd.FG + 3], row[rd.BG:rd.BG + 3] = fg, bg
    for k, v in kw.items():
        row[getattr(rd, k)] = v
    return row


def _grained(bg, seed, h, w):
    return np.clip(np.asarray(bg)[None, None] + rd.grain(seed, h * w).reshape(h, w, 1), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("font,gh", [(0, 64), (1, 40)])
def test_single_glyph_equals_pil_composite(font, gh):
    """no shear, no spacing, flat background, atlas height = gh: the image is Image.composite of fg over the (grained) bg with the
    glyph's own alpha, byte for byte -- the bilinear sample reads the atlas byte itself and the blend is PIL's"""
    from PIL import Image
    at = _atlases()
    for ch, case in (("g", 0), ("Q", 1), ("7", 0)):
        c = rd.DICT36.index(ch.lower()) + 1
        w = int(at.advance[font, case, c])
        alpha = at.alpha[font, case, c, :gh, :w]
        assert alpha.max() == 255 and 0 < (alpha > 0).mean() < 1
        for seed in (0, 2 ** 63 - 1):
            img = rd.render_u8([c], _row(font, gh, CASE=case, SEED=seed), at)
            fg = Image.new("RGB", (w, gh), (200, 30, 90))
            ref = Image.composite(fg, Image.fromarray(_grained((10, 220, 130), seed, gh, w)), Image.fromarray(alpha, "L"))
            assert img.shape == (gh, w, 3) and np.array_equal(img, np.asarray(ref))
    g = rd.grain(5, 100000)
    assert g.min() == -4 and g.max() == 4 and abs(g.mean()) < 0.05


def test_word_equals_the_glyphs_pasted_at_the_summed_advances():
    """no kerning, no ligatures: glyph k starts where the advances of the glyphs before it end"""
    from PIL import Image
    at = _atlases()
    for word, case in (("hello42", 0), ("WAVE", 1), ("Type", 2)):
        cls = rd.word_classes(word)
        planes = [1 if case == 1 or (case == 2 and k == 0) else 0 for k in range(len(cls))]
        ws = [int(at.advance[1, pl, c]) for pl, c in zip(planes, cls)]
        mask = Image.new("L", (sum(ws), 40), 0)
        x = 0
        for pl, c, a in zip(planes, cls, ws):
            mask.paste(Image.fromarray(at.alpha[1, pl, c, :40, :a], "L"), (x, 0))
            x += a
        img = rd.render_u8(cls, _row(1, 40, CASE=case, SEED=9), at)
        ref = Image.composite(Image.new("RGB", mask.size, (200, 30, 90)), Image.fromarray(_grained((10, 220, 130), 9, 40, sum(ws))), mask)
        assert np.array_equal(img, np.asarray(ref))
    # margins, spacing and shear only move the same glyphs: the flat margin rows hold the background alone
    row = _row(0, 32, M_LEFT=3, M_RIGHT=5, M_TOP=4, M_BOTTOM=2, SPACING=4, SHEAR=-19660, STYLE=2, SEED=1)
    row[rd.BG2:rd.BG2 + 3] = (250, 0, 40)
    img = rd.render_u8(rd.word_classes("ab"), row, at)
    h, w = img.shape[:2]
    assert h == 38 and np.abs(img[0].astype(int) - (10, 220, 130)).max() <= 4 and np.abs(img[-1].astype(int) - (250, 0, 40)).max() <= 4
    assert rd.word_classes("it's") == [9, 20, 0, 19]          # a character without a glyph is the blank


# --------------------------------------------------------------------------------------------------- word file, flags, fingerprint
def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_render", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_word_file_reader(tmp_path, capsys):
    f = tmp_path / "words.txt"
    f.write_text("Hello\n\n  café \n!!!\n" + "y" * 26 + "\n" + "z" * 25 + "\nit's\n", encoding="utf-8")
    assert rd.read_words(str(f), "upper") == ["Hello", "caf", "z" * 25, "its"]
    assert "4 of 7 lines" in capsys.readouterr().out
    assert rd.read_words(str(f), "lower")[0] == "hello" and rd.read_words(str(f), "all")[-1] == "it's"
    empty = tmp_path / "empty.txt"
    empty.write_text("\n???\n" + "w" * 30 + "\n")
    with pytest.raises(SystemExit, match="no usable word"):
        rd.read_words(str(empty), "upper")


def test_flag_conflicts_exit_with_one_clear_line(tmp_path):
    m = _main()
    f = tmp_path / "words.txt"
    f.write_text("word\n")
    d = tmp_path / "hr"
    d.mkdir()
    for args, msg in ((dict(train_words=str(f), train_hr_dir=str(d)), "--train_words and --train_hr_dir are two sources"),
                      (dict(train_words_fonts=str(d)), "--train_words_fonts needs --train_words"),
                      (dict(train_words=str(tmp_path / "missing.txt")), "--train_words .* is not a file"),
                      (dict(train_words=str(f), train_words_fonts=str(tmp_path / "nodir")), "--train_words_fonts .* is not a directory"),
                      (dict(train_words=str(f), train_words_fonts=str(d)), r"holds no \*.ttf / \*.otf file"),
                      (dict(train_words=str(f), train_words_epoch=0), "--train_words_epoch must be a positive")):
        with pytest.raises(SystemExit, match=msg) as e:
            m.main(SimpleNamespace(), SimpleNamespace(**args))
        assert str(e.value).startswith("main.py: ") and "\n" not in str(e.value)
    (d / "broken.ttf").write_bytes(b"not a font")
    with pytest.raises(SystemExit, match="holds no font that PIL can open"):
        m.main(SimpleNamespace(), SimpleNamespace(train_words=str(f), train_words_fonts=str(d)))
    # --cutblur and --jpeg_degrade are allowed on top of --train_words (it implies --manmade_degrade): the run gets past their checks
    src = m.train_words_source(SimpleNamespace(train_words=str(f), train_words_epoch=12), "upper")
    assert src[0] == ["word"] and src[1].n_fonts == 1 and src[1].names == ["default"] and src[2] == 12
    assert m.train_words_source(SimpleNamespace(), "upper") is None


def test_fingerprint_field(tmp_path):
    from dpmn_amd.interfaces import base
    cfg = SimpleNamespace(TRAIN=SimpleNamespace(height=32, width=128))
    args = SimpleNamespace(arch="tatt", stu_iter_b1=1, stu_iter_b2=1, window_num=3, sr_share=False, patch_size="4,", embed_dim="96,",
                           depths="1,", num_heads="6,", window_size="2,4,8,", mlp_ratio="4,")
    at = _atlases()
    off = base.state_fingerprint(args, cfg)
    assert "train_words" in off and off["train_words"] is None and "train_words" in base.FINGERPRINT_FIELDS and "train_words" in base.DATA_FIELDS
    args_on = SimpleNamespace(**dict(vars(args), train_words="words.txt"))
    setting = rd.words_setting(WORDS, at, 100)
    assert sorted(setting) == ["crc32", "epoch", "fonts"] and setting["fonts"] == ["default", "default"] and setting["epoch"] == 100
    on = base.state_fingerprint(args_on, cfg, train_words=setting)
    assert on["train_words"] == setting and on["manmade_degrade"] is True
    old = {k: v for k, v in off.items() if k != "train_words"}          # a state written before the field existed loads as off
    base.check_fingerprint(old, off)
    base.check_fingerprint(on, base.state_fingerprint(args_on, cfg, train_words=rd.words_setting(list(WORDS), at, 100)))
    path = str(tmp_path / "state.pt")
    base.write_train_state(path, {"version": base.TRAIN_STATE_VERSION, "fingerprint": on})
    assert base.read_train_state(path, on)["fingerprint"]["train_words"] == setting      # (survives the weights_only round trip)
    other_words = base.state_fingerprint(args_on, cfg, train_words=rd.words_setting(WORDS[:-1], at, 100))
    other_epoch = base.state_fingerprint(args_on, cfg, train_words=rd.words_setting(WORDS, at, 101))
    other_fonts = base.state_fingerprint(args_on, cfg, train_words=rd.words_setting(WORDS, rd.build_atlases(None, 64), 100))
    for cur in (other_words, other_epoch, other_fonts):
        with pytest.raises(ValueError, match="train_words"):
            base.read_train_state(path, cur)
    with pytest.raises(ValueError, match="manmade_degrade|train_words"):
        base.check_fingerprint(old, on)
    with pytest.raises(ValueError, match="manmade_degrade|train_words"):
        base.check_fingerprint(on, off)


# -------------------------------------------------------------------------------------------------- sr_batches with stubbed device ops
@pytest.fixture
def stub_ops(monkeypatch):
    """ops.render_words_u8 -> the NumPy restatement; the degrade chain's ops -> host stand-ins that record what they were given"""
    from dpmn_amd import ops
    calls = {"render": [], "degrade": []}

    def render(cls, lens, params, atlases, device=None, out=None):
        calls["render"].append((np.array(cls), np.array(lens), np.array(params)))
        return pack_ragged([rd.render_u8(c[:n], p, atlases) for c, n, p in zip(cls, lens, params)], pin=False)

    def degrade(packed, meta, params, z=None, seed=0):
        calls["degrade"].append((np.array(params), int(seed)))
        return packed.clone()

    def resize(packed, meta, H, W):
        flat = packed.numpy()
        return torch.from_numpy(np.stack([pil_resize_u8(flat[o:o + h * w * 3].reshape(h, w, 3), H, W) for o, h, w in np.asarray(meta).tolist()]))

    monkeypatch.setattr(ops, "render_words_u8", render)
    monkeypatch.setattr(ops, "degrade_ragged_u8", degrade)
    monkeypatch.setattr(ops, "resize_ragged_u8", resize)
    monkeypatch.setattr(ops, "collate_u8", lambda img, mask: img.permute(0, 3, 1, 2).float() / 255.0)
    return calls


def _words_loader(batch=4, epoch=6):
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.words import WordsHR
    ds = WordsHR(WORDS, epoch)
    col = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=False, gpu_finish=True, gpu_resize=True, degrade=True,
                                       cutblur=True, render=(WORDS, _atlases()))
    assert col.render is True and col.degrade is True
    return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=False, drop_last=False, collate_fn=col, num_workers=0)


def test_words_dataset_and_collate():
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.words import WordsHR
    ds = WordsHR(WORDS, 10)
    assert len(ds) == 10 and ds[7] == (None, None, None, None, WORDS[1])
    with pytest.raises(IndexError):
        ds[10]
    with pytest.raises(ValueError):
        WordsHR([], 10)
    with pytest.raises(ValueError):
        WordsHR(WORDS, 0)
    with pytest.raises(ValueError, match="degrade"):
        tz.alignCollate_realWTLAMask(gpu_finish=True, gpu_resize=True, render=(WORDS, _atlases()))
    out = next(iter(_words_loader()))
    assert len(out) == 9 and out[0] is None and out[2] is None and list(out[5]) == WORDS[:4]


def test_sr_batches_over_words_replays_from_the_restored_stream(stub_ops):
    from dpmn_amd.dataset import textzoom as tz
    dev = torch.device("cpu")
    loader = _words_loader()
    random.seed(3)
    state = random.getstate()
    a = list(tz.sr_batches(loader, dev))
    after = random.getstate()
    first = [(c.copy(), n.copy(), p.copy()) for c, n, p in stub_ops["render"]], list(stub_ops["degrade"])
    assert len(a) == 2 and [len(b[3]) for b in a] == [4, 2]
    hr, lr, lv, labels = a[0]
    assert hr.shape == (4, 3, 32, 128) and lr.shape == (4, 3, 16, 64) and lv is None and set(labels) <= set(WORDS)
    # (a) then (b) from random.Random(pass_key + j): the render draws, then exactly degrade_on_gpu's
    random.setstate(state)
    key = random.getrandbits(63)
    assert random.getstate() == after, "a pass draws once from the global stream, when it starts"
    from dpmn_amd.utils.degrade import draw_params
    for j, n in enumerate((4, 2)):
        rng = random.Random(key + j)
        want = rd.draw_render(WORDS, 2, rng, n=n)
        assert a[j][3] == want[0] and all(np.array_equal(x, y) for x, y in zip(first[0][j], want[1:]))
        widths = rd.render_meta(*want[1:], _atlases())[:, 2]
        assert np.array_equal(first[1][j][0], draw_params(n, cutblur=True, hr_widths=widths.tolist(), rng=rng))
        assert first[1][j][1] == rng.getrandbits(63)
    # a second pass from the restored state: the same words, parameters and images; another state: others
    stub_ops["render"].clear()
    random.setstate(state)
    b = list(tz.sr_batches(loader, dev))
    assert [x[3] for x in a] == [x[3] for x in b] and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    assert all(np.array_equal(p, q) for x, y in zip(first[0], stub_ops["render"]) for p, q in zip(x, y))
    random.seed(4)
    c = list(tz.sr_batches(loader, dev))
    assert not torch.equal(a[0][0], c[0][0])


def test_flagless_degrade_pass_draws_what_it_drew_before(stub_ops, tmp_path, monkeypatch):
    """A FolderHR pass (no render collate): the global stream moves by the one pass key and every batch draws exactly draw_params + the
    noise seed from random.Random(key + j) -- with utils/render never imported (the module is made unimportable for the second pass)."""
    from PIL import Image
    from dpmn_amd.dataset import textzoom as tz
    from dpmn_amd.dataset.folder import FolderHR
    from dpmn_amd.utils.degrade import draw_params
    rng = np.random.RandomState(3)
    d = tmp_path / "hr"
    d.mkdir()
    for i in range(4):
        Image.fromarray(rng.randint(0, 256, (8 + i, 20 + 3 * i, 3)).astype(np.uint8)).save(str(d / ("im%d.png" % i)))
    ds = FolderHR(str(d))
    col = tz.alignCollate_realWTLAMask(imgH=32, imgW=128, down_sample_scale=2, mask=False, gpu_finish=True, gpu_resize=True, degrade=True,
                                       cutblur=True)
    assert col.render is False
    batches = [col([ds[0], ds[1]]), col([ds[2], ds[3]])]
    loader = type("Loader", (), {"collate_fn": col, "__iter__": lambda self: iter(batches)})()
    random.seed(5)
    before = random.getstate()
    a = list(tz.sr_batches(loader, torch.device("cpu")))
    after = random.getstate()
    seen = list(stub_ops["degrade"])
    random.setstate(before)
    key = random.getrandbits(63)
    assert random.getstate() == after
    for j, (params, seed) in enumerate(seen):
        r = random.Random(key + j)
        assert np.array_equal(params, draw_params(2, cutblur=True, hr_widths=[int(w) for w in batches[j][0][1][:, 2]], rng=r))
        assert seed == r.getrandbits(63)
    assert len(stub_ops["render"]) == 0
    # the same pass where utils/render cannot be imported at all: same end state, same draws, same images
    import dpmn_amd.utils
    monkeypatch.delattr(dpmn_amd.utils, "render", raising=False)
    monkeypatch.setitem(sys.modules, "dpmn_amd.utils.render", None)
    with pytest.raises(ImportError):
        importlib.import_module("dpmn_amd.utils.render")
    stub_ops["degrade"].clear()
    random.setstate(before)
    b = list(tz.sr_batches(loader, torch.device("cpu")))
    assert random.getstate() == after
    assert all(np.array_equal(p, q) and s == t for (p, s), (q, t) in zip(seen, stub_ops["degrade"])) and len(stub_ops["degrade"]) == 2
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[3] == y[3] for x, y in zip(a, b))
