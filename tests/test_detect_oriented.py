"""The oriented part of utils/detect.py (main.py --demo_detect_oriented): the table of directions against its formula, the tables against
brute-force loops, the upright special case against boxes_from_components, and rotated rectangle-words against their true angle and
size.  CPU only."""
import importlib.util
import math
import os
import types

import numpy as np
import pytest

import detect_oriented_cases as oc
from dpmn_amd.utils import detect, quad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 180.0 / 64
_Q = {}


def quads_of(name):
    """(photo, quads) of a case of detect_oriented_cases, computed once."""
    if name not in _Q:
        make, kw = oc.CASES[name]
        photo = make()
        _Q[name] = (photo, detect.detect_oriented_np(photo, **kw))
    return _Q[name]


def passes_of(photo, gap=detect.GAP, vgap=detect.VGAP, floor=detect.FLOOR):
    """[(labels, what oriented_pass_np returns)] of the row pass and the column pass."""
    g, hist = detect.gradient(detect.luma_map(photo))
    b = g >= detect.threshold(hist, floor)
    out = []
    for column, (a, c) in enumerate(((gap, vgap), (vgap, gap))):
        lab = detect.label(detect.smooth(b, a, c))
        out.append((lab, detect.oriented_pass_np(lab, photo.shape[0], photo.shape[1], bool(column))))
    return out


def test_dirs_equal_their_formula():
    assert len(detect.DIRS) == 64
    for k, (c, s) in enumerate(detect.DIRS):
        t = math.radians((k - 32) * 180 / 64)
        assert (c, s) == (round(16384 * math.cos(t)), round(16384 * math.sin(t))), k
        assert c >= 0 and isinstance(c, int) and isinstance(s, int)
    assert detect.DIRS[32] == (16384, 0) and detect.DIRS[0] == (0, -16384)


@pytest.mark.parametrize("name", ["angle_20", "two_in_a_word", "bar"])
def test_moments_and_extents_agree_with_a_brute_force_loop(name):
    make, kw = oc.CASES[name]
    for lab, (m, ks, ext, _) in passes_of(make(), **kw):
        ids = sorted(set(lab[lab >= 0].tolist()))
        assert len(ids) == len(m) == len(ks) == len(ext) and len(ids) >= 1
        comps = detect.components(lab)
        for i, root in enumerate(ids):
            px = [(x, y) for y in range(lab.shape[0]) for x in range(lab.shape[1]) if lab[y, x] == root]
            want = [len(px), sum(x for x, y in px), sum(y for x, y in px), sum(x * x for x, y in px), sum(x * y for x, y in px),
                    sum(y * y for x, y in px)]
            assert m[i].tolist() == want, (name, i)
            if comps[i, 3] - comps[i, 1] < detect.MIN_H:
                assert ks[i] == -1 and ext[i].tolist() == [0, 0, 0, 0]
                continue
            A, sx, sy, sxx, sxy, syy = want
            mxx, mxy, myy = A * sxx - sx * sx, A * sxy - sx * sy, A * syy - sy * sy
            val = [c * c * mxx + 2 * c * s * mxy + s * s * myy for c, s in detect.DIRS]
            best = min((k for k in range(64) if val[k] == max(val)), key=lambda k: (abs(k - 32), k))
            assert ks[i] == best, (name, i)
            c, s = detect.DIRS[best]
            U = [c * (2 * x + 1) + s * (2 * y + 1) for x, y in px]
            V = [-s * (2 * x + 1) + c * (2 * y + 1) for x, y in px]
            assert ext[i].tolist() == [min(U), max(U), min(V), max(V)], (name, i)
            assert max(map(abs, U + V)) < 2 ** 31


def _brute_axis(row):
    A, sx, sy, sxx, sxy, syy = (int(v) for v in row)
    mxx, mxy, myy = A * sxx - sx * sx, A * sxy - sx * sy, A * syy - sy * sy
    val = [c * c * mxx + 2 * c * s * mxy + s * s * myy for c, s in detect.DIRS]
    return min((k for k in range(64) if val[k] == max(val)), key=lambda k: (abs(k - 32), k))


def test_axis_ties_go_to_the_direction_nearest_32_then_the_lower():
    m = np.array([[4, 2, 2, 2, 1, 2]])      # the 2 x 2 block at the origin: mxx = myy = 4, mxy = 0 -> the value is 4 (c^2 + s^2)
    n = [c * c + s * s for c, s in detect.DIRS]
    ties = [k for k in range(64) if n[k] == max(n)]
    assert len(ties) > 1 and 32 - ties[0] == ties[-1] - 32      # (the table is symmetric: a k below 32 and its mirror tie)
    assert detect.axis_index(m).tolist() == [min(ties, key=lambda k: (abs(k - 32), k))] == [_brute_axis(m[0])]
    assert detect.axis_index(m)[0] < 32      # of the two nearest, the lower
    bar = np.array([[3, 0, 3, 0, 0, 5]])      # the pixels (0, 0), (0, 1), (0, 2): myy = 6, mxx = mxy = 0 -> s^2 greatest: k = 0 only
    assert detect.axis_index(bar).tolist() == [0]
    assert detect.axis_index(np.zeros((0, 6), np.int64)).shape == (0,)


def test_terms_beyond_64_bits_are_compared_exactly():
    # a full 1024 x 1024 map as one component with one unit of x y more or less: the terms pass 2^64 and that unit still decides
    n = 1024
    A, sx, sxx = n * n, n * (n * (n - 1) // 2), n * ((n - 1) * n * (2 * n - 1) // 6)
    sxy = (n * (n - 1) // 2) ** 2
    m = np.array([[A, sx, sx, sxx, sxy + 1, sxx], [A, sx, sx, sxx, sxy - 1, sxx], [A, sx, sx, sxx, sxy, sxx]], np.int64)
    assert (A * sxx - sx * sx) * 16384 ** 2 > 2 ** 64
    got = detect.axis_index(m).tolist()
    assert got == [_brute_axis(r) for r in m]
    assert got[0] > 32 > got[1] and got[0] - 32 == 32 - got[1]


def test_an_upright_component_gives_the_unclamped_padded_upright_box():
    photo, quads = quads_of("angle_0")
    (lab, (m, ks, ext, rects)), _ = passes_of(photo)
    assert ks.tolist() == [32] and len(rects) == 1 and len(quads) == 1
    comps = detect.components(lab)
    x0, y0, x1, y1, _ = comps[0].tolist()
    assert rects[0, 5] == detect.S2 * (x1 - x0) and rects[0, 6] == detect.S2 * (y1 - y0)
    p = (y1 - y0 + 5) // 10
    assert quads[0].tolist() == [100 * v for v in (x0 - p, y0 - p, x1 + p, y0 - p, x1 + p, y1 + p, x0 - p, y1 + p)]
    big = 64      # boxes_from_components on a larger photo, where nothing is clamped, agrees
    shift = np.array([big, big, big, big, 0])
    box = detect.boxes_from_components(comps + shift, 1024, 1024)[0] - big
    assert quads[0].tolist() == [100 * int(v) for v in (box[0], box[1], box[2], box[1], box[2], box[3], box[0], box[3])]


def test_a_quad_may_leave_the_photo():
    photo = oc.rotated_word(0)[:, oc.MARGIN - 1:]      # the word's ring begins at the photo's left border: the padding leaves it
    q = detect.detect_oriented_np(photo)
    assert len(q) == 1 and q[0, 0] < 0 and q[0, 6] < 0
    assert detect.quad_lines(q).startswith("-")
    quad.check_quad(q[0] / 100.0)


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_every_quad_is_a_valid_quad(name, capsys):
    _, quads = quads_of(name)
    assert quads.dtype == np.int64 and quads.shape[1:] == (8,)
    for q in quads:
        quad.check_quad(q / 100.0)
    keys = [(q[1], q[0]) + tuple(q[2:]) for q in quads.tolist()]
    assert keys == sorted(keys) and len(quads) <= detect.MAX_BOXES


def _word(name):
    """(k, W2 H2, the rectangles that stay) of an angle case: the largest region that the cross-pass rule leaves."""
    photo, quads = quads_of(name)
    rows, cols = (p[1][3] for p in passes_of(photo))
    rects = detect.cross_pass(rows, cols)
    assert len(rects) == len(quads)
    i = int(np.argmax(rects[:, 5] * rects[:, 6]))
    return int(rects[i, 0]), int(rects[i, 5] * rects[i, 6]), rects


@pytest.mark.parametrize("angle", oc.ANGLES)
def test_the_axis_and_the_size_of_a_rotated_word(angle):
    k, area, _ = _word("angle_%d" % angle)
    found = (k - 32) * STEP
    err = abs((found - angle + 90) % 180 - 90)      # (directions are equal modulo 180 degrees)
    base = _word("angle_0")[1]
    print("angle %d: k %d = %.4f degrees, off by %.4f; area %.4f of the upright word's" % (angle, k, found, err, area / base))
    assert err <= STEP
    assert 100 * area <= 125 * base
    # the word is among the quads that are written, along +u: its top edge has the direction's angle
    _, quads = quads_of("angle_%d" % angle)
    w = max(quads.tolist(), key=lambda q: math.hypot(q[2] - q[0], q[3] - q[1]) * math.hypot(q[6] - q[0], q[7] - q[1]))
    assert abs(math.degrees(math.atan2(w[3] - w[1], w[2] - w[0])) - found) < 0.05


def test_the_row_pass_holds_up_to_45_degrees_and_the_column_pass_beyond():
    for angle in oc.ANGLES:
        k, _, rects = _word("angle_%d" % angle)
        assert (abs(k - 32) <= detect.AXIS_ROW) == (abs(angle) <= 45), angle
    assert _word("angle_90")[0] == 0      # exactly vertical: the tie rule reads it upward


def test_no_word_appears_twice_at_45_degrees():
    photo, quads = quads_of("angle_45")
    assert len(quads) == 1
    rows, cols = (p[1][3] for p in passes_of(photo))
    assert len(rows) == 1 and len(detect.cross_pass(rows, cols)) == 1      # (both passes find it; k = 48 is the row pass's)
    # the rule itself: of one rectangle found by both passes the row pass's stays; one that lies elsewhere stays
    r = rows[:1].copy()
    c = r.copy()
    c[0, 0] = 49
    assert detect.cross_pass(r, c).tolist() == r.tolist()
    small = c.copy()
    small[0, 5] -= 1
    assert detect.cross_pass(r, small).tolist() == r.tolist()
    # a smaller row-pass rectangle inside a column-pass one: it goes when squat (a turned letter), stays when long (a line)
    letter = r.copy()
    letter[0, 5], letter[0, 6] = (3 * r[0, 6] - 1) // 2, r[0, 6]      # 2 W2 < 3 H2
    assert detect.covered(letter, c, False).all() and detect.cross_pass(letter, c).tolist() == c.tolist()
    letter[0, 5] += 1
    assert detect.cross_pass(letter, c).tolist() == np.concatenate([letter, c]).tolist()
    far = c.copy()
    far[0, 1:3] += 400 * detect.S2
    assert len(detect.cross_pass(r, far)) == 2
    assert detect.covered(r, np.zeros((0, 8), np.int64), True).tolist() == [False]


def _sizes(quads):
    """(length of the top edge, length of the left edge, angle of the top edge in degrees) per quad, in photo pixels."""
    return [(math.hypot(q[2] - q[0], q[3] - q[1]) / 100, math.hypot(q[6] - q[0], q[7] - q[1]) / 100,
             math.degrees(math.atan2(q[3] - q[1], q[2] - q[0]))) for q in np.asarray(quads).tolist()]


@pytest.mark.parametrize("letter_w", [12, 20])
@pytest.mark.parametrize("letters", [5, 7, 8])
@pytest.mark.parametrize("angle", [60, 80, 90])
def test_a_steep_word_is_written_whatever_its_letters(letters, angle, letter_w):
    """The turned letters, 6 apart, pass the row pass on their own (30 wide, 12 or 20 high), and with an odd number of letters the
    word's centre lies on one of them.  The word is written in every case.  With letters 20 x 30 (a glyph's proportions) one quad is written.  The 12 x 30 letters are
    more than 1.5 times as long as high when turned, as a short line of a block of text would be: the shape cannot tell, and those that
    the rule covers and finds long are written beside the word."""
    photo = oc.rotated_word(angle, letters=letters, letter_w=letter_w)
    rows, cols = (p[1][3] for p in passes_of(photo))
    if angle >= 80:
        assert len(cols) == 1
        if letter_w == 12:
            assert len(rows) == letters      # (what the rule has to sort out; the hollow 20-wide rings fail the fill filter)
    sizes = _sizes(detect.detect_oriented_np(photo))
    want = letters * letter_w + (letters - 1) * oc.LETTER_GAP
    words = [(w, h, a) for w, h, a in sizes if w >= want]
    assert len(words) == 1
    w, h, got = words[0]
    assert w <= want + 16 and oc.LETTER_H <= h <= oc.LETTER_H + 16      # the whole word: ring, padding and the slack of the axis
    assert abs((got - angle + 90) % 180 - 90) <= STEP + 0.05
    if letter_w == 20 or angle == 60:
        assert len(sizes) == 1
    else:
        assert all(w <= oc.LETTER_H + 10 for w, h, _ in sizes if w < want)      # what stays beside it are letters


@pytest.mark.parametrize("lines", [6, 8])
def test_the_lines_of_a_narrow_block_of_horizontal_text_all_stay(lines):
    """Lines of 5 upright letters, 3 apart, the lines 8 apart: the column pass joins them into one tall blob that is larger than any
    line and holds every line's centre.  Every line is written, as the upright detector finds it; the blob comes with them."""
    photo = oc.block(lines)
    rows, cols = (p[1][3] for p in passes_of(photo))
    assert len(rows) == lines and len(cols) == 1 and (cols[0, 5] * cols[0, 6] > rows[:, 5] * rows[:, 6]).all()
    assert detect.covered(rows, cols, False).all()
    sizes = _sizes(detect.detect_oriented_np(photo))
    flat = [(w, h) for w, h, a in sizes if abs(a) < 0.01]
    assert len(flat) == lines == len(detect.detect_text_np(photo))
    assert all(72 <= w <= 72 + 10 and 30 <= h <= 30 + 10 for w, h in flat)
    assert len(sizes) == lines + 1      # the blob: steep, for the user to delete


def test_the_lines_of_a_rendered_paragraph_all_stay():
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default(size=24)
    im = Image.new("RGB", (300, 320), (oc.PAPER,) * 3)
    draw, y = ImageDraw.Draw(im), 40
    for text in "fresh bread baked daily since 1952".split():
        draw.text((40, y), text, fill=(oc.INK,) * 3, font=font)
        y = draw.textbbox((40, y), text, font=font)[3] + 5
    photo = np.asarray(im)
    sizes = _sizes(detect.detect_oriented_np(photo))
    assert len(detect.detect_text_np(photo)) == 6
    assert len([1 for w, h, a in sizes if abs(a) <= STEP + 0.05 and 40 < w < 90 and h < 40]) == 6      # (the least is 'daily', 56 x 28)


def test_more_than_max_boxes_keeps_the_largest(capsys):
    make, kw = oc.CASES["many"]
    _Q.pop("many", None)
    photo, quads = quads_of("many")
    out = capsys.readouterr().out
    assert len(quads) == detect.MAX_BOXES and "regions found, the 256 of largest area kept" in out
    assert all(len(detect.components(lab)) > 4096 for lab, _ in passes_of(photo, **kw))


def test_write_quads_round_trips_through_numbered_boxes(tmp_path):
    quads = np.array([[-5, -150, 12345, 7, 12399, 20001, 100, 19950], [0, 99, 100, 101, -100, -99, 5, 50]], np.int64)
    assert detect.quad_lines(quads[:1]) == "-0.05,-1.50,123.45,0.07,123.99,200.01,1.00,199.50\n"
    path = str(tmp_path / "q.txt")
    detect.write_quads(path, quads)
    back = quad.numbered_boxes(path)
    assert [k for k, _, _, _ in back] == [0, 1]
    got = np.array([q.reshape(-1) for _, _, q, _ in back])
    assert np.array_equal(np.round(got * 100).astype(np.int64), quads) and np.abs(got * 100 - quads).max() < 1e-9
    detect.write_quads(path, np.zeros((0, 8), np.int64))
    assert quad.numbered_boxes(path) == []
    for name in ("angle_20", "angle_60"):
        _, q = quads_of(name)
        detect.write_quads(path, q)
        assert np.array_equal(np.round(np.array([b[2].reshape(-1) for b in quad.numbered_boxes(path)]) * 100).astype(np.int64), q)


def _main():
    spec = importlib.util.spec_from_file_location("dpmn_main_detect_oriented", os.path.join(ROOT, "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_flag_needs_demo_detect():
    m = _main()
    for flags in (dict(demo_detect_oriented=True), dict(demo_detect_oriented=True, demo_dir="d"),
                  dict(demo_detect_oriented=True, demo_dir="d", demo_boxes="b")):
        args = types.SimpleNamespace(**flags)
        with pytest.raises(ValueError) as e:
            m.demo_detect_setting(args)
        assert "main.py: " + str(e.value) == m.DEMO_DETECT_ORIENTED_NEEDS
        with pytest.raises(SystemExit) as e:
            m.main(types.SimpleNamespace(), args)
        assert str(e.value) == m.DEMO_DETECT_ORIENTED_NEEDS and "\n" not in str(e.value)


def test_the_command_line_knows_the_flag_and_it_combines_with_its_neighbours():
    import subprocess
    import sys
    m = _main()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--demo_dir", "d", "--demo_detect_oriented"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and m_text(r.stderr).endswith(m.DEMO_DETECT_ORIENTED_NEEDS[len("main.py: "):])
    ok = types.SimpleNamespace(demo_detect=True, demo_detect_oriented=True, demo_dir="d", demo_tile=True, demo_paste=True, rec="crnn",
                               rec_lexicon="words.txt", demo_detect_gap=20)
    assert m.demo_detect_setting(ok) == (20, 24)
    with pytest.raises(ValueError) as e:      # the rules of --demo_detect still hold with it
        m.demo_detect_setting(types.SimpleNamespace(demo_detect=True, demo_detect_oriented=True, demo_dir="d", demo_boxes="b"))
    assert "main.py: " + str(e.value) == m.DEMO_DETECT_OR_BOXES


def m_text(stderr):
    return " ".join(stderr.split())


def test_detect_box_files_writes_oriented_quads(tmp_path, monkeypatch):
    """dataset.folder.detect_box_files(oriented=True) asks ops.detect_oriented_u8 (here: the restatement in its place, no GPU) and
    writes its quads in decimals; without the flag it asks detect_text_u8 as before."""
    from PIL import Image
    from dpmn_amd import ops
    from dpmn_amd.dataset import folder
    from dpmn_amd.utils import resize
    photo, quads = quads_of("angle_30")
    src = tmp_path / "photos"
    src.mkdir()
    Image.fromarray(photo).save(str(src / "a.png"))
    calls = []

    def fake(which, one):
        def run(packed, offsets, sizes, gap=12, vgap=2, floor=24, names=None):
            calls.append(which)
            (off, h, w), = [(int(o), int(a), int(b)) for o, (a, b) in zip(offsets, sizes)]
            return [one(packed.numpy()[off:off + h * w * 3].reshape(h, w, 3), gap, vgap, floor)]
        return run

    monkeypatch.setattr(ops, "detect_oriented_u8", fake("oriented", detect.detect_oriented_np))
    monkeypatch.setattr(ops, "detect_text_u8", fake("upright", detect.detect_text_np))
    assert folder.detect_box_files(str(src), str(tmp_path / "o"), 2, "cpu", oriented=True) == 1 and calls == ["oriented"]
    with open(str(tmp_path / "o" / "a.txt")) as f:
        assert f.read() == detect.quad_lines(quads) and "." in detect.quad_lines(quads)
    assert [q.reshape(-1).tolist() for _, _, q, _ in quad.numbered_boxes(str(tmp_path / "o" / "a.txt"))] == (quads / 100.0).tolist()
    folder.detect_box_files(str(src), str(tmp_path / "u"), 2, "cpu")
    assert calls == ["oriented", "upright"]
