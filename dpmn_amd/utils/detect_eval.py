"""Detected regions and their reads scored against ground truth (main.py --demo_eval): the ICDAR 2015 detection protocol -- precision,
recall and h-mean at IoU > 0.5 with don't-care regions -- and the end-to-end score, where a match counts only when the SR read equals
the transcription.  This module is the definition: the overlap of two regions in integers, the protocol, the reader of the ground-truth
files and the CSV.  NumPy and Python integers only, importable without a GPU; ops.region_overlap_counts (csrc/detect_eval.hip)
reproduces region_counts_np with ==.

Regions and units.  A region is a closed polygon of n points (x, y) in photo pixels, MIN_POINTS <= n <= MAX_POINTS: a detected quad, a
ground-truth quad or a ground-truth polygon of 2k points, taken AS WRITTEN (no check_quad, no check_polygon: real ground truth holds
anticlockwise and self-crossing quads).  Every coordinate is rounded to hundredths of a pixel and multiplied by 8, so one pixel is
UNIT = 800 units and every vertex coordinate is a multiple of 8.  utils.detect._hundredths formats integers and does not fit floats:
the rounding here is HALF AWAY FROM ZERO of 100 * v in float64 (floor(|100 v| + 0.5) with the sign put back).  A coordinate beyond
+-MAX_PX pixels is a ValueError.

Samples.  4 x 4 per pixel: pixel (i, j) has its samples at x = 800 j + 100 (2a + 1), y = 800 i + 100 (2b + 1), a, b in 0 .. 3 -- with
the sample column c = 4 j + a and the sample row m = 4 i + b, x = 200 c + 100 and y = 200 m + 100.  A sample coordinate is an odd
multiple of 100 = 4 * 25, so it is 4 mod 8 and never a multiple of 8: no sample shares an x or a y with a vertex and the crossing
test has no vertex case.  Samples are not clipped to the photo.

Inside test.  Even-odd: an edge (x0, y0) -> (x1, y1) counts for the sample (px, py) when (y0 > py) != (y1 > py) and its crossing with
the line y = py lies strictly to the right of px; the sample is inside when an odd number of edges count.  The crossing is at
x0 + (py - y0) (x1 - x0) / (y1 - y0); it is right of px exactly when cross = (x1 - x0) (py - y0) - (px - x0) (y1 - y0) is non-zero and has
the sign of y1 - y0 (cross == 0, the sample on the edge, does not count).  No division and no floating point.  Magnitudes: |coordinate| <=
16384 * 800 < 2^24 for vertices and (the samples of a box of vertices) for samples, so every difference is below 2^25, every product
below 2^50 and cross below 2^51 < 2^53.

Counts.  The integer pixel box of a region is [floor(min / 800), ceil(max / 800)) on both axes (empty for a region without extent on
an axis).  area(R) = the samples inside R over R's box; inter(A, B) = the samples inside both over the intersection of the two boxes, 0
with no work when the boxes do not meet.  IoU > 0.5 is 2 * inter > area_A + area_B - inter in integers; a region of area 0 matches
nothing (its inter is 0).

The row form (what the kernel computes; rows_count_np here, asserted equal to the sample form by the tests): on the sample row m an
edge that crosses y = py has the edge to the right of exactly the sample columns c < t, t = ceil((xc - 100) / 200) with xc its crossing:
with dy = y1 - y0 > 0 (both signs flipped otherwise), t = ceil(((x0 - 100) dy + (py - y0) (x1 - x0)) / (200 dy)), one exact integer
division (numerator below 2^51).  A row has an even number of crossings; sorted, t_0 <= t_1 <= ..., the inside columns are
[t_0, t_1), [t_2, t_3), ..., clamped to the box: counting is a sum of differences, not a walk over samples.

Limits, stated plainly: IoU is sampled at 16 samples per pixel, not the exact polygon area, so a pair within the sampling error of
0.5 can fall either way; the even-odd rule gives a self-crossing quad its bow-tie area; matching is the ICDAR script's greedy order,
not an optimal assignment; the numbers say nothing about the quality of the SR images.
"""
import csv
import math
import os

import numpy as np

from .poly import CTW_MARK, _leading_floats
from .quad import DONT_CARE

UNIT = 800              # units per pixel: hundredths times 8
SUB = 4                 # samples per pixel and axis
STEP = UNIT // SUB      # 200 units between samples, the first at STEP // 2
MAX_PX = 16384          # a coordinate beyond +-MAX_PX pixels is refused
MIN_POINTS, MAX_POINTS = 4, 64
_CHUNK = 1 << 21        # samples per slab of the sample form

CSV_HEAD = ["file", "gt", "gt_care", "det", "det_care", "matched", "precision", "recall", "hmean", "e2e_labelled", "e2e_correct",
            "e2e_precision", "e2e_recall", "e2e_hmean"]
CSV_LEXICON = ["e2e_lexicon_precision", "e2e_lexicon_recall", "e2e_lexicon_hmean"]
CSV_LM = ["e2e_lm_precision", "e2e_lm_recall", "e2e_lm_hmean"]      # (the reads of the CTC beam search: main.py --rec_beam / --rec_lm)


def region_units(points):
    """(n, 2) points in pixels -> int64 (n, 2) in units: hundredths rounded half away from zero, times 8.  ValueError for a shape that
    is not MIN_POINTS .. MAX_POINTS points, a coordinate that is not finite or one beyond +-MAX_PX pixels."""
    p = np.asarray(points, np.float64)
    if p.ndim != 2 or p.shape[1] != 2 or not MIN_POINTS <= p.shape[0] <= MAX_POINTS:
        raise ValueError("detect_eval: a region is %d .. %d points (x, y), got shape %s" % (MIN_POINTS, MAX_POINTS, p.shape))
    if not np.isfinite(p).all():
        raise ValueError("detect_eval: a coordinate is not finite")
    if (np.abs(p) > MAX_PX).any():
        raise ValueError("detect_eval: a coordinate lies beyond +-%d pixels" % MAX_PX)
    h = np.floor(np.abs(p * 100.0) + 0.5) * np.sign(p)
    return h.astype(np.int64) * 8


def regions_flat(regions):
    """region_units and region_box of a whole list of regions at once (the host plan of ops.region_overlap_counts) -> (units int64
    (sum n, 2) of all regions back to back, n int64 per region, boxes int64 (len, 4)), the same numbers and the same refusals."""
    pts = [np.asarray(r, np.float64) for r in regions]
    for p in pts:
        if p.ndim != 2 or p.shape[1] != 2 or not MIN_POINTS <= p.shape[0] <= MAX_POINTS:
            raise ValueError("detect_eval: a region is %d .. %d points (x, y), got shape %s" % (MIN_POINTS, MAX_POINTS, p.shape))
    n = np.array([len(p) for p in pts], np.int64)
    if not len(pts):
        return np.zeros((0, 2), np.int64), n, np.zeros((0, 4), np.int64)
    cat = np.concatenate(pts)
    if not np.isfinite(cat).all():
        raise ValueError("detect_eval: a coordinate is not finite")
    if (np.abs(cat) > MAX_PX).any():
        raise ValueError("detect_eval: a coordinate lies beyond +-%d pixels" % MAX_PX)
    units = (np.floor(np.abs(cat * 100.0) + 0.5) * np.sign(cat)).astype(np.int64) * 8
    starts = np.cumsum(n) - n
    lo, hi = np.minimum.reduceat(units, starts, axis=0), np.maximum.reduceat(units, starts, axis=0)
    return units, n, np.concatenate([lo // UNIT, -(-hi // UNIT)], axis=1)


def region_box(units):
    """int64 (n, 2) units -> the integer pixel box (x0, y0, x1, y1), ends exclusive: floor of the least, ceil of the greatest."""
    u = np.asarray(units, np.int64)
    lo, hi = u.min(axis=0), u.max(axis=0)
    return int(lo[0] // UNIT), int(lo[1] // UNIT), int(-(-hi[0] // UNIT)), int(-(-hi[1] // UNIT))


def boxes_of(units_list):
    """A list of unit arrays -> int64 (n, 4) boxes."""
    return np.array([region_box(u) for u in units_list], np.int64).reshape(-1, 4)


def meeting_pairs(boxes_a, boxes_b):
    """int64 (na, 4) and (nb, 4) boxes -> int64 (p, 2): the (a, b) whose boxes share a pixel, in row-major order."""
    a, b = np.asarray(boxes_a, np.int64).reshape(-1, 4), np.asarray(boxes_b, np.int64).reshape(-1, 4)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((0, 2), np.int64)
    meet = ((np.maximum(a[:, None, 0], b[None, :, 0]) < np.minimum(a[:, None, 2], b[None, :, 2]))
            & (np.maximum(a[:, None, 1], b[None, :, 1]) < np.minimum(a[:, None, 3], b[None, :, 3])))
    return np.stack(np.nonzero(meet), axis=1).astype(np.int64)


def inside_np(units, box):
    """The sample form of the inside test: int64 (n, 2) units and a pixel box -> bool (4 h, 4 w), the samples of the box inside the
    region under the even-odd rule, decided by the sign of one int64 cross product per sample and edge."""
    x0b, y0b, x1b, y1b = (int(v) for v in box)
    h, w = max(SUB * (y1b - y0b), 0), max(SUB * (x1b - x0b), 0)
    out = np.zeros((h, w), bool)
    if h == 0 or w == 0:
        return out
    u = np.asarray(units, np.int64)
    nxt = np.roll(u, -1, axis=0)
    ys = STEP * (SUB * y0b + np.arange(h, dtype=np.int64)) + STEP // 2
    xs = STEP * (SUB * x0b + np.arange(w, dtype=np.int64)) + STEP // 2
    for (ex0, ey0), (ex1, ey1) in zip(u.tolist(), nxt.tolist()):
        rows = np.nonzero((ey0 > ys) != (ey1 > ys))[0]
        dy = ey1 - ey0
        for s in range(0, len(rows), max(_CHUNK // w, 1)):
            r = rows[s:s + max(_CHUNK // w, 1)]
            cross = ((ex1 - ex0) * (ys[r] - ey0))[:, None] - (xs - ex0)[None, :] * dy
            out[r] ^= (cross > 0) if dy > 0 else (cross < 0)
    return out


def _meet(box_a, box_b):
    return max(box_a[0], box_b[0]), max(box_a[1], box_b[1]), min(box_a[2], box_b[2]), min(box_a[3], box_b[3])


def area_np(units):
    return int(inside_np(units, region_box(units)).sum())


def inter_np(units_a, units_b):
    box = _meet(region_box(units_a), region_box(units_b))
    if box[0] >= box[2] or box[1] >= box[3]:
        return 0
    return int((inside_np(units_a, box) & inside_np(units_b, box)).sum())


def row_breaks(units, m, c0, c1):
    """The row form of one sample row m: the sorted t of the edges that cross it, clamped to the sample columns c0 .. c1 (Python ints)."""
    py = STEP * m + STEP // 2
    u = np.asarray(units, np.int64).tolist()
    ts = []
    for (x0, y0), (x1, y1) in zip(u, u[1:] + u[:1]):
        if (y0 > py) == (y1 > py):
            continue
        dy, num = y1 - y0, (x0 - STEP // 2) * (y1 - y0) + (py - y0) * (x1 - x0)
        if dy < 0:
            dy, num = -dy, -num
        ts.append(min(max(-((-num) // (STEP * dy)), c0), c1))
    return sorted(ts)


def rows_count_np(units_a, units_b=None):
    """The row form: area(A) for one region, inter(A, B) for two -- sums of differences of the rows' sorted breaks.  Equal to
    area_np / inter_np (the tests assert it); what csrc/detect_eval.hip computes."""
    box = region_box(units_a) if units_b is None else _meet(region_box(units_a), region_box(units_b))
    if box[0] >= box[2] or box[1] >= box[3]:
        return 0
    c0, c1, total = SUB * box[0], SUB * box[2], 0
    for m in range(SUB * box[1], SUB * box[3]):
        a = row_breaks(units_a, m, c0, c1)
        if units_b is None:
            total += sum(a[1::2]) - sum(a[0::2])
            continue
        b = row_breaks(units_b, m, c0, c1)
        i = j = 0
        while i < len(a) and j < len(b):
            total += max(min(a[i + 1], b[j + 1]) - max(a[i], b[j]), 0)
            if a[i + 1] < b[j + 1]:
                i += 2
            else:
                j += 2
    return total


def region_counts_np(regions_a, regions_b):
    """Two lists of (n, 2) point arrays in pixels (one photo's detections and its ground truth) -> (area_a uint64 (na), area_b uint64
    (nb), pairs int64 (p, 2), inter uint64 (p)): pairs are the (a, b) whose boxes meet, in row-major order, inter their common
    samples.  The restatement that ops.region_overlap_counts reproduces with ==."""
    ua, ub = [region_units(r) for r in regions_a], [region_units(r) for r in regions_b]
    pairs = meeting_pairs(boxes_of(ua), boxes_of(ub))
    return (np.array([area_np(u) for u in ua], np.uint64), np.array([area_np(u) for u in ub], np.uint64), pairs,
            np.array([inter_np(ua[a], ub[b]) for a, b in pairs.tolist()], np.uint64))


def region_counts_batch_np(photos_a, photos_b):
    """region_counts_np per photo: two lists (one entry per photo) of region lists -> a list of its four arrays per photo."""
    if len(photos_a) != len(photos_b):
        raise ValueError("detect_eval: %d and %d photos" % (len(photos_a), len(photos_b)))
    return [region_counts_np(a, b) for a, b in zip(photos_a, photos_b)]


# ---- the protocol ----

def prf(matched, n_gt, n_det, total=False):
    """(precision, recall, hmean) of the ICDAR script.  Per photo: without a care ground truth recall is 1 and precision is 1 when
    there is no care detection either, else 0; without a care detection otherwise precision is 0.  total=True (the script's dataset
    line): a ratio without a denominator is 0."""
    matched, n_gt, n_det = int(matched), int(n_gt), int(n_det)
    if total:
        r = matched / n_gt if n_gt else 0.0
        p = matched / n_det if n_det else 0.0
    elif n_gt == 0:
        r, p = 1.0, (0.0 if n_det else 1.0)
    else:
        r, p = matched / n_gt, (matched / n_det if n_det else 0.0)
    return p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)


def match(area_det, area_gt, pairs, inter, gt_dont_care, det_absent=()):
    """One photo's record from the counts of region_counts_np(detections, ground truth).  gt_dont_care: one flag per ground-truth
    region.  A detection is don't-care when 2 * inter > area_det with some don't-care ground truth.  Greedy as the script: the ground
    truth in file order, per region the detections in file order; a pair matches when both are unmatched, neither is don't-care and
    2 * inter > area_det + area_gt - inter.  det_absent: indices of detections that do not take part at all (not counted).
    -> {matches [(gt, det)], det_dont_care [det], gt, gt_care, det, det_care, matched, precision, recall, hmean}."""
    ad, ag = [int(v) for v in np.asarray(area_det).reshape(-1)], [int(v) for v in np.asarray(area_gt).reshape(-1)]
    dc_gt = [bool(v) for v in gt_dont_care]
    if len(dc_gt) != len(ag):
        raise ValueError("detect_eval: %d don't-care flags for %d ground-truth regions" % (len(dc_gt), len(ag)))
    absent = set(int(d) for d in det_absent)
    table = {(int(d), int(g)): int(v) for (d, g), v in zip(np.asarray(pairs, np.int64).reshape(-1, 2).tolist(), np.asarray(inter).reshape(-1).tolist())}
    dc_det = sorted({d for (d, g), v in table.items() if dc_gt[g] and d not in absent and 2 * v > ad[d]})
    matches, taken = [], set(dc_det) | absent
    for g in range(len(ag)):
        if dc_gt[g]:
            continue
        for d in range(len(ad)):
            v = table.get((d, g), 0)
            if d not in taken and 2 * v > ad[d] + ag[g] - v:
                matches.append((g, d))
                taken.add(d)
                break
    n_det = len(ad) - len(absent)
    rec = {"matches": matches, "det_dont_care": dc_det, "gt": len(ag), "gt_care": len(ag) - sum(dc_gt), "det": n_det,
           "det_care": n_det - len(dc_det), "matched": len(matches)}
    rec["precision"], rec["recall"], rec["hmean"] = prf(rec["matched"], rec["gt_care"], rec["det_care"])
    return rec


def e2e(record, gt_labels, gt_dont_care, det_reads, spaces=True):
    """The end-to-end counts of one photo: a matched pair is read correctly when str_filt(label, "lower") equals the detection's read
    (spaces=False, the rows of --demo_line_read: both sides without their spaces).  A care ground truth whose filtered label is empty
    is out of the count, and so is a detection matched to it.  -> {e2e_labelled, e2e_correct, e2e_det, e2e_precision, e2e_recall,
    e2e_hmean}: recall over the labelled care ground truth, precision over the care detections less those matched to a label-less
    ground truth (prf's per-photo conventions for empty sets)."""
    from .util import str_filt
    keep = (lambda s: s) if spaces else (lambda s: s.replace(" ", ""))
    labels = [keep(str_filt(t, "lower")) for t in gt_labels]
    labelled = sum(1 for t, dc in zip(labels, gt_dont_care) if t and not dc)
    correct = sum(1 for g, d in record["matches"] if labels[g] and labels[g] == keep(det_reads[d]))
    n_det = record["det_care"] - sum(1 for g, d in record["matches"] if not labels[g])
    p, r, h = prf(correct, labelled, n_det)
    return {"e2e_labelled": labelled, "e2e_correct": correct, "e2e_det": n_det, "e2e_precision": p, "e2e_recall": r, "e2e_hmean": h}


def score(records):
    """The dataset line: matched, care ground truth and care detections summed over the photos' records (micro average; prf with
    total=True) -> {gt, gt_care, det, det_care, matched, precision, recall, hmean}, and the same sums of the e2e keys where the
    records hold them (e2e_*, and e2e_lexicon_* / e2e_lm_* when present)."""
    records = list(records)
    tot = {k: sum(r[k] for r in records) for k in ("gt", "gt_care", "det", "det_care", "matched")}
    tot["precision"], tot["recall"], tot["hmean"] = prf(tot["matched"], tot["gt_care"], tot["det_care"], total=True)
    for pre in ("e2e_", "e2e_lexicon_", "e2e_lm_"):
        if records and all(pre + "correct" in r for r in records):
            for k in ("labelled", "correct", "det"):
                tot[pre + k] = sum(r[pre + k] for r in records)
            tot[pre + "precision"], tot[pre + "recall"], tot[pre + "hmean"] = prf(tot[pre + "correct"], tot[pre + "labelled"],
                                                                                 tot[pre + "det"], total=True)
    return tot


# ---- files ----

def numbered_regions(path):
    """The lines of a ground-truth or box file -> [(k, line number, points, label, dont_care)].  The conventions of
    utils.poly.numbered_polygons -- UTF-8 with a BOM dropped, empty lines ignored, k counting the non-empty lines from 0, a line split at
    EVERY comma, the first 4 * (n // 4) leading numbers the coordinates and the rest the transcription, a leading #### stripped, a line
    of fewer than 8 leading numbers or more than MAX_POINTS points skipped with one printed line -- except that a line whose
    transcription is ### (also after the #### was stripped) is KEPT, with dont_care True."""
    out, k = [], -1
    with open(path, encoding="utf-8-sig") as fh:
        for lineno, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            k += 1
            parts = line.split(",")
            nums = _leading_floats(parts)
            n = 4 * (len(nums) // 4)
            if n < 8 or n > 2 * MAX_POINTS:
                why = "%d leading numbers" % len(nums) if n < 8 else "%d points, more than %d" % (n // 2, MAX_POINTS)
                print("detect_eval: %s line %d does not parse (%s), skipped" % (path, lineno, why))
                continue
            label = ",".join(parts[n:])
            if label.startswith(CTW_MARK) and label.strip() != DONT_CARE:
                label = label[len(CTW_MARK):]
            out.append((k, lineno, np.array(nums[:n], np.float64).reshape(-1, 2), label if label != "" else " ", label.strip() == DONT_CARE))
    return out


def find_file(dir_, stem):
    """dir_/<stem>.txt, or else dir_/gt_<stem>.txt, or None."""
    return next((p for p in (os.path.join(dir_, stem + ".txt"), os.path.join(dir_, "gt_" + stem + ".txt")) if os.path.isfile(p)), None)


def _usable(regions, what, path):
    """numbered_regions' items -> [(item, refused)]: a region whose coordinates region_units refuses gets one printed line."""
    out = []
    for item in regions:
        try:
            region_units(item[2])
            out.append((item, False))
        except ValueError as e:
            print("detect_eval: %s region refused (%s line %d: %s)" % (what, path, item[1], e))
            out.append((item, True))
    return out


_PLACEHOLDER = np.zeros((MIN_POINTS, 2), np.float64)      # stands in for a refused region: area 0, box empty, meets nothing


def load_photo(stem, box_dir, gt_dir, reads):
    """One photo's two region lists, or None (one printed line) when it has no ground-truth file.  reads: {k: (sr_string, sr_lexicon or
    None)} for the lines of the box file that the run read and kept; the other lines are left out.  A ground-truth region refused for
    its coordinates counts as don't-care, a refused detection as absent (one printed line each).
    -> {stem, det [points], det_reads [(sr, lex)], det_absent [index], gt [points], gt_labels, gt_dont_care}."""
    gt_file = find_file(gt_dir, stem)
    if gt_file is None:
        print("detect_eval: %s has no ground truth (%s.txt or gt_%s.txt in %s), left out" % (stem, stem, stem, gt_dir))
        return None
    box_file = find_file(box_dir, stem)
    dets = [it for it in (numbered_regions(box_file) if box_file else []) if it[0] in reads]
    photo = {"stem": stem, "det": [], "det_reads": [], "det_absent": [], "gt": [], "gt_labels": [], "gt_dont_care": []}
    for (k, _, pts, _, _), refused in _usable(dets, "detected", box_file):
        if refused:
            photo["det_absent"].append(len(photo["det"]))
        photo["det"].append(_PLACEHOLDER if refused else pts)
        photo["det_reads"].append(reads[k])
    for (_, _, pts, label, dc), refused in _usable(numbered_regions(gt_file), "ground-truth", gt_file):
        photo["gt"].append(_PLACEHOLDER if refused else pts)
        photo["gt_labels"].append(label)
        photo["gt_dont_care"].append(bool(dc or refused))
    return photo


def _fmt(v):
    return "%.4f" % v


def evaluate(photos, counts, recogniser=True, lexicon=False, spaces=True, lm=False):
    """The records of a list of load_photo's photos: counts is region_counts_batch_np or a callable with its contract
    (ops.region_overlap_counts on a device).  recogniser=False: no e2e keys.  lm: the reads hold a third item, the beam search's
    string, scored under e2e_lm_* as the lexicon's word is under e2e_lexicon_*.  -> (records, totals)."""
    records = []
    for photo, (ad, ag, pairs, inter) in zip(photos, counts([p["det"] for p in photos], [p["gt"] for p in photos]) if photos else ()):
        rec = match(ad, ag, pairs, inter, photo["gt_dont_care"], photo["det_absent"])
        rec["file"] = photo["stem"]
        if recogniser:
            rec.update(e2e(rec, photo["gt_labels"], photo["gt_dont_care"], [r[0] for r in photo["det_reads"]], spaces))
            if lexicon:
                lex = e2e(rec, photo["gt_labels"], photo["gt_dont_care"], [r[1] or "" for r in photo["det_reads"]], spaces)
                rec.update({"e2e_lexicon_" + k[4:]: v for k, v in lex.items()})
            if lm:
                got = e2e(rec, photo["gt_labels"], photo["gt_dont_care"], [r[2] or "" for r in photo["det_reads"]], spaces)
                rec.update({"e2e_lm_" + k[4:]: v for k, v in got.items()})
        records.append(rec)
    return records, score(records)


def csv_rows(records, totals, recogniser=True, lexicon=False, lm=False):
    """The rows of detect_eval.csv, header first and TOTAL last; ratios with four decimals, the e2e columns empty without a recogniser."""
    head = CSV_HEAD + (CSV_LEXICON if lexicon else []) + (CSV_LM if lm else [])
    rows = [head]
    for rec in list(records) + [dict(totals, file="TOTAL")]:
        row = [rec["file"]] + [str(rec[k]) for k in ("gt", "gt_care", "det", "det_care", "matched")] + [_fmt(rec[k]) for k in ("precision", "recall", "hmean")]
        if recogniser and "e2e_correct" in rec:
            row += [str(rec["e2e_labelled"]), str(rec["e2e_correct"])] + [_fmt(rec["e2e_" + k]) for k in ("precision", "recall", "hmean")]
        else:
            row += [""] * 5
        if lexicon:
            row += [_fmt(rec["e2e_lexicon_" + k]) for k in ("precision", "recall", "hmean")] if "e2e_lexicon_correct" in rec else [""] * 3
        if lm:
            row += [_fmt(rec["e2e_lm_" + k]) for k in ("precision", "recall", "hmean")] if "e2e_lm_correct" in rec else [""] * 3
        rows.append(row)
    return rows


def write_csv(path, records, totals, recogniser=True, lexicon=False, lm=False):
    with open(path, "w", newline="") as out:
        csv.writer(out).writerows(csv_rows(records, totals, recogniser, lexicon, lm))


def totals_line(totals, n_photos):
    """The one printed line of a run."""
    line = ("detect_eval: %d photos, %d of %d care ground-truth regions matched by %d care detections: precision %.4f recall %.4f hmean %.4f"
            % (n_photos, totals["matched"], totals["gt_care"], totals["det_care"], totals["precision"], totals["recall"], totals["hmean"]))
    for pre, name in (("e2e_", "end to end"), ("e2e_lexicon_", "end to end under the lexicon"),
                      ("e2e_lm_", "end to end under the beam search")):
        if pre + "correct" in totals:
            line += "; %s %d of %d read correctly: precision %.4f recall %.4f hmean %.4f" % (
                name, totals[pre + "correct"], totals[pre + "labelled"], totals[pre + "precision"], totals[pre + "recall"], totals[pre + "hmean"])
    return line


def evaluate_dir(stems, reads_by_stem, box_dir, gt_dir, out_path, counts, recogniser=True, lexicon=False, spaces=True, batch=64, lm=False):
    """main.py --demo_eval: the photos `stems` of a run, scored in batches of `batch` photos (one counts call each), written to
    out_path as detect_eval.csv -> (records, totals); one line with the totals is printed.  reads_by_stem: {stem: {k: (sr_string,
    sr_lexicon or None)}} of the regions the run read and kept; lm: the reads are (sr_string, sr_lexicon or None, sr_lm)."""
    photos = [p for p in (load_photo(s, box_dir, gt_dir, reads_by_stem.get(s, {})) for s in stems) if p is not None]
    records = []
    for i in range(0, len(photos), int(batch)):
        records += evaluate(photos[i:i + int(batch)], counts, recogniser, lexicon, spaces, lm)[0]
    totals = score(records)
    if not recogniser:
        totals = {k: v for k, v in totals.items() if not k.startswith("e2e_")}
    write_csv(out_path, records, totals, recogniser, lexicon, lm)
    print(totals_line(totals, len(records)))
    return records, totals


def row_reads(rows, conf=False, upright=False, lexicon=False, min_conf=False, lm=False):
    """The rows TextSR.demo returns with boxes=True (file, box, label, lr_string, [lr_conf,] sr_string, [sr_conf, [turned,]]
    [sr_lexicon, sr_lexicon_score,] [kept]) -> {stem: {k: (sr_string, sr_lexicon or None)}} of the regions that were kept.
    lm: the rows also hold sr_lm, sr_lm_score -- behind the lexicon's columns, or without a lexicon behind sr_string / sr_conf and
    before turned -- and the values are (sr_string, sr_lexicon or None, sr_lm)."""
    out = {}
    i_sr = 5 if conf else 4
    i_lex = i_sr + 1 + (1 + bool(upright) if conf else 0)
    i_lm = i_lex + 2 if lexicon else i_sr + 1 + bool(conf)
    for r in rows:
        if min_conf and str(r[-1]) == "0":
            continue
        out.setdefault(r[0], {})[int(r[1])] = (r[i_sr], r[i_lex] if lexicon else None) + ((r[i_lm],) if lm else ())
    return out
