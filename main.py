#!/usr/bin/env python3
"""Command-line entry with the reference's flags (main.py:37-67) and config file (config/super_resolution.yaml, main.py:69).

`python main.py --arch tatt --mask --gradient --stu_iter_b1 3 --stu_iter_b2 3 ...` builds the same TextSR mission on the
HIP-backed modules.  `--rec crnn` loads the native CRNN recogniser (config TRAIN.VAL.crnn_pretrained) for the word accuracy,
`--rec aster` the native ASTER recogniser (config TRAIN.VAL.rec_pretrained, when set), `--rec moran` the native MORAN recogniser
(config TRAIN.VAL.moran_pretrained, when set).  Without a TextZoom LMDB directory the loop is fed synthetic (images_hr, images_lr, label_vecs)
batches of the real shapes -- `--synthetic_steps` of them -- and the text priors come from `TextSR.synthetic_text_prior()`;
everything between the loader and the optimizer step is the real path.  `--demo_dir DIR --resume CKPT` super-resolves a folder of images
(any sizes; resized on the GPU) into `--demo_out`; with `--demo_tile` a wide image keeps its aspect ratio and goes through the model in
overlapping windows (`--demo_line_read` with `--rec crnn`: its text is then ONE read of the line, not the windows' reads joined with
`|`); with `--demo_boxes BOXDIR` the folder holds whole photos and BOXDIR one text file of quadrilaterals per photo, each
rectified on the GPU and super-resolved as a crop of its own; with `--demo_paste` on top every photo is also enlarged by the scale factor on
the GPU, its SR regions are warped back into their quadrilaterals and blended in (`--demo_paste_feather F`: the width of the blended edge
in SR pixels, 0 for a hard edge), and written as `<stem>_photo_sr.png`; with `--demo_polygons` a line of a box file may also name a curved
word by a polygon (2k points, k along the top edge and k along the bottom, as CTW1500 and Total-Text write them), which is straightened
strip by strip on the GPU (polygon regions are written as files; `--demo_paste_polygons` on top of `--demo_paste` also warps them back into
the photo, strip by strip, in box-file order with the quadrilaterals); with `--demo_detect` in place of `--demo_boxes` the box files are
written by the run itself: the text regions of every photo are found on the GPU by a classical, integer recipe (utils/detect.py) into
`<demo_out>/boxes`, and the run goes on as with `--demo_boxes <demo_out>/boxes` (`--demo_detect_oriented` on top: the regions are
rotated quadrilaterals along the text's own direction, so slanted and vertical text is found too; `--demo_detect_local [C]` on top: a
threshold of its own per C x C cell of the working map, so a faint word is not lost to a strong edge elsewhere; `--demo_detect_curved`
on top, in place of `--demo_detect_oriented`: a bowed line is written as a polygon cut by vertical lines along its centre line and
the run reads its box files as `--demo_polygons` does).  `--train_state PATH` makes a training run continuable: the same command line starts the
run or, when PATH exists, continues it bit for bit.  `--ema DECAY` keeps an exponential moving average of the trained weights; the
validation passes score it and the best-model checkpoints hold it.  `--manmade_degrade` synthesises the LR training images from the HR images on the GPU
(`--cutblur`: with the reference's cutblur on top; `--jpeg_degrade LO,HI`: with JPEG artefacts of a random quality on the resized LR image; `--psf_blur KINDS`: with a random motion, defocus or elongated-Gaussian blur of the HR pixels first); `--train_hr_dir DIR` trains from a folder of HR images alone (no LMDB); `--train_words FILE` trains from a word list alone: the HR images are rendered on the GPU (`--train_words_fonts DIR`: in the fonts of a directory; `--train_words_epoch N`: samples per epoch).  Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N main.py ...` (one process
per GPU, RCCL gradient all-reduce; replaces nn.DataParallel)."""
import argparse
import csv
import functools
import os

import yaml


class AttrDict(dict):
    """Tiny stand-in for easydict.EasyDict (not installed here): attribute access, recursive."""

    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = AttrDict(v) if isinstance(v, dict) else v

    __getattr__ = dict.get
    __setattr__ = dict.__setitem__


def synthetic_loader(batch_size, steps, seed, labels=False):
    """labels=True: a 4th item of seeded random words (the label strings a recogniser's accuracy is counted against; on noise
    images they only exercise the accuracy path, they say nothing about the recogniser)."""
    import numpy as np
    from dpmn_amd.utils import synth
    for i in range(steps):
        b = synth.synth_batch(batch_size, seed=seed + i)
        if not labels:
            yield b["images_hr"], b["images_lr"], b["label_vecs"]
            continue
        rng = np.random.RandomState(seed + i)
        words = ["".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz0123456789"), rng.randint(1, 9))) for _ in range(batch_size)]
        yield b["images_hr"], b["images_lr"], b["label_vecs"], words


def recogniser(mission, args):
    """--rec crnn: the native CRNN of config TRAIN.VAL.crnn_pretrained (TextBase.CRNN_init); --rec aster: the native ASTER of
    config TRAIN.VAL.rec_pretrained (TextBase.Aster_init) -> word accuracy in test / eval and best-model selection by accuracy.
    --rec moran: the native MORAN of config TRAIN.VAL.moran_pretrained (TextBase.MORAN_init).  --rec aster / --rec moran without
    configured weights: accuracy is not computed (None)."""
    if args.rec == "crnn":
        return mission.CRNN_init()
    val = getattr(mission.config.TRAIN, "VAL", None)
    if args.rec == "aster" and val is not None and getattr(val, "rec_pretrained", None):
        return mission.Aster_init()[0]
    if args.rec == "moran" and val is not None and getattr(val, "moran_pretrained", None):
        return mission.MORAN_init()
    print("--rec %s: recogniser not built (only --rec crnn is); accuracy is not computed" % args.rec)
    return None


DEMO_BOXES_NEEDS_DIR = "main.py: --demo_boxes needs --demo_dir: the photos whose regions the box files name are read from that folder"
DEMO_PASTE_NEEDS_BOXES = "main.py: --demo_paste needs --demo_boxes: the SR regions are pasted back into the quadrilaterals that the box files name"
DEMO_POLYGONS_NEEDS_BOXES = "main.py: --demo_polygons needs --demo_boxes: the polygons of curved words are read from the box files"
DEMO_PASTE_POLYGONS_NEEDS = ("main.py: --demo_paste_polygons needs --demo_paste and --demo_polygons: it pastes the SR regions of the polygons "
                             "that --demo_polygons reads into the photo that --demo_paste writes")
DEMO_PASTE_FEATHER = "main.py: --demo_paste_feather must be a finite number >= 0 (the width of the blended edge in SR pixels; 0: a hard edge)"
DEMO_DETECT_NEEDS_DIR = "main.py: --demo_detect needs --demo_dir: the text regions are looked for in the photos of that folder"
DEMO_DETECT_OR_BOXES = ("main.py: --demo_detect does not combine with --demo_boxes or --demo_polygons: it writes the box files itself, as "
                        "upright rectangles (correct them by hand and pass them with --demo_boxes in a second run)")
DEMO_DETECT_GAP = "main.py: --demo_detect_gap must be 1 .. 64 (the longest gap between letters, in pixels of the working map, that joins a word)"
DEMO_DETECT_FLOOR = "main.py: --demo_detect_floor must be 1 .. 255 (the least gradient of the luma that counts as an edge of a letter)"
DEMO_DETECT_FLAGS_NEED = "main.py: --demo_detect_gap and --demo_detect_floor need --demo_detect"
DEMO_DETECT_ORIENTED_NEEDS = ("main.py: --demo_detect_oriented needs --demo_detect: it makes the regions that --demo_detect finds rotated "
                              "quadrilaterals along the text's own direction")


def demo_detect_setting(args):
    """--demo_detect and its two numbers, checked -> None without the flag, else (gap, floor).  ValueError (the message without its
    'main.py: ') for the flag without --demo_dir or with --demo_boxes / --demo_polygons, a number outside its range, or a number or
    --demo_detect_oriented without the flag."""
    from dpmn_amd.utils.detect import FLOOR, GAP, MAX_GAP
    gap, floor = getattr(args, "demo_detect_gap", None), getattr(args, "demo_detect_floor", None)
    if not getattr(args, "demo_detect", False):
        if getattr(args, "demo_detect_oriented", False):
            raise ValueError(DEMO_DETECT_ORIENTED_NEEDS[len("main.py: "):])
        if gap is not None or floor is not None:
            raise ValueError(DEMO_DETECT_FLAGS_NEED[len("main.py: "):])
        return None
    if not getattr(args, "demo_dir", None):
        raise ValueError(DEMO_DETECT_NEEDS_DIR[len("main.py: "):])
    if getattr(args, "demo_boxes", None) or getattr(args, "demo_polygons", False):
        raise ValueError(DEMO_DETECT_OR_BOXES[len("main.py: "):])
    gap, floor = GAP if gap is None else int(gap), FLOOR if floor is None else int(floor)
    if not 1 <= gap <= MAX_GAP:
        raise ValueError(DEMO_DETECT_GAP[len("main.py: "):])
    if not 1 <= floor <= 255:
        raise ValueError(DEMO_DETECT_FLOOR[len("main.py: "):])
    return gap, floor


DEMO_DETECT_LOCAL_NEEDS = ("main.py: --demo_detect_local needs --demo_detect: it gives the detector of --demo_detect a threshold of its own per "
                           "cell of the working map")
DEMO_DETECT_LOCAL_RANGE = "main.py: --demo_detect_local must be 32 .. 1024 (the side of a cell in pixels of the working map; 1024: one cell)"


DEMO_DETECT_CURVED_NEEDS = ("main.py: --demo_detect_curved needs --demo_detect: it writes the bowed lines among the regions that --demo_detect "
                            "finds as polygons")
DEMO_DETECT_CURVED_OR_ORIENTED = ("main.py: --demo_detect_curved does not combine with --demo_detect_oriented: the polygons are cut by vertical "
                                  "lines from the components of the row pass alone")


def demo_detect_curved_setting(args):
    """--demo_detect_curved, checked -> False without the flag, else True: the run then reads its own box files as --demo_polygons
    does.  ValueError (the message without its 'main.py: ') for the flag without --demo_detect or with --demo_detect_oriented."""
    if not getattr(args, "demo_detect_curved", False):
        return False
    if not getattr(args, "demo_detect", False):
        raise ValueError(DEMO_DETECT_CURVED_NEEDS[len("main.py: "):])
    if getattr(args, "demo_detect_oriented", False):
        raise ValueError(DEMO_DETECT_CURVED_OR_ORIENTED[len("main.py: "):])
    return True


def demo_detect_local_setting(args):
    """--demo_detect_local, checked -> 0 without the flag, else the cell side C.  ValueError (the message without its 'main.py: ') for
    the flag without --demo_detect or a C outside 32 .. 1024."""
    from dpmn_amd.utils.detect import MAP_SIDE, MIN_LOCAL
    local = getattr(args, "demo_detect_local", None)
    if local is None:
        return 0
    if not getattr(args, "demo_detect", False):
        raise ValueError(DEMO_DETECT_LOCAL_NEEDS[len("main.py: "):])
    if not MIN_LOCAL <= int(local) <= MAP_SIDE:
        raise ValueError(DEMO_DETECT_LOCAL_RANGE[len("main.py: "):])
    return int(local)


DEMO_CONF_NEEDS_DIR = ("main.py: --demo_conf, --demo_upright and --demo_min_conf need --demo_dir: the confidence is that of the reads of the "
                       "images of that folder")
DEMO_CONF_OR_TILE = "main.py: --demo_conf, --demo_upright and --demo_min_conf do not combine with --demo_tile: a window of a line is not a word"
DEMO_MIN_CONF_NEEDS_BOXES = ("main.py: --demo_min_conf needs --demo_boxes or --demo_detect: it drops candidate regions of a photo by the "
                             "confidence of their SR read")
DEMO_MIN_CONF_RANGE = "main.py: --demo_min_conf must lie strictly between 0 and 1 (a confidence is a geometric-mean probability)"


def demo_conf_setting(args):
    """--demo_conf, --demo_upright, --demo_min_conf C, checked -> None without the three, else TextSR.demo's keywords
    {confidence, upright, min_conf} (--demo_conf is implied by the other two).  ValueError (the message without its 'main.py: ') for
    a flag without --demo_dir or with --demo_tile, --demo_min_conf without --demo_boxes / --demo_detect, or C outside (0, 1)."""
    import math
    upright, c = bool(getattr(args, "demo_upright", False)), getattr(args, "demo_min_conf", None)
    if not (getattr(args, "demo_conf", False) or upright or c is not None):
        return None
    if not getattr(args, "demo_dir", None):
        raise ValueError(DEMO_CONF_NEEDS_DIR[len("main.py: "):])
    # (--demo_line_read gives a tiled line one read and one score: --demo_conf then combines with --demo_tile, the other two do not)
    if getattr(args, "demo_tile", False) and (upright or c is not None or not getattr(args, "demo_line_read", False)):
        raise ValueError(DEMO_CONF_OR_TILE[len("main.py: "):])
    if c is not None:
        if not (getattr(args, "demo_boxes", None) or getattr(args, "demo_detect", False)):
            raise ValueError(DEMO_MIN_CONF_NEEDS_BOXES[len("main.py: "):])
        c = float(c)
        if not (math.isfinite(c) and 0.0 < c < 1.0):
            raise ValueError(DEMO_MIN_CONF_RANGE[len("main.py: "):])
    return {"confidence": True, "upright": upright, "min_conf": c}


DEMO_EVAL_NEEDS_DIR = "main.py: --demo_eval needs --demo_dir: the regions that are scored are those of the photos of that folder"
DEMO_EVAL_NEEDS_BOXES = ("main.py: --demo_eval needs --demo_detect or --demo_boxes: it scores the regions of the run's box files against "
                         "the ground truth")


def demo_eval_setting(args):
    """--demo_eval GTDIR, checked -> None without the flag, else GTDIR.  ValueError (the message without its 'main.py: ') for the flag
    without --demo_dir or without a box source (--demo_detect or --demo_boxes), and for a GTDIR that is not a directory."""
    gt_dir = getattr(args, "demo_eval", None)
    if not gt_dir:
        return None
    if not getattr(args, "demo_dir", None):
        raise ValueError(DEMO_EVAL_NEEDS_DIR[len("main.py: "):])
    if not (getattr(args, "demo_detect", False) or getattr(args, "demo_boxes", None)):
        raise ValueError(DEMO_EVAL_NEEDS_BOXES[len("main.py: "):])
    if not os.path.isdir(gt_dir):
        raise ValueError("--demo_eval %s is not a directory" % gt_dir)
    return gt_dir


def demo_eval(rows, demo_dir, box_dir, gt_dir, out_dir, device, recogniser=True, conf=False, upright=False, lexicon=False, min_conf=False,
              spaces=True, lm=False):
    """--demo_eval: the rows TextSR.demo returned for the photos of demo_dir and the box files of box_dir, scored against
    gt_dir/<stem>.txt (or gt_<stem>.txt) by utils/detect_eval.py with the overlap counts of ops.region_overlap_counts on `device`;
    writes out_dir/detect_eval.csv and prints one line with the totals -> (records, totals).  The lines of a box file without a row
    (regions the run refused, or dropped under --demo_min_conf) are left out.  conf / upright / lexicon / min_conf: which columns
    the rows hold; recogniser=False: the e2e columns stay empty; spaces=False: the rows of --demo_line_read; lm: the rows hold sr_lm,
    sr_lm_score (--rec_beam / --rec_lm), scored end to end as the lexicon's word is (e2e_lm_*)."""
    from dpmn_amd import ops
    from dpmn_amd.utils import detect_eval as de
    stems = list(dict.fromkeys(os.path.splitext(f)[0] for f in sorted(os.listdir(demo_dir))
                               if os.path.isfile(os.path.join(demo_dir, f)) and not f.lower().endswith(".txt")))
    return de.evaluate_dir(stems, de.row_reads(rows, conf, upright, lexicon, min_conf, **({"lm": True} if lm else {})), box_dir, gt_dir,
                           os.path.join(out_dir, "detect_eval.csv"), lambda a, b: ops.region_overlap_counts(a, b, device), recogniser, lexicon,
                           spaces, **({"lm": True} if lm else {}))


DEMO_LINE_READ_NEEDS_TILE = ("main.py: --demo_line_read needs --demo_dir and --demo_tile: it reads a line that was super-resolved in overlapping "
                             "windows as one string")
DEMO_LINE_READ_NEEDS_CRNN = ("main.py: --demo_line_read needs --rec crnn: the frame posteriors of the CRNN are blended along the line; ASTER "
                             "and MORAN have none")
DEMO_LINE_SPACE_NEEDS = "main.py: --demo_line_space needs --demo_line_read: the spaces go into the one read of a tiled line"
DEMO_LINE_SPACE_RANGE = "main.py: --demo_line_space must be an integer 0 .. 64 (the blank line frames between two symbols that make a space; 0: none)"


def demo_line_setting(args):
    """--demo_line_read [--demo_line_space N], checked -> None without the flag, else TextSR.demo's keywords {line_read, line_space}.
    ValueError (the message without its 'main.py: ') for the flag without --demo_dir and --demo_tile or with a recogniser that is not
    the CRNN, and for N without the flag or outside 0 .. 64."""
    n = getattr(args, "demo_line_space", None)
    n = 0 if n is None else n
    if not getattr(args, "demo_line_read", False):
        if n:
            raise ValueError(DEMO_LINE_SPACE_NEEDS[len("main.py: "):])
        return None
    if not (getattr(args, "demo_dir", None) and getattr(args, "demo_tile", False)):
        raise ValueError(DEMO_LINE_READ_NEEDS_TILE[len("main.py: "):])
    if getattr(args, "rec", None) != "crnn":
        raise ValueError(DEMO_LINE_READ_NEEDS_CRNN[len("main.py: "):])
    if isinstance(n, bool) or n != int(n) or not 0 <= int(n) <= 64:
        raise ValueError(DEMO_LINE_SPACE_RANGE[len("main.py: "):])
    return {"line_read": True, "line_space": int(n)}


def paste_feather(args):
    """--demo_paste_feather as a float, checked; 1.0 when the flag is absent."""
    import math
    f = getattr(args, "demo_paste_feather", None)
    f = 1.0 if f is None else float(f)
    if not (math.isfinite(f) and f >= 0):
        raise ValueError(DEMO_PASTE_FEATHER[len("main.py: "):])
    return f


def rec_lexicon_setting(args, load=True):
    """--rec_lexicon FILE [--rec_lexicon_mode score|edit], checked -> (the words, the mode), or None without the flag.  The mode
    defaults to score for --rec crnn and to edit for --rec aster / moran.  Every problem is a ValueError of one line: the mode without
    the file, score with a recogniser that is not the CRNN, the flag together with --demo_tile (unless --demo_line_read is set: the
    line is then read as a sequence of the lexicon's words, in score mode only), --rec_lexicon_penalty without its two flags, the
    flag on a training run, a missing file, a file without a usable word.  load=False: only the checks that need no file contents (-> (None, mode))."""
    path, mode = getattr(args, "rec_lexicon", None), getattr(args, "rec_lexicon_mode", None)
    if not path:
        if mode:
            raise ValueError("--rec_lexicon_mode needs --rec_lexicon FILE: the word list the recogniser's answer is taken from")
        return None
    rec = getattr(args, "rec", None)
    if mode not in (None, "score", "edit"):
        raise ValueError("--rec_lexicon_mode is score or edit, got %r" % (mode,))
    if mode is None:
        mode = "score" if rec == "crnn" else "edit"
    if mode == "score" and rec != "crnn":
        raise ValueError("--rec_lexicon_mode score needs --rec crnn: the CTC likelihood of a word is computed from the CRNN's frame "
                         "posteriors; --rec %s reads under a lexicon with --rec_lexicon_mode edit" % rec)
    if getattr(args, "demo_tile", False):
        # (--demo_line_read reads a tiled line once: its posteriors are then decoded as a sequence of the lexicon's words)
        if not getattr(args, "demo_line_read", False):
            raise ValueError("--rec_lexicon does not combine with --demo_tile: a window of a line is not a word")
        if mode != "score":
            raise ValueError("--rec_lexicon_mode edit does not combine with --demo_tile --demo_line_read: the line's words come from "
                             "its frame posteriors, and there is no single string to take an edit distance to")
    rec_lexicon_penalty(args)
    if not (getattr(args, "test", False) or getattr(args, "demo_dir", None)):
        raise ValueError("--rec_lexicon needs --test or --demo_dir: the lexicon is used where SR images are read, not in training")
    if not os.path.isfile(path):
        raise ValueError("--rec_lexicon %s is not a file" % path)
    if not load:
        return None, mode
    from dpmn_amd.utils.lexicon import load_lexicon
    return load_lexicon(path, "lower"), mode


def rec_lexicon_penalty(args):
    """--rec_lexicon_penalty F, checked -> the float, 0.0 without the flag: the log-domain score every word of a tiled line's lexicon
    read pays (utils/line_words.py; negative: fewer, longer words).  ValueError of one line for a value that is not finite and for
    the flag without --rec_lexicon and --demo_line_read."""
    import math
    f = getattr(args, "rec_lexicon_penalty", None)
    if f is None:
        return 0.0
    if not (getattr(args, "rec_lexicon", None) and getattr(args, "demo_line_read", False)):
        raise ValueError("--rec_lexicon_penalty needs --rec_lexicon and --demo_line_read: it is the per-word score of a tiled line's "
                         "lexicon read")
    f = float(f)
    if not math.isfinite(f):
        raise ValueError("--rec_lexicon_penalty must be a finite number (a log-domain score added once per word)")
    return f


def rec_beam_setting(args, load=True):
    """--rec_beam W, --rec_lm FILE [--rec_lm_order N] [--rec_lm_weight A], [--rec_lm_bonus B], checked -> None without --rec_beam and
    --rec_lm, else {width, order, alpha, beta, words}: the CTC prefix beam search of utils/beam.py on the SR images (--rec_lm implies
    --rec_beam 16; words: the file's, duplicates kept, or None without a model).  Every problem is a ValueError of one line: a number
    without its flag, a recogniser that is not the CRNN, --demo_tile, a training run, a width outside 1 .. 32, an order outside
    1 .. 3, a weight or bonus that is not finite, a missing file, a file without a usable word.  load=False: the file is not read."""
    import math
    width, path = getattr(args, "rec_beam", None), getattr(args, "rec_lm", None)
    order, alpha, beta = (getattr(args, k, None) for k in ("rec_lm_order", "rec_lm_weight", "rec_lm_bonus"))
    if (order is not None or alpha is not None) and not path:
        raise ValueError("--rec_lm_order and --rec_lm_weight need --rec_lm FILE: the word list the character model is built from")
    if width is None and not path:
        if beta is not None:
            raise ValueError("--rec_lm_bonus needs --rec_beam or --rec_lm: it is added per symbol of the beam search's prefixes")
        return None
    rec = getattr(args, "rec", None)
    if rec != "crnn":
        raise ValueError("--rec_beam and --rec_lm need --rec crnn: the beam search runs on the CRNN's frame posteriors; --rec %s has its "
                         "own decoder" % rec)
    if getattr(args, "demo_tile", False):
        raise ValueError("--rec_beam and --rec_lm do not combine with --demo_tile: a line has word boundaries that the CRNN has no class "
                         "for, so a character model of words cannot weigh it")
    if not (getattr(args, "test", False) or getattr(args, "demo_dir", None)):
        raise ValueError("--rec_beam and --rec_lm need --test or --demo_dir: the beam search is used where SR images are read, not in training")
    width = 16 if width is None else width
    if isinstance(width, bool) or width != int(width) or not 1 <= int(width) <= 32:
        raise ValueError("--rec_beam must be an integer 1 .. 32 (the prefixes kept per frame), got %r" % (width,))
    order = 3 if order is None else order
    if isinstance(order, bool) or order != int(order) or not 1 <= int(order) <= 3:
        raise ValueError("--rec_lm_order must be 1 .. 3 (the symbols of an n-gram), got %r" % (order,))
    alpha, beta = 0.5 if alpha is None else float(alpha), 0.0 if beta is None else float(beta)
    if not math.isfinite(alpha):
        raise ValueError("--rec_lm_weight must be a finite number (the weight of the model's log-probabilities)")
    if not math.isfinite(beta):
        raise ValueError("--rec_lm_bonus must be a finite number (a log-domain score added per symbol)")
    words = None
    if path:
        if not os.path.isfile(path):
            raise ValueError("--rec_lm %s is not a file" % path)
        if load:
            from dpmn_amd.utils.beam import load_lm_words
            words = load_lm_words(path, "lower")
    return {"width": int(width), "order": int(order), "alpha": alpha, "beta": beta, "words": words, "model": bool(path)}


def lexicon_accuracies(rows, spaces=True):
    """The rows of demo_result.csv with boxes and a lexicon (file, box, label, lr_string, sr_string, sr_lexicon, sr_lexicon_score) ->
    (labelled regions, open-vocabulary accuracy, lexicon accuracy); the accuracies are None without a labelled region.
    spaces=False (the rows of --demo_line_read: a line's reads hold spaces, a filtered label none): the reads are compared with
    their spaces removed."""
    from dpmn_amd.utils.util import str_filt
    keep = (lambda s: s) if spaces else (lambda s: s.replace(" ", ""))
    labelled = [(keep(str_filt(r[2], "lower")), keep(r[4]), keep(r[5])) for r in rows if str_filt(r[2], "lower")]
    if not labelled:
        return 0, None, None
    n = len(labelled)
    return n, round(sum(t == s for t, s, _ in labelled) / n, 4), round(sum(t == w for t, _, w in labelled) / n, 4)


TRAIN_WORDS_OR_HR_DIR = ("main.py: --train_words and --train_hr_dir are two sources of the HR training images (a word list rendered on the "
                         "GPU, a folder of images); give one of them")
TRAIN_WORDS_FONTS_NEEDS = "main.py: --train_words_fonts needs --train_words: the fonts are those the words are rendered in"


TRAIN_WORDS_FX_NEEDS = ("main.py: --train_words_fx and --train_words_backgrounds need --train_words: outline, shadow and texture are drawn "
                        "on the rendered words")


def train_words_fx(args, atlases=None):
    """--train_words_fx KINDS [--train_words_fx_prob P] [--train_words_backgrounds DIR], checked -> the utils.render.RenderFx of the
    run (atlases: those the words are rendered from), or None without the flags.  Every problem is a SystemExit of one line: the flags
    without --train_words, an unknown kind, a probability outside 0 .. 1, texture without the folder or the folder without texture, a
    folder that is missing or holds no image PIL can open."""
    kinds, folder = getattr(args, "train_words_fx", None), getattr(args, "train_words_backgrounds", None)
    if not kinds and not folder:
        return None
    if not getattr(args, "train_words", None):
        raise SystemExit(TRAIN_WORDS_FX_NEEDS)
    if not kinds:
        raise SystemExit("main.py: --train_words_backgrounds needs --train_words_fx texture: the photos are the texture's backgrounds")
    from dpmn_amd.utils import render
    kinds = [k.strip() for k in str(kinds).split(",")]
    prob = getattr(args, "train_words_fx_prob", None)
    prob = 0.5 if prob is None else prob
    try:
        render.fx_kinds(kinds, prob, bool(folder))
    except ValueError as e:
        raise SystemExit("main.py: %s" % e)
    pool = None
    if folder:
        if not os.path.isdir(folder):
            raise SystemExit("main.py: --train_words_backgrounds %s is not a directory" % folder)
        try:
            pool = render.load_backgrounds(folder)
        except ValueError as e:
            raise SystemExit("main.py: --train_words_backgrounds %s" % e)
    return render.RenderFx(kinds, prob, pool, atlases)


TRAIN_WORDS_WARP_NEEDS = ("main.py: --train_words_warp needs --train_words: perspective, rotate and curve distort the rendered words")


def train_words_warp(args, atlases=None):
    """--train_words_warp KINDS [--train_words_warp_prob P] [--train_words_warp_persp F] [--train_words_warp_angle DEG]
    [--train_words_warp_curve F], checked -> the utils.render.RenderWarp of the run (atlases: those the words are rendered from; None:
    the values are only checked), or None without the flag.  Every problem is a SystemExit of one line: the flag without --train_words,
    an unknown kind, a probability outside 0 .. 1, a magnitude outside its range."""
    kinds = getattr(args, "train_words_warp", None)
    if not kinds:
        return None
    if not getattr(args, "train_words", None):
        raise SystemExit(TRAIN_WORDS_WARP_NEEDS)
    from dpmn_amd.utils import render
    kinds = [k.strip() for k in str(kinds).split(",")]
    val = lambda name, default: default if getattr(args, name, None) is None else getattr(args, name)
    setting = (val("train_words_warp_prob", 0.5), val("train_words_warp_persp", 0.15), val("train_words_warp_angle", 10.0),
               val("train_words_warp_curve", 0.2))
    try:
        render.warp_kinds(kinds, *setting)
    except ValueError as e:
        raise SystemExit("main.py: %s" % e)
    return None if atlases is None else render.RenderWarp(kinds, *setting, atlases=atlases)


def train_words_source(args, voc_type):
    """--train_words FILE [--train_words_fonts DIR] [--train_words_epoch N] -> (words, atlases, epoch size, fx[, warp]), or None without
    the flag; fx: the RenderFx of --train_words_fx, or None; warp, only with --train_words_warp: its RenderWarp.  Every problem is a
    SystemExit of one line: the two-sources conflict, a missing file, a file without a usable word, a font directory without a usable
    font, an epoch size below 1, and those of train_words_fx and train_words_warp."""
    path, fonts = getattr(args, "train_words", None), getattr(args, "train_words_fonts", None)
    if not path:
        if fonts:
            raise SystemExit(TRAIN_WORDS_FONTS_NEEDS)
        train_words_fx(args)
        train_words_warp(args)
        return None
    if getattr(args, "train_hr_dir", None):
        raise SystemExit(TRAIN_WORDS_OR_HR_DIR)
    from dpmn_amd.utils import render
    epoch = getattr(args, "train_words_epoch", None)
    epoch = render.DEFAULT_EPOCH if epoch is None else int(epoch)
    train_words_warp(args)
    if epoch < 1:
        raise SystemExit("main.py: --train_words_epoch must be a positive number of samples, got %d" % epoch)
    if not os.path.isfile(path):
        raise SystemExit("main.py: --train_words %s is not a file" % path)
    words = render.read_words(path, voc_type)
    files = None
    if fonts:
        if not os.path.isdir(fonts):
            raise SystemExit("main.py: --train_words_fonts %s is not a directory" % fonts)
        files = render.font_files(fonts)
        if not files:
            raise SystemExit("main.py: --train_words_fonts %s holds no *.ttf / *.otf file" % fonts)
    try:
        atlases = render.build_atlases(files)
    except ValueError:
        raise SystemExit("main.py: --train_words_fonts %s holds no font that PIL can open" % fonts)
    source, warp = (words, atlases, epoch, train_words_fx(args, atlases)), train_words_warp(args, atlases)
    return source + (warp,) if warp else source


def main(config, args):
    words_on = bool(getattr(args, "train_words", None))
    if words_on and getattr(args, "train_hr_dir", None):
        raise SystemExit(TRAIN_WORDS_OR_HR_DIR)
    if getattr(args, "train_words_fonts", None) and not words_on:
        raise SystemExit(TRAIN_WORDS_FONTS_NEEDS)
    if not words_on:
        train_words_fx(args)
    train_words_warp(args)
    if getattr(args, "cutblur", False) and not (getattr(args, "manmade_degrade", False) or getattr(args, "train_hr_dir", None) or words_on):
        raise SystemExit("main.py: --cutblur needs --manmade_degrade (or --train_hr_dir): it mixes columns of the HR image into the "
                         "synthesised LR image")
    from dpmn_amd.utils.jpeg import jpeg_setting
    try:
        jpeg = jpeg_setting(args)
    except ValueError as e:
        raise SystemExit("main.py: %s" % e)
    if jpeg is not None and not (getattr(args, "manmade_degrade", False) or getattr(args, "train_hr_dir", None) or words_on):
        raise SystemExit("main.py: --jpeg_degrade needs --manmade_degrade (or --train_hr_dir): the JPEG artefacts are put on the "
                         "synthesised LR images")
    from dpmn_amd.utils.psf import psf_setting
    try:
        psf = psf_setting(args)
    except ValueError as e:
        raise SystemExit("main.py: %s" % e)
    if psf is not None and not (getattr(args, "manmade_degrade", False) or getattr(args, "train_hr_dir", None) or words_on):
        raise SystemExit("main.py: --psf_blur needs --manmade_degrade (or --train_hr_dir or --train_words): the point-spread function "
                         "blurs the HR pixels that the LR images are synthesised from")
    if getattr(args, "demo_tile", False) and not getattr(args, "demo_dir", None):
        raise SystemExit("main.py: --demo_tile needs --demo_dir: it super-resolves the wide images of that folder in overlapping windows")
    try:
        detect_curved = demo_detect_curved_setting(args)
        detect = demo_detect_setting(args)
        detect_local = demo_detect_local_setting(args)
    except ValueError as e:
        raise SystemExit("main.py: %s" % e)
    if getattr(args, "demo_boxes", None) and not getattr(args, "demo_dir", None):
        raise SystemExit(DEMO_BOXES_NEEDS_DIR)
    if getattr(args, "demo_paste", False) and not (getattr(args, "demo_boxes", None) or detect):
        raise SystemExit(DEMO_PASTE_NEEDS_BOXES)
    if getattr(args, "demo_polygons", False) and not getattr(args, "demo_boxes", None):
        raise SystemExit(DEMO_POLYGONS_NEEDS_BOXES)
    # (--demo_detect_curved writes polygons into its box files: the run reads them as --demo_polygons does)
    polygons = bool(getattr(args, "demo_polygons", False)) or detect_curved
    if getattr(args, "demo_paste_polygons", False) and not (getattr(args, "demo_paste", False) and polygons):
        raise SystemExit(DEMO_PASTE_POLYGONS_NEEDS)
    try:
        feather = paste_feather(args)
    except ValueError as e:
        raise SystemExit("main.py: %s" % e)
    # (the lexicon is read before anything touches the GPU: a bad file or a wrong combination ends the run here)
    try:
        lex_words = rec_lexicon_setting(args)
        lex_penalty = rec_lexicon_penalty(args)
        beam_set = rec_beam_setting(args)
    except ValueError as e:
        raise SystemExit("main.py: %s" % e)
    try:
        conf_kw = demo_conf_setting(args) or {}
        line_kw = demo_line_setting(args) or {}
        eval_dir = demo_eval_setting(args)
    except ValueError as e:
        raise SystemExit("main.py: %s" % e)
    hr_dir = getattr(args, "train_hr_dir", None)
    if hr_dir and not os.path.isdir(hr_dir):
        raise SystemExit("main.py: --train_hr_dir %s is not a directory" % hr_dir)
    # (the word list is read and the atlases are rasterised before anything touches the GPU: a bad file ends the run here)
    words = train_words_source(args, getattr(getattr(config, "TRAIN", None), "voc_type", None) or "upper") if words_on else None
    import torch
    import torch.distributed as dist
    from dpmn_amd.interfaces.super_resolution import TextSR
    from dpmn_amd.utils.util import set_seed
    if "RANK" in os.environ and not dist.is_initialized():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl")
    rank = dist.get_rank() if dist.is_initialized() else 0
    # same seed on every rank while the models are built (replicas must start identical, like nn.DataParallel's replicate of
    # ONE model, base.py:160-162; the Trainer additionally broadcasts rank 0's parameters and buffers); the per-rank stream
    # (data order, augmentation, dropout seeds) is re-seeded in TextSR.train after construction
    set_seed(config.TRAIN.manualSeed)
    mission = TextSR(config, args)
    mission.rank_seed = config.TRAIN.manualSeed + rank
    bs = args.batch_size or config.TRAIN.batch_size
    os.makedirs(config.TRAIN.ckpt_dir, exist_ok=True)
    rec = recogniser(mission, args)
    lex_kw = {}
    if lex_words is not None:
        if rec is None:
            raise SystemExit("main.py: --rec_lexicon needs a recogniser, and --rec %s built none (see the line above)" % args.rec)
        from dpmn_amd.ops import Lexicon
        lex_kw = {"lexicon": Lexicon(lex_words[0], mode=lex_words[1])}
        print("rec_lexicon: %d words, mode %s" % (len(lex_words[0]), lex_words[1]))
        if line_kw:
            lex_kw["lexicon_penalty"] = lex_penalty
    beam_kw = {}
    if beam_set is not None:
        if not callable(getattr(rec, "read_beam", None)):
            raise SystemExit("main.py: --rec_beam and --rec_lm need the native CRNN, and --rec %s built none (see the line above)" % args.rec)
        lm = None
        if beam_set["model"]:
            from dpmn_amd.ops import CharLM
            from dpmn_amd.utils.beam import build_char_lm
            lm = CharLM(build_char_lm(beam_set["words"], beam_set["order"]), beam_set["order"])
            print("rec_lm: %d words, order %d, weight %g" % (len(beam_set["words"]), beam_set["order"], beam_set["alpha"]))
        print("rec_beam: width %d, bonus %g per symbol" % (beam_set["width"], beam_set["beta"]))
        beam_kw = {"beam": {"lm": lm, "width": beam_set["width"], "alpha": beam_set["alpha"], "beta": beam_set["beta"]}}
    if line_kw and not callable(getattr(rec, "read_lines", None)):
        raise SystemExit("main.py: --demo_line_read needs the native CRNN, and --rec %s built none (see the line above)" % args.rec)
    if conf_kw and not callable(getattr(rec, "read_conf", None)):
        raise SystemExit("main.py: --demo_conf, --demo_upright and --demo_min_conf need a native recogniser (--rec crnn, aster or moran), "
                         "and --rec %s built none with a confidence (see the line above)" % args.rec)
    if getattr(args, "demo_dir", None):
        # a folder of the user's own text crops -> one <stem>_sr.png per image and demo_result.csv (TextSR.demo); the trained models
        # are loaded as for --test
        if not mission.resume:
            raise SystemExit("main.py: --demo_dir needs --resume <dir> holding the trained models (as --test does)")
        if rank != 0:
            return
        from dpmn_amd.dataset.folder import box_region_batches, box_window_batches, folder_batches, folder_window_batches
        models, psn = mission.build_models(testing=True)
        scale = config.TRAIN.down_sample_scale
        out_dir = getattr(args, "demo_out", None) or os.path.join(mission.vis_dir, "demo")
        lr_size = (config.TRAIN.height // scale, config.TRAIN.width // scale)
        box_dir = getattr(args, "demo_boxes", None)
        if detect:
            # no box files: the regions of every photo are found on the GPU (utils/detect.py) and written as <demo_out>/boxes/<stem>.txt;
            # from here the run is the one that --demo_boxes <demo_out>/boxes starts
            from dpmn_amd.dataset.folder import detect_box_files
            box_dir = os.path.join(out_dir, "boxes")
            print("%d regions detected, box files in %s"
                  % (detect_box_files(args.demo_dir, box_dir, bs, mission.device, *detect,
                                      oriented=getattr(args, "demo_detect_oriented", False), local=detect_local,
                                      **({"curved": True} if detect_curved else {})), box_dir))
        if box_dir:
            # whole photos and one box file per photo: every quadrilateral is rectified on the GPU (utils/quad.py), then goes the way
            # of a crop of the folder -- one <stem>_<k>_sr.png per region
            if not os.path.isdir(box_dir):
                raise SystemExit("main.py: --demo_boxes %s is not a directory" % box_dir)
            tile = bool(getattr(args, "demo_tile", False))
            make = box_window_batches if tile else box_region_batches
            if polygons:
                # a line of more than 4 points is a curved word, straightened strip by strip (utils/poly.py)
                make = functools.partial(make, polygons=True)
            # (--demo_upright / --demo_min_conf write boxes_read/<stem>.txt from the corner lists, which come with photos=True)
            with_photos = bool(conf_kw.get("upright") or conf_kw.get("min_conf") is not None)
            if getattr(args, "demo_paste", False):
                # every photo enlarged and its SR regions pasted back into their quadrilaterals: <stem>_photo_sr.png (utils/paste.py)
                batches = make(args.demo_dir, box_dir, bs, lr_size, mission.mask, mission.device, photos=True)
                # (--demo_paste_polygons: the polygons too, strip by strip, in box-file order with the quadrilaterals: utils/paste_poly.py)
                rows = mission.demo(models, psn, batches, out_dir, rec=rec, tile=tile, chunk=bs, boxes=True, paste=True, feather=feather,
                                    paste_polygons=bool(getattr(args, "demo_paste_polygons", False)), **lex_kw, **conf_kw, **line_kw, **beam_kw)
            else:
                batches = make(args.demo_dir, box_dir, bs, lr_size, mission.mask, mission.device, **({"photos": True} if with_photos else {}))
                rows = mission.demo(models, psn, batches, out_dir, rec=rec, tile=tile, chunk=bs, boxes=True, **lex_kw, **conf_kw, **line_kw,
                                    **beam_kw)
            if lex_kw:
                # (with the confidence columns sr_string is column 5 and the lexicon's word follows sr_conf and turned)
                lex_rows = [r[:4] + [r[5], r[7 + bool(conf_kw["upright"])]] for r in rows] if conf_kw else rows
                # (a line read holds spaces and a filtered label none: there both sides are compared without them)
                print("accuracy %s accuracy_lexicon %s over %d labelled regions"
                      % tuple(lexicon_accuracies(lex_rows, spaces=not line_kw)[i] for i in (1, 2, 0)))
            print("%d regions super-resolved into %s" % (len(rows), out_dir))
            if eval_dir:
                # the run's regions and reads scored against the ground truth of GTDIR: detect_eval.csv (utils/detect_eval.py)
                demo_eval(rows, args.demo_dir, box_dir, eval_dir, out_dir, mission.device, recogniser=rec is not None, conf=bool(conf_kw),
                          upright=bool(conf_kw.get("upright")), lexicon=bool(lex_kw), min_conf=conf_kw.get("min_conf") is not None,
                          spaces=not line_kw, lm=bool(beam_kw))
            return
        if getattr(args, "demo_tile", False):
            # wide images keep their aspect ratio: overlapping LR windows per image, one stitched <stem>_sr.png (utils/tile.py)
            batches = folder_window_batches(args.demo_dir, bs, lr_size, mission.mask, mission.device)
            # (--demo_line_read: one read per line instead of the windows' reads joined with '|'; with it --demo_conf combines)
            # (... and so does --rec_lexicon: lex_kw is empty otherwise, rec_lexicon_setting refused it)
            rows = mission.demo(models, psn, batches, out_dir, rec=rec, tile=True, chunk=bs, **lex_kw, **conf_kw, **line_kw)
        else:
            batches = folder_batches(args.demo_dir, bs, lr_size, mission.mask, mission.device)
            rows = mission.demo(models, psn, batches, out_dir, rec=rec, **lex_kw, **conf_kw, **beam_kw)
        print("%d images super-resolved into %s" % (len(rows), out_dir))
        return
    if args.test:
        result_path = os.path.join(config.TRAIN.ckpt_dir, "test_result.csv")
        if rank == 0 and not os.path.exists(result_path):
            with open(result_path, "w+") as out:
                csv.writer(out).writerow(["recognizer", "subset", "accuracy", "psnr", "ssim"] + (["accuracy_lexicon"] if lex_kw else [])
                                         + (["accuracy_lm"] if beam_kw else []))
        if args.test_data_dir and os.path.isdir(args.test_data_dir):       # a TextZoom LMDB directory (needs the lmdb package)
            from dpmn_amd.dataset.textzoom import sr_batches
            loader = sr_batches(mission.get_test_data(args.test_data_dir)[1], mission.device, mission.mask)
        else:
            loader = synthetic_loader(bs, args.synthetic_steps, 1000 + rank, labels=rec is not None)
        res = mission.test(loader, rec=rec, display=args.vis_dir is not None and rank == 0, **lex_kw, **beam_kw)
        if rank == 0:
            with open(result_path, "a") as out:
                csv.writer(out).writerow([args.rec, "synthetic", res["accuracy"], res["psnr_avg"], res["ssim_avg"]]
                                         + ([res["accuracy_lexicon"]] if lex_kw else []) + ([res["accuracy_lm"]] if beam_kw else []))
            if lex_kw:
                print("accuracy_lexicon %s" % res["accuracy_lexicon"])
            if beam_kw:
                print("accuracy_lm %s" % res["accuracy_lm"])
            print("psnr %.4f ssim %.4f accuracy %s over %d synthetic batches" % (res["psnr_avg"], res["ssim_avg"], res["accuracy"],
                                                                                args.synthetic_steps))
    else:
        log_path = os.path.join(config.TRAIN.ckpt_dir, "log.csv")
        if rank == 0 and not os.path.exists(log_path):
            with open(log_path, "w+") as out:
                csv.writer(out).writerow(["epoch", "dataset", "accuracy", "psnr_avg", "ssim_avg", "best", "best_sum"])
        dirs = config.TRAIN.train_data_dir or []
        if words or hr_dir or (dirs and all(os.path.isdir(d) for d in dirs)):       # TextZoom LMDBs from the config, like base.py:85-103, --train_hr_dir or --train_words
            from dpmn_amd.dataset.textzoom import sr_batches
            world = dist.get_world_size() if dist.is_initialized() else 1
            if bs % world != 0 or bs // world < 2:
                raise SystemExit("main.py: batch_size %d does not shard over %d ranks in per-rank batches of >= 2 images (the global batch "
                                 "stays batch_size: nn.DataParallel's scatter, base.py:160-162)" % (bs, world))
            # per-rank shard of a per-epoch permutation (DistributedSampler); --train_words: of the epoch's sample numbers
            dl = (mission.get_train_data(train_words=words) if words else mission.get_train_data())[1]
            words_fp = None
            if words:
                from dpmn_amd.utils.render import words_setting
                words_fp = words_setting(*words)
            val_dirs = (config.TRAIN.VAL or {}).get("val_data_dir") or []
            val_dls = mission.get_val_data()[1] if val_dirs and all(os.path.isdir(d) for d in val_dirs) else []
            # eval every VAL.valInterval over every validation subset + best-model checkpoints (super_resolution.py:283-337)
            # one entry per validation subset (easy / medium / hard): evaluated, logged and check-pointed separately, best model by the sum
            val_loader = {name: (lambda v=vdl: sr_batches(v, mission.device, mission.mask))
                          for name, vdl in zip(subset_names(val_dirs), val_dls)} if val_dls else None
            mission.train(lambda epoch: sr_batches(dl, mission.device, mission.mask), epochs=config.TRAIN.epochs,
                          sampler=getattr(mission, "train_sampler", None), val_loader=val_loader, rec=rec,
                          display=args.vis_dir is not None, state_path=getattr(args, "train_state", None), ema_decay=getattr(args, "ema", None),
                          train_words=words_fp)
        else:
            # (a callable, not a one-shot generator: a run continued from --train_state walks the epoch again up to where it stopped)
            mission.train(lambda epoch: synthetic_loader(bs, args.synthetic_steps, 2000 + rank), steps=args.synthetic_steps, rec=rec,
                          display=args.vis_dir is not None, epochs=1, state_path=getattr(args, "train_state", None), ema_decay=getattr(args, "ema", None))


def ema_decay_arg(text):
    """--ema DECAY: a float with 0 < DECAY < 1 (NaN fails both comparisons)"""
    try:
        d = float(text)
    except ValueError:
        d = float("nan")
    if not 0.0 < d < 1.0:
        raise argparse.ArgumentTypeError("--ema must be a decay with 0 < DECAY < 1, got %r" % text)
    return d


def subset_names(val_dirs):
    """One key per validation directory: its leaf name (the reference's data_name, super_resolution.py:286), made unique -- two
    directories with the same leaf get their parent in front, and a leaf that equals one of train()'s bookkeeping keys
    ('epoch', 'score') gets the parent too -- so that no subset silently replaces another in the per-subset tables."""
    norm = [os.path.normpath(d) for d in val_dirs]
    leaf = [os.path.basename(d) for d in norm]
    names = []
    for d, name in zip(norm, leaf):
        if leaf.count(name) > 1 or name in ("epoch", "score", ""):
            name = (os.path.basename(os.path.dirname(d)) + "_" + name).strip("_") or d
        while name in names or name in ("epoch", "score"):
            name += "_"
        names.append(name)
    return names


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='DPMN scene-text SR on MI355X (reference CLI, main.py:37-67)')
    parser.add_argument('--arch', default='tsrn', choices=['tsrn', 'tbsrn', 'tg', 'tpgsr', 'tatt'])
    parser.add_argument('--test', action='store_true', default=False)
    parser.add_argument('--test_data_dir', type=str, default='/root/data/TextZoom/test/easy')
    parser.add_argument('--batch_size', type=int, default=None)
    parser.add_argument('--resume', type=str, default=None)
    parser.add_argument('--vis_dir', type=str, default=None)
    parser.add_argument('--rec', default='aster', choices=['aster', 'moran', 'crnn'])
    parser.add_argument('--mask', action='store_true', default=False)
    parser.add_argument('--gradient', action='store_true', default=False)
    parser.add_argument('--hd_u', type=int, default=32)
    parser.add_argument('--srb', type=int, default=5)
    parser.add_argument('--STN', action='store_true', default=False)
    parser.add_argument('--patch_size', type=str, default="4,", help='1, 2, 4, 8, 16')
    parser.add_argument('--embed_dim', type=str, default="96,")
    parser.add_argument('--window_size', type=str, default="2,")
    parser.add_argument('--depths', type=str, default="1,")
    parser.add_argument('--num_heads', type=str, default="6,")
    parser.add_argument('--mlp_ratio', type=str, default="4,")
    parser.add_argument('--drop_rate', type=str, default="0,")
    parser.add_argument('--attn_drop_rate', type=str, default="0,")
    parser.add_argument('--drop_path_rate', type=str, default="0.1,")
    parser.add_argument('--rotate_train', type=float, default=0.)
    parser.add_argument('--rotate_test', type=float, default=0.)
    parser.add_argument('--stu_iter_b1', type=int, default=1)
    parser.add_argument('--stu_iter_b2', type=int, default=1)
    parser.add_argument('--tpg', default='visionlan', type=str, choices=['aster', 'moran', 'crnn', 'visionlan', None])
    parser.add_argument('--rec_path', type=str, default=None)
    parser.add_argument('--font_path', type=str, default=None)
    parser.add_argument('--sr_share', action='store_true', default=False)
    parser.add_argument('--alpha', type=float, default=0.5)
    parser.add_argument('--window_num', type=int, default=3)
    parser.add_argument('--synthetic_prior', action='store_true', default=False,
                        help='seeded noise text priors instead of the VisionLAN + glyph-atlas prior of --tpg visionlan')
    parser.add_argument('--synthetic_steps', type=int, default=20, help='number of synthetic batches to run (no dataset reader here)')
    parser.add_argument('--demo_dir', type=str, default=None,
                        help='super-resolve every image of this directory with the models of --resume (no HR images, no metrics)')
    parser.add_argument('--demo_out', type=str, default=None, help='where --demo_dir writes (default: <vis_dir>/demo)')
    parser.add_argument('--demo_tile', action='store_true', default=False,
                        help='with --demo_dir: an image wider than the LR aspect keeps its aspect ratio and is super-resolved in '
                             'overlapping windows that are blended into one image')
    parser.add_argument('--demo_boxes', type=str, default=None, metavar='BOXDIR',
                        help='with --demo_dir: the folder holds whole photos, and BOXDIR one text file per photo (<stem>.txt or '
                             'gt_<stem>.txt, lines x1,y1,x2,y2,x3,y3,x4,y4[,transcription], corners clockwise from top-left); every '
                             'quadrilateral is rectified on the GPU and super-resolved (combines with --demo_tile)')
    parser.add_argument('--demo_paste', action='store_true', default=False,
                        help='with --demo_boxes: every photo is also enlarged by the scale factor and its super-resolved regions are '
                             'pasted back into their quadrilaterals on the GPU: one <stem>_photo_sr.png per photo (combines with '
                             '--demo_tile and --rec)')
    parser.add_argument('--demo_polygons', action='store_true', default=False,
                        help='with --demo_boxes: a line of a box file may hold a polygon of 2k points (k along the top edge, then k '
                             'along the bottom edge, clockwise; CTW1500 / Total-Text style, at most 32 per edge) for a curved word, '
                             'which is straightened strip by strip on the GPU.  Everything after the leading numbers is the '
                             'transcription (a leading #### is stripped); lines of 4 points are read as without the flag.  With '
                             '--demo_paste the polygon regions are written but not pasted (see --demo_paste_polygons)')
    parser.add_argument('--demo_paste_polygons', action='store_true', default=False,
                        help='with --demo_paste and --demo_polygons: the super-resolved polygon regions are pasted back too, every strip '
                             'through the inverse of its bilinear map, in box-file order with the quadrilaterals')
    parser.add_argument('--demo_paste_feather', type=float, default=1.0, metavar='F',
                        help='with --demo_paste: the width, in SR pixels, of the edge over which a pasted region is blended into the '
                             'photo (>= 0; 0 gives a hard edge)')
    parser.add_argument('--demo_conf', action='store_true', default=False,
                        help='with --demo_dir and a native recogniser (--rec crnn / aster / moran): demo_result.csv gains lr_conf and '
                             'sr_conf, the geometric-mean symbol probability of each read (exp(score / terms), utils/confidence.py), at no '
                             'extra forward pass; implied by --demo_upright and --demo_min_conf; not with --demo_tile')
    parser.add_argument('--demo_upright', action='store_true', default=False,
                        help='with --demo_dir: every LR image is read as it is and turned by 180 degrees, and goes through the model in '
                             'the direction of the more confident read (column turned); with box files the regions are written in '
                             'their reading order to <demo_out>/boxes_read/<stem>.txt; not with --demo_tile')
    parser.add_argument('--demo_min_conf', type=float, default=None, metavar='C',
                        help='with --demo_boxes or --demo_detect: a region whose SR read is empty or less confident than C (0 < C < 1) '
                             'is dropped: no region file, not pasted, column kept = 0; not with --demo_tile')
    parser.add_argument('--demo_eval', type=str, default=None, metavar='GTDIR',
                        help='with --demo_detect or --demo_boxes: score the regions of the run\'s box files against the ground truth of '
                             'GTDIR (<stem>.txt or gt_<stem>.txt per photo; ICDAR 2015 quads, CTW1500 / Total-Text polygons, ### for '
                             'don\'t-care): precision, recall and h-mean at IoU > 0.5 by the ICDAR protocol, and end to end (a match '
                             'counts when the SR read equals the transcription), per photo and in total, into '
                             '<demo_out>/detect_eval.csv.  Regions dropped by --demo_min_conf are left out.  IoU is counted on 4 x 4 '
                             'samples per pixel on the GPU (utils/detect_eval.py)')
    parser.add_argument('--demo_line_read', action='store_true', default=False,
                        help='with --demo_tile and --rec crnn: lr_string / sr_string are ONE read of the whole line instead of the '
                             "windows' reads joined with '|': the CRNN's frame posteriors of the overlapping windows are blended along "
                             'the line, decoded once and scored once (utils/line_read.py), at no extra recogniser pass; --demo_conf then '
                             'combines with --demo_tile.  The string is over the 36 symbols of the CRNN')
    parser.add_argument('--demo_line_space', type=int, default=0, metavar='N',
                        help='with --demo_line_read: a space goes where at least N (0 .. 64) line frames lie between two symbols; a '
                             'heuristic on the blank runs, the CRNN has no space class; 0 (default) inserts none')
    parser.add_argument('--demo_detect', action='store_true', default=False,
                        help='with --demo_dir and without box files: the folder holds whole photos whose text regions are found on the '
                             'GPU by a classical recipe (gradient of the luma, Otsu threshold, run-length smoothing, connected '
                             'components, geometric filters), written as <demo_out>/boxes/<stem>.txt and then used as --demo_boxes uses '
                             'them (combines with --demo_tile, --demo_paste and --rec).  It finds well-contrasted, roughly horizontal '
                             'words and lines; it is no learned detector (not EAST or DBNet): low-contrast, vertical or strongly rotated '
                             'text is missed and very large glyphs may split into several boxes.  The files are ordinary box files: '
                             'correct them by hand and pass them with --demo_boxes')
    parser.add_argument('--demo_detect_oriented', action='store_true', default=False,
                        help='with --demo_detect: the box files hold rotated quadrilaterals along every region\'s own direction (one of '
                             '64 directions, 2.8125 degrees apart, from the second moments of its pixels) instead of upright rectangles, '
                             'so slanted and vertical text is found and rectified along its baseline.  Of a word that both smoothing '
                             'passes find one region is written, and a turned letter inside a steep word is left out; a narrow block '
                             'of short horizontal lines keeps its lines and also gets one steep region around the block, to be '
                             'deleted by hand.  Text steeper than 45 degrees is read along its longer side; whether a vertical sign reads upward '
                             'or downward cannot be told from its shape (exactly vertical text is read upward)')
    parser.add_argument('--demo_detect_curved', action='store_true', default=False,
                        help='with --demo_detect (not with --demo_detect_oriented): a bowed line -- on a bottle, an arch, a round sign -- is '
                             'written as a polygon of up to 16 points a side, cut by vertical lines along its centre line, and the run '
                             'reads its box files as --demo_polygons does (--demo_paste_polygons pastes them back); straight text keeps '
                             'its upright boxes.  Vertical cuts shear the glyphs of a steep arc: fine up to a slope of about 0.5, wrong '
                             'for a half circle; the constants are untuned (utils/detect.py)')
    parser.add_argument('--demo_detect_local', type=int, nargs='?', const=128, default=None, metavar='C',
                        help='with --demo_detect: a locally adaptive threshold -- Otsu\'s threshold per C x C cell of the working map '
                             '(32 .. 1024, 128 when C is left out), interpolated between the cell centres, instead of one threshold per '
                             'photo, so that a faint word is not lost to a strong edge elsewhere in the photo.  More clutter reaches the '
                             'shape filters in textured areas (--demo_min_conf drops it downstream); --demo_detect_floor still bounds '
                             'the threshold from below.  1024 is one cell: the regions without the flag')
    parser.add_argument('--demo_detect_gap', type=int, default=None, metavar='N',
                        help='with --demo_detect: the longest gap between letters, in pixels of the working map (the photo reduced to at '
                             'most 1024 on its long side), that still joins them into one word (1 .. 64, default 12)')
    parser.add_argument('--demo_detect_floor', type=int, default=None, metavar='N',
                        help='with --demo_detect: the least threshold on the 3 x 3 gradient of the luma (1 .. 255, default 24)')
    parser.add_argument('--gpu_resize', action='store_true', default=False,
                        help='TextZoom loaders: the bicubic resize of the decoded images runs on the GPU (same bytes as PIL)')
    parser.add_argument('--train_state', type=str, default=None,
                        help='one file that holds everything needed to continue the training run exactly: if it exists the run '
                             'continues from it, otherwise it starts fresh; rewritten at every checkpoint save and at the end')
    parser.add_argument('--ema', type=ema_decay_arg, default=None, metavar='DECAY',
                        help='training: keep an exponential moving average of the weights (0 < DECAY < 1, for example 0.999); every '
                             'validation pass scores the averaged weights and the best-model checkpoints hold them, checkpoint.pth '
                             'keeps the live ones, --train_state carries the average')
    parser.add_argument('--manmade_degrade', action='store_true', default=False,
                        help='training: the LR images are synthesised from the HR images on the GPU (blur, noise, noise reduction, '
                             'sharpening) instead of read from the LMDB')
    parser.add_argument('--cutblur', action='store_true', default=False,
                        help='with --manmade_degrade: columns on one side of a random cut of the synthesised LR image are the HR image\'s')
    parser.add_argument('--jpeg_degrade', type=str, default=None, metavar='LO,HI',
                        help='with --manmade_degrade: a synthesised LR image goes through a JPEG of a quality drawn from LO .. HI '
                             '(1 .. 100, for example 30,95; 40,40 is the fixed quality of the reference\'s helper) with probability '
                             '--jpeg_prob')
    parser.add_argument('--jpeg_prob', type=float, default=0.5, help='with --jpeg_degrade: the probability of the JPEG stage per image')
    parser.add_argument('--psf_blur', type=str, default=None, metavar='KINDS',
                        help='with --manmade_degrade: the HR pixels a synthesised LR image is made from are first blurred by a random '
                             'point-spread function, a comma list of motion (camera shake: a line at a random angle), disk (defocus) and '
                             'aniso (an elongated Gaussian), with probability --psf_prob')
    parser.add_argument('--psf_prob', type=float, default=0.5, help='with --psf_blur: the probability of the blur per image')
    parser.add_argument('--psf_radius', type=float, default=0.12,
                        help='with --psf_blur: the largest radius of the point-spread function as a fraction of the image height '
                             '(drawn from 1 pixel up to it, 10 pixels at the most)')
    parser.add_argument('--train_hr_dir', type=str, default=None,
                        help='train from this folder of HR images (optional labels.txt: file name<TAB>word); implies --manmade_degrade, '
                             'needs no LMDB')
    parser.add_argument('--train_words', type=str, default=None, metavar='FILE',
                        help='train from this word list alone (one word per line, UTF-8): the HR images are rendered on the GPU in random '
                             'fonts, sizes, colours, spacing and shear, every sample with its true label; implies --manmade_degrade, needs '
                             'no image data; not together with --train_hr_dir')
    parser.add_argument('--rec_lexicon', type=str, default=None, metavar='FILE',
                        help='with --test or --demo_dir and a recogniser: also read every SR image under this word list (one word per '
                             'line, UTF-8; filtered like --train_words, duplicates dropped): --test reports accuracy_lexicon beside '
                             'accuracy, --demo_dir writes the columns sr_lexicon and sr_lexicon_score; with --demo_tile only under '
                             '--demo_line_read: the line is then read as a sequence of the words (utils/line_words.py)')
    parser.add_argument('--rec_lexicon_penalty', type=float, default=None, metavar='F',
                        help='with --rec_lexicon and --demo_tile --demo_line_read: a log-domain score added once per word of a line\'s '
                             'lexicon read (default 0.0, untuned; negative: fewer, longer words)')
    parser.add_argument('--rec_lexicon_mode', default=None, choices=['score', 'edit'],
                        help='with --rec_lexicon: score = the word of the highest CTC likelihood under the frame posteriors (--rec crnn '
                             'only, its default), edit = the word at the least edit distance to the recognised string (any recogniser; '
                             'the default of --rec aster / moran)')
    parser.add_argument('--rec_beam', type=int, default=None, metavar='W',
                        help='with --test or --demo_dir and --rec crnn: also read every SR image by a CTC prefix beam search of W (1 .. 32) '
                             'prefixes over the frame posteriors (utils/beam.py; one HIP launch per batch): --test reports accuracy_lm '
                             'beside accuracy, --demo_dir writes the columns sr_lm and sr_lm_score; not with --demo_tile')
    parser.add_argument('--rec_lm', type=str, default=None, metavar='FILE',
                        help='a character n-gram model for the beam search, built from this word list (one word per line, UTF-8; filtered '
                             'like --rec_lexicon, but a repeated word counts as often as it is listed); implies --rec_beam 16.  The '
                             'vocabulary stays open: the model weighs every new symbol, it forbids none')
    parser.add_argument('--rec_lm_order', type=int, default=None, metavar='N', help='with --rec_lm: the n of the n-gram, 1 .. 3 (default 3)')
    parser.add_argument('--rec_lm_weight', type=float, default=None, metavar='A',
                        help='with --rec_lm: the weight of the model\'s log-probabilities in a prefix\'s score (default 0.5, untuned)')
    parser.add_argument('--rec_lm_bonus', type=float, default=None, metavar='B',
                        help='with --rec_beam or --rec_lm: a log-domain score added per symbol of a prefix (default 0.0, untuned; positive: '
                             'longer strings)')
    parser.add_argument('--train_words_fonts', type=str, default=None, metavar='DIR',
                        help='with --train_words: every *.ttf / *.otf of this directory is a font (default: PIL\'s built-in font)')
    parser.add_argument('--train_words_epoch', type=int, default=10000, metavar='N',
                        help='with --train_words: the number of rendered samples that counts as one epoch')
    parser.add_argument('--train_words_fx', type=str, default=None, metavar='KINDS',
                        help='with --train_words: a comma list of outline (a border of 1 .. 3 pixels in a contrasting colour), shadow (a '
                             'drop shadow up to 3 pixels away) and texture (a crop of a photo of --train_words_backgrounds blended into '
                             'the background); each listed kind is on per sample with probability --train_words_fx_prob')
    parser.add_argument('--train_words_fx_prob', type=float, default=0.5, help='with --train_words_fx: the probability of each kind per sample')
    parser.add_argument('--train_words_warp', type=str, default=None, metavar='KINDS',
                        help='with --train_words: a comma list of perspective (every corner of the word moves on its own), rotate (the '
                             'word turns about its centre) and curve (a parabolic baseline; the columns are displaced, the glyphs are not '
                             'turned); each listed kind is on per sample with probability --train_words_warp_prob')
    parser.add_argument('--train_words_warp_prob', type=float, default=0.5, help='with --train_words_warp: the probability of each kind per sample')
    parser.add_argument('--train_words_warp_persp', type=float, default=0.15, metavar='F',
                        help='with --train_words_warp perspective: a corner moves by up to F of the glyph height in x and in y, 0 < F <= 0.3')
    parser.add_argument('--train_words_warp_angle', type=float, default=10.0, metavar='DEG',
                        help='with --train_words_warp rotate: the angle is drawn from +-DEG degrees, 0 < DEG <= 20')
    parser.add_argument('--train_words_warp_curve', type=float, default=0.2, metavar='F',
                        help='with --train_words_warp curve: the baseline rises or sags by up to F of the glyph height, 0 < F <= 0.4')
    parser.add_argument('--train_words_backgrounds', type=str, default=None, metavar='DIR',
                        help='with --train_words_fx texture: a folder of photos (whatever PIL opens; reduced to 512 pixels on the long side)')
    args = parser.parse_args()
    if args.train_words and args.train_hr_dir:
        parser.error(TRAIN_WORDS_OR_HR_DIR[len("main.py: "):])
    if args.train_words_fonts and not args.train_words:
        parser.error(TRAIN_WORDS_FONTS_NEEDS[len("main.py: "):])
    try:
        curved = demo_detect_curved_setting(args)
        demo_detect_setting(args)
        demo_detect_local_setting(args)
    except ValueError as e:
        parser.error(str(e))
    if args.demo_boxes and not args.demo_dir:
        parser.error(DEMO_BOXES_NEEDS_DIR[len("main.py: "):])
    if args.demo_paste and not (args.demo_boxes or args.demo_detect):
        parser.error(DEMO_PASTE_NEEDS_BOXES[len("main.py: "):])
    if args.demo_polygons and not args.demo_boxes:
        parser.error(DEMO_POLYGONS_NEEDS_BOXES[len("main.py: "):])
    if args.demo_paste_polygons and not (args.demo_paste and (args.demo_polygons or curved)):
        parser.error(DEMO_PASTE_POLYGONS_NEEDS[len("main.py: "):])
    try:
        paste_feather(args)
    except ValueError as e:
        parser.error(str(e))
    try:
        rec_lexicon_setting(args, load=False)
        rec_lexicon_penalty(args)
        rec_beam_setting(args, load=False)
    except ValueError as e:
        parser.error(str(e))
    try:
        demo_conf_setting(args)
        demo_line_setting(args)
        demo_eval_setting(args)
    except ValueError as e:
        parser.error(str(e))
    config_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'config', 'super_resolution.yaml')
    config = AttrDict(yaml.load(open(config_path, 'r'), Loader=yaml.Loader))
    main(config, args)
