"""A directory of someone's own text crops as the LR input of the SR path (main.py --demo_dir, TextSR.demo): files in sorted name
order, decoded with PIL, converted to RGB, packed as a ragged batch (utils/resize.py pack_ragged), uploaded once and resized to the
model's LR size on the GPU (ops.resize_ragged_u8, byte for byte PIL's bicubic resize), then finished like a TextZoom batch
(ops.collate_u8: ToTensor and the mask channel).  The host half (`host_batches`) needs no GPU.  `folder_window_batches` (main.py
--demo_tile) keeps the aspect ratio of wide images: every image as overlapping windows of the LR size (ops.resize_windows_u8).
`FolderHR`: the same kind of directory as the HR images of a TRAINING set (main.py --train_hr_dir): the LR images are synthesised on
the GPU (dataset/textzoom.py, alignCollate_realWTLAMask(degrade=True) and sr_batches), so training needs neither LMDB nor LR images.
`box_batches` / `box_region_batches` / `box_window_batches` (main.py --demo_boxes): a directory of WHOLE photos and a directory of box
files (one quadrilateral per word, utils/quad.py); every region is rectified on the GPU (ops.quad_crop_u8) and then takes the path of a
crop of the folder.  With photos=True (main.py --demo_paste) the two generators also hand out the uploaded photos and the
quadrilaterals, which TextSR.demo(paste=True) needs to put the SR regions back (utils/paste.py).  With polygons=True (main.py
--demo_polygons) a line of a box file may name a curved word by a polygon of more than 4 points (utils/poly.py): it is rectified strip
by strip (ops.poly_crop_u8) into the same packed buffer as the quadrilaterals (ops.crop_regions_u8).
`detect_box_files` (main.py --demo_detect) writes the box files itself: the regions of every photo are found on the GPU
(ops.detect_text_u8, utils/detect.py), with oriented=True (main.py --demo_detect_oriented) as rotated quadrilaterals
(ops.detect_oriented_u8), with local=C (main.py --demo_detect_local) under a threshold of its own per C x C cell of the working map,
with curved=True (main.py --demo_detect_curved) with bowed lines as polygons among the upright boxes (ops.detect_curved_u8).
"""
import os

import numpy as np
import torch

LABELS_FILE = "labels.txt"


def host_batches(dir_, batch_size, check=None, skip_txt=False):
    """Yields (names, packed, meta) per batch of at most batch_size images: the file names and utils.resize.pack_ragged of their RGB
    pixels.  Regular files of `dir_` in sorted name order; a file PIL cannot open, or an image pack_ragged rejects (check: a callable
    (image, name) in place of utils.resize.check_image, which raises for an image it rejects), is skipped with one printed line.  A
    directory without files raises.  skip_txt: files named *.txt are passed over without a line, as box_batches passes them over."""
    from PIL import Image
    from ..utils.resize import MAX_PACKED_BYTES, check_image, pack_ragged
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("folder: batch_size must be positive, got %d" % batch_size)
    files = sorted(f for f in os.listdir(dir_) if os.path.isfile(os.path.join(dir_, f)))
    if not files:
        raise FileNotFoundError("folder: %s holds no files" % dir_)
    names, images, nbytes = [], [], 0
    for f in files:
        if skip_txt and f.lower().endswith(".txt"):
            continue
        try:
            with Image.open(os.path.join(dir_, f)) as im:
                a = np.asarray(im.convert('RGB'), dtype=np.uint8)
            (check or check_image)(a, f)
        except Exception as e:      # whatever a decoder raises on a file that is not its format, or is damaged
            print("folder: skipping %s (%s: %s)" % (f, type(e).__name__, e))
            continue
        if names and nbytes + a.size > MAX_PACKED_BYTES:      # pack_ragged's limit on a batch: this image starts the next one
            yield (names,) + pack_ragged(images)
            names, images, nbytes = [], [], 0
        names.append(f)
        images.append(a)
        nbytes += a.size
        if len(names) == batch_size:
            yield (names,) + pack_ragged(images)
            names, images, nbytes = [], [], 0
    if names:
        yield (names,) + pack_ragged(images)


def folder_batches(dir_, batch_size, lr_size, mask, device):
    """Yields (names, images_lr) per batch: images_lr (B, 3 + mask, h, w) float on `device`, (h, w) = lr_size = the config's
    (height // scale, width // scale).  Per batch one upload of the packed pixels, the ragged resize and the collate kernel."""
    from .. import ops
    h, w = lr_size
    for names, packed, meta in host_batches(dir_, batch_size):
        yield names, ops.collate_u8(ops.resize_ragged_u8(packed.to(device, non_blocking=True), meta, h, w), mask)


def folder_window_batches(dir_, batch_size, lr_size, mask, device):
    """folder_batches for wide images (main.py --demo_tile): yields (names, plan, images_lr) per batch of at most batch_size files.
    Every image is resized to the LR height with its aspect ratio kept and cut into overlapping windows of lr_size
    (ops.resize_windows_u8; utils/tile.py): images_lr (T, 3 + mask, h, w) float on `device` holds the T windows of the batch, plan
    their (image, x0) -- what ops.stitch_windows_u8 needs to put the SR windows together again.  An image of aspect w : h or less is
    one window, the image folder_batches yields.  An image whose line would be wider than utils.resize.MAX_SIDE is skipped with one
    printed line."""
    from .. import ops
    from ..utils.tile import check_line
    h, w = lr_size
    for names, packed, meta in host_batches(dir_, batch_size, check=lambda a, f: check_line(a, (h, w), f)):
        windows, plan = ops.resize_windows_u8(packed.to(device, non_blocking=True), meta, h, w)
        yield names, plan, ops.collate_u8(windows, mask)


def detect_box_files(dir_, box_dir, batch_size, device, gap=12, floor=24, oriented=False, local=0, curved=False):
    """main.py --demo_detect: the text regions of every photo of `dir_` (host_batches' files, *.txt passed over), found on the GPU
    (ops.detect_text_u8; utils/detect.py holds the recipe and its limits), written as box_dir/<stem>.txt in the format that box_batches
    reads -- an ordinary box file that can be corrected by hand and fed back with --demo_boxes.  Per batch one upload of the packed
    photos.  A photo without a region gets an empty file and one printed line.  oriented (main.py --demo_detect_oriented): the
    regions are rotated quadrilaterals along the text's own direction, in decimals (ops.detect_oriented_u8).  local (main.py
    --demo_detect_local): the cell side of the locally adaptive threshold, 0 for the one threshold per photo.  curved (main.py
    --demo_detect_curved; not with oriented): bowed lines are written as polygons, which box_batches(polygons=True) reads
    (ops.detect_curved_u8).  -> the number of boxes written."""
    from .. import ops
    from ..utils.detect import write_boxes, write_quads, write_regions
    if curved and oriented:
        raise ValueError("detect_box_files: curved does not combine with oriented")
    find, write = (ops.detect_oriented_u8, write_quads) if oriented else (ops.detect_text_u8, write_boxes)
    if curved:
        find, write = ops.detect_curved_u8, write_regions
    kw = {"local": int(local)} if local else {}      # (off: the call is the one it was)
    os.makedirs(box_dir, exist_ok=True)
    n = 0
    for names, packed, meta in host_batches(dir_, batch_size, skip_txt=True):
        found = find(packed.to(device, non_blocking=True), meta[:, 0], meta[:, 1:], gap=gap, floor=floor, names=names, **kw)
        for name, boxes in zip(names, found):
            if len(boxes) == 0:
                print("detect: no text region found in %s" % name)
            write(os.path.join(box_dir, os.path.splitext(name)[0] + ".txt"), boxes)
            n += len(boxes)
    return n


def box_batches(dir_, box_dir, batch_size, check=None, quads=False, polygons=False):
    """The host half of the box path: yields (region names, labels, packed, meta, regions) per batch -- packed / meta =
    utils.resize.pack_ragged of the batch's photos, regions = the list of (photo index in the batch, h, w, coeffs) that
    ops.quad_crop_u8 takes (utils.quad: quad_size and quad_coeffs of every quadrilateral), names and labels one per region.
    The photos are the regular files of `dir_` in sorted name order, as host_batches walks them (files named *.txt are passed over, so
    the box files may lie beside the photos).  The boxes of name.ext are read from box_dir/<stem>.txt, or else box_dir/gt_<stem>.txt
    (utils.quad.read_boxes' format).  A region is named <stem>_<k>, k = the number of its line among the file's non-empty lines from 0,
    as 3 digits; a line that is skipped keeps its number.  A photo without a box file, without a usable region, or that PIL cannot
    open is skipped with one printed line; so is a region that utils.quad.check_quad, quad_coeffs or `check` (a callable (h, w, name)
    that raises ValueError for a region size it rejects) refuses, naming the photo and the line.  A photo is never split: a batch
    closes once it holds at least batch_size regions, or once the next photo would exceed utils.resize.MAX_PACKED_BYTES.  A directory
    without files raises.  quads=True: every tuple gains a last item, the float64 (4, 2) quadrilateral of every region in photo
    coordinates (the default leaves the tuples as they are).
    polygons=True: the box files are read with utils.poly.numbered_polygons.  A line of 4 points is the quadrilateral it is without the
    flag, with the same region; a line of more points is a polygon, checked with utils.poly.check_polygon, and its region is (photo
    index, h, w, cells) of polygon_plan and polygon_cells -- what ops.poly_crop_u8 takes, ops.crop_regions_u8 a list of both kinds.  A
    polygon that check_polygon, polygon_plan or `check` refuses is skipped like a refused quadrilateral; with quads=True a polygon's
    item is its float64 (2k, 2) points."""
    from PIL import Image
    from ..utils.poly import check_polygon, numbered_polygons, polygon_cells, polygon_plan
    from ..utils.quad import check_quad, numbered_boxes, quad_coeffs, quad_size
    from ..utils.resize import MAX_PACKED_BYTES, check_image, pack_ragged
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("folder: batch_size must be positive, got %d" % batch_size)
    files = sorted(f for f in os.listdir(dir_) if os.path.isfile(os.path.join(dir_, f)))
    if not files:
        raise FileNotFoundError("folder: %s holds no files" % dir_)
    names, labels, images, regions, corners, nbytes = [], [], [], [], [], 0
    for f in files:
        stem = os.path.splitext(f)[0]
        if f.lower().endswith(".txt"):
            continue
        box_file = next((p for p in (os.path.join(box_dir, stem + ".txt"), os.path.join(box_dir, "gt_" + stem + ".txt")) if os.path.isfile(p)), None)
        if box_file is None:
            print("folder: skipping %s (no box file %s.txt or gt_%s.txt in %s)" % (f, stem, stem, box_dir))
            continue
        found = []
        for k, lineno, quad, label in (numbered_polygons if polygons else numbered_boxes)(box_file):
            try:
                if len(quad) > 4:      # (polygons only: a curved line, its cells in the place of the 8 coefficients)
                    check_polygon(quad)
                    h, w, xs = polygon_plan(quad)
                    coeffs = polygon_cells(quad, h, xs)
                else:
                    check_quad(quad)
                    h, w = quad_size(quad)
                    coeffs = quad_coeffs(quad, w, h)
                if check is not None:
                    check(h, w, "%s_%03d" % (stem, k))
            except ValueError as e:
                print("folder: skipping a region of %s (%s line %d: %s)" % (f, os.path.basename(box_file), lineno, e))
                continue
            found.append(("%s_%03d" % (stem, k), label, h, w, coeffs, quad))
        if not found:
            print("folder: skipping %s (no usable region in %s)" % (f, os.path.basename(box_file)))
            continue
        try:
            with Image.open(os.path.join(dir_, f)) as im:
                a = np.asarray(im.convert('RGB'), dtype=np.uint8)
            check_image(a, f)
        except Exception as e:      # whatever a decoder raises on a file that is not its format, or is damaged
            print("folder: skipping %s (%s: %s)" % (f, type(e).__name__, e))
            continue
        if images and nbytes + a.size > MAX_PACKED_BYTES:      # pack_ragged's limit on a batch: this photo starts the next one
            yield (names, labels) + pack_ragged(images) + ((regions, corners) if quads else (regions,))
            names, labels, images, regions, corners, nbytes = [], [], [], [], [], 0
        for name, label, h, w, coeffs, quad in found:
            names.append(name)
            labels.append(label)
            regions.append((len(images), h, w, coeffs))
            corners.append(quad)
        images.append(a)
        nbytes += a.size
        if len(names) >= batch_size:
            yield (names, labels) + pack_ragged(images) + ((regions, corners) if quads else (regions,))
            names, labels, images, regions, corners, nbytes = [], [], [], [], [], 0
    if names:
        yield (names, labels) + pack_ragged(images) + ((regions, corners) if quads else (regions,))


def box_region_batches(dir_, box_dir, batch_size, lr_size, mask, device, photos=False, polygons=False):
    """folder_batches for whole photos with box files (main.py --demo_boxes): yields (region names, labels, images_lr) per batch of
    box_batches, images_lr (R, 3 + mask, h, w) float on `device`, (h, w) = lr_size.  Per batch one upload of the packed photos, then
    the rectification of every region at its own size (ops.quad_crop_u8), the ragged resize to the LR size and the collate kernel.
    photos=True (main.py --demo_paste): every tuple gains a last item (packed, meta, owners, quads) -- the batch's photos as uploaded
    (the pack_ragged buffer on `device` and its host meta), and per region the index of its photo in the batch and its quadrilateral.
    polygons=True (main.py --demo_polygons): box_batches' -- polygons are rectified too (ops.crop_regions_u8), in box-file order."""
    from .. import ops
    h, w = lr_size
    for names, labels, packed, meta, regions, *quads in box_batches(dir_, box_dir, batch_size, quads=photos, polygons=polygons):
        packed = packed.to(device, non_blocking=True)
        crops, crop_meta = (ops.crop_regions_u8 if polygons else ops.quad_crop_u8)(packed, meta, regions)
        images_lr = ops.collate_u8(ops.resize_ragged_u8(crops, crop_meta, h, w), mask)
        if photos:
            yield names, labels, images_lr, (packed, meta, [r[0] for r in regions], quads[0])
        else:
            yield names, labels, images_lr


def box_window_batches(dir_, box_dir, batch_size, lr_size, mask, device, photos=False, polygons=False):
    """folder_window_batches for whole photos with box files (main.py --demo_boxes --demo_tile): yields (region names, labels, plan,
    images_lr) per batch of box_batches -- every rectified region keeps its aspect ratio and is cut into overlapping windows of lr_size
    (ops.resize_windows_u8), plan as folder_window_batches yields it, over the batch's regions.  A region whose line would be wider than
    utils.resize.MAX_SIDE (utils.tile.line_width of the REGION's size, not the photo's) is skipped with one printed line.
    photos=True: a last item as box_region_batches yields it.  polygons=True: as box_region_batches takes it."""
    from .. import ops
    from ..utils.tile import line_width
    h, w = lr_size
    for names, labels, packed, meta, regions, *quads in box_batches(dir_, box_dir, batch_size, check=lambda rh, rw, name: line_width(rh, rw, h, w),
                                                                    quads=photos, polygons=polygons):
        packed = packed.to(device, non_blocking=True)
        crops, crop_meta = (ops.crop_regions_u8 if polygons else ops.quad_crop_u8)(packed, meta, regions)
        windows, plan = ops.resize_windows_u8(crops, crop_meta, h, w)
        images_lr = ops.collate_u8(windows, mask)
        if photos:
            yield names, labels, plan, images_lr, (packed, meta, [r[0] for r in regions], quads[0])
        else:
            yield names, labels, plan, images_lr


class FolderHR(torch.utils.data.Dataset):
    """The images of a directory as the HR images of a training set: items (img_HR, img_HR, None, None, label) like
    textzoom.lmdbDataset_real(manmade_degrade=True) -- the HR image stands in the LR position.  Regular files of `dir_` in sorted name
    order, as host_batches walks them; a file PIL cannot open, or whose sides pack_ragged rejects, is skipped with one printed line
    (checked once, here, from the file's header; an image that then fails to decode raises in __getitem__).  Labels: an optional
    `labels.txt` in the directory with lines `file name<TAB>word` (not an image itself); a file without a line, or a directory
    without the file, gets " " (what the LMDB reader gives a missing label).  A directory without usable images raises."""

    def __init__(self, dir_, voc_type='upper'):
        super().__init__()
        from PIL import Image
        from ..utils.resize import MAX_SIDE
        self.dir, self.voc_type = dir_, voc_type
        files = sorted(f for f in os.listdir(dir_) if os.path.isfile(os.path.join(dir_, f)) and f != LABELS_FILE)
        self.labels = {}
        if os.path.isfile(os.path.join(dir_, LABELS_FILE)):
            with open(os.path.join(dir_, LABELS_FILE), encoding="utf-8") as fh:
                for line in fh:
                    name, tab, word = line.rstrip("\r\n").partition("\t")
                    if tab:
                        self.labels[name] = word
        self.files = []
        for f in files:
            try:
                with Image.open(os.path.join(dir_, f)) as im:
                    w, h = im.size
                if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
                    raise ValueError("%d x %d, sides outside 1 .. %d" % (h, w, MAX_SIDE))
            except Exception as e:      # whatever a decoder raises on a file that is not its format, or is damaged
                print("folder: skipping %s (%s: %s)" % (f, type(e).__name__, e))
                continue
            self.files.append(f)
        if not self.files:
            raise FileNotFoundError("folder: %s holds no usable images" % dir_)

    def __len__(self):
        return len(self.files)

    def __getitem__(self, index):
        from PIL import Image
        from ..utils.util import str_filt
        f = self.files[index]
        with Image.open(os.path.join(self.dir, f)) as im:
            img = im.convert('RGB')
        return img, img, None, None, str_filt(self.labels.get(f, " "), self.voc_type)
