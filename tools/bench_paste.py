#!/usr/bin/env python3
"""What pasting the SR regions back into their photo (main.py --demo_paste, csrc/paste_poly.hip) costs on one MI355X: prints ONE JSON line.

One photo of 1536 x 2048, enlarged by 2, and --regions slanted regions whose SR images are 32 x 128 go through
  paste_us         -- dpmn_paste_mixed_u8 alone (one launch), the table, the tiles and the list already on the device
  enlarge_paste_ms -- what TextSR.demo does per photo: ops.resize_ragged_u8 of the uploaded photo at its own target size, then
                      ops.paste_regions_u8 (host binning, one upload, launch), synchronised; the photo and the SR images are on the device
  pil_ms           -- the same work with PIL on the host: Image.resize(BICUBIC), then per region Image.transform(PERSPECTIVE, BICUBIC) of
                      the SR image and of an all-255 mask and Image.paste.  PIL is given the region's bounding box, not the whole photo
                      (the coefficients shifted by the box's corner), so its work, too, is proportional to the area pasted; its mask is the
                      hard one, whose cost does not depend on the feather.
The kernel is timed with HIP events around --kernel-reps back-to-back calls after 10 warm-up calls, --reps times: median, best and
spread = (max - min) / median over the repetitions; the other figures are medians of --reps runs after 2 warm-up runs.
differing_bytes counts the bytes of the GPU's photo that differ from utils.paste.paste_regions_np on PIL's enlargement (expected: 0).
The measurement runs in a child process under a time limit of its own (--timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHOTO, SCALE, SR = (1536, 2048), 2, (32, 128)


def make_scene(n_regions, feather, seed=9):
    """(photo, SR images, quads, regions): a random photo, n_regions random 32 x 128 SR images and as many slanted, slightly perturbed
    quadrilaterals of about 16 x 64 photo pixels, as the (SR index, coeffs, feather) that ops.paste_regions_u8 takes."""
    import numpy as np
    from dpmn_amd.utils import paste, quad
    rng = np.random.RandomState(seed)
    photo = rng.randint(0, 256, PHOTO + (3,)).astype(np.uint8)
    srs = [rng.randint(0, 256, SR + (3,)).astype(np.uint8) for _ in range(n_regions)]
    quads = []
    while len(quads) < n_regions:
        ww, hh, th = rng.uniform(56, 72), rng.uniform(14, 18), rng.uniform(-0.35, 0.35)
        base = np.array([[-ww / 2, -hh / 2], [ww / 2, -hh / 2], [ww / 2, hh / 2], [-ww / 2, hh / 2]])
        rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        q = base @ rot.T + [rng.uniform(60, PHOTO[1] - 60), rng.uniform(40, PHOTO[0] - 40)] + rng.uniform(-1.5, 1.5, (4, 2))
        quad.check_quad(q)
        quads.append(q)
    regions = [(k, paste.paste_coeffs(q, SCALE, SR[1], SR[0]), feather) for k, q in enumerate(quads)]
    return photo, srs, quads, regions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=50)
    ap.add_argument("--feather", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the measuring child process, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        import subprocess
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print("bench_paste: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import numpy as np
    import torch
    from PIL import Image
    from dpmn_amd import ops
    from dpmn_amd._abi import check, lib, stream
    from dpmn_amd.utils import paste
    from dpmn_amd.utils.resize import pack_ragged
    if not torch.cuda.is_available():
        print("bench_paste: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    photo, srs, quads, regions = make_scene(a.regions, a.feather)
    H2, W2 = SCALE * PHOTO[0], SCALE * PHOTO[1]
    packed, meta = pack_ragged([photo])
    packed = packed.to(dev)
    sr_packed, sr_meta = pack_ragged(srs)
    sr_packed = sr_packed.to(dev)
    enlarge = lambda: ops.resize_ragged_u8(packed, meta, H2, W2)[0]

    # the launch alone: everything it reads is uploaded once (pasting again and again over the same photo: the same work each time)
    photo2 = enlarge()
    host = ops._paste_mixed_plan(photo2, sr_packed, sr_meta, regions, what="paste_regions_u8", polygons=False)
    table, tiles, lst = host["table"], host["tiles"], host["list"]
    R, n_tiles, n_list = table.shape[0], tiles.shape[0], lst.size
    d_table, d_tiles, d_list = torch.from_numpy(table).to(dev), torch.from_numpy(tiles).to(dev), torch.from_numpy(lst).to(dev)
    call = lambda: check(lib.dpmn_paste_mixed_u8(photo2.data_ptr(), H2, W2, sr_packed.data_ptr(), sr_packed.numel(), d_table.data_ptr(),
                                                 table.ctypes.data, R, None, 0, d_tiles.data_ptr(), n_tiles, d_list.data_ptr(), n_list, stream()))
    for _ in range(10):
        call()
    t = []
    for _ in range(a.reps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(a.kernel_reps):
            call()
        ev1.record()
        torch.cuda.synchronize()
        t.append(ev0.elapsed_time(ev1) * 1e3 / a.kernel_reps)
    med = statistics.median(t)
    res = {"photo": list(PHOTO), "scale": SCALE, "regions": R, "feather": a.feather, "tiles": n_tiles, "photo_tiles": -(-H2 // 8) * -(-W2 // 32),
           "list_entries": n_list, "reps": a.reps, "kernel_reps": a.kernel_reps, "enlarged_bytes": H2 * W2 * 3, "paste_us": round(med, 2),
           "paste_best_us": round(min(t), 2), "paste_spread": round((max(t) - min(t)) / med, 3)}

    def timed(fn, sync):
        ms = []
        for _ in range(a.reps + 2):
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            if sync:
                torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms[2:]), 3), out

    res["enlarge_ms"], _ = timed(enlarge, True)
    res["enlarge_paste_ms"], got = timed(lambda: ops.paste_regions_u8(enlarge(), sr_packed, sr_meta, regions), True)

    pil_photo, pil_srs, white = Image.fromarray(photo), [Image.fromarray(s) for s in srs], Image.new("L", (SR[1], SR[0]), 255)

    def pil():
        im = pil_photo.resize((W2, H2), Image.BICUBIC)
        for k, c, _ in regions:
            x0, y0, x1, y1 = paste.region_box(c, SR[1], SR[0], H2, W2)
            # (X, Y) = (x + x0, y + y0): the constant terms take the shift
            cb = (c[0], c[1], c[0] * x0 + c[1] * y0 + c[2], c[3], c[4], c[3] * x0 + c[4] * y0 + c[5], c[6], c[7])
            den = c[6] * x0 + c[7] * y0 + 1
            cb = tuple(float(v / den) for v in cb)
            size = (x1 - x0, y1 - y0)
            im.paste(pil_srs[k].transform(size, Image.PERSPECTIVE, cb, Image.BICUBIC), (x0, y0),
                     mask=white.transform(size, Image.PERSPECTIVE, cb, Image.BICUBIC))
        return im

    res["pil_ms"], _ = timed(pil, False)
    res["pil_resize_ms"], enlarged = timed(lambda: np.asarray(pil_photo.resize((W2, H2), Image.BICUBIC)), False)
    expected = paste.paste_regions_np(enlarged, srs, regions)
    res["differing_bytes"] = int((got.cpu().numpy() != expected).sum())
    res["pasted_bytes"] = int((expected != enlarged).sum())
    res["host_cpus"] = len(os.sched_getaffinity(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
