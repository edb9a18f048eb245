#!/usr/bin/env python3
"""What the rectification of text regions (main.py --demo_boxes, csrc/quad.hip) costs on one MI355X: prints ONE JSON line.

--photos photos of 720 x 1280 with --regions slanted regions of about 40 x 160 in all go through
  quad_crop_us      -- dpmn_quad_crop_u8 alone (one launch), the region table and the tiles already on the device
  quad_crop_host_ms -- ops.quad_crop_u8 as the loader calls it (host plan, one upload, launch, synchronise)
  pil_transform_ms  -- the same regions through Image.transform(PERSPECTIVE, BICUBIC) on the host, photos already decoded
The kernel is timed with HIP events around --kernel-reps back-to-back calls after 10 warm-up calls, --reps times: median, best and
spread = (max - min) / median over the repetitions; the host figures are medians of --reps runs after 2 warm-up runs.
differing_bytes counts the bytes of the GPU's regions that differ from PIL's (expected: 0).  The measurement runs in a child process
under a time limit of its own (--timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHOTO = (720, 1280)


def make_batch(n_photos, n_regions, seed=7):
    """(photos, regions): n_photos random (720, 1280, 3) uint8 photos and n_regions slanted, slightly perturbed quadrilaterals of about
    40 x 160 spread over them, as the (photo, h, w, coeffs) that ops.quad_crop_u8 takes."""
    import numpy as np
    from dpmn_amd.utils import quad
    rng = np.random.RandomState(seed)
    photos = [rng.randint(0, 256, PHOTO + (3,)).astype(np.uint8) for _ in range(n_photos)]
    regions = []
    while len(regions) < n_regions:
        ww, hh, th = rng.uniform(140, 180), rng.uniform(34, 46), rng.uniform(-0.35, 0.35)
        base = np.array([[-ww / 2, -hh / 2], [ww / 2, -hh / 2], [ww / 2, hh / 2], [-ww / 2, hh / 2]])
        rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        q = base @ rot.T + [rng.uniform(100, PHOTO[1] - 100), rng.uniform(60, PHOTO[0] - 60)] + rng.uniform(-3, 3, (4, 2))
        quad.check_quad(q)
        h, w = quad.quad_size(q)
        regions.append((len(regions) % n_photos, h, w, quad.quad_coeffs(q, w, h)))
    return photos, regions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photos", type=int, default=8)
    ap.add_argument("--regions", type=int, default=48)
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
            print("bench_quad: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import numpy as np
    import torch
    from PIL import Image
    from dpmn_amd import ops
    from dpmn_amd._abi import check, lib, stream
    from dpmn_amd.utils.resize import pack_ragged
    if not torch.cuda.is_available():
        print("bench_quad: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    photos, regions = make_batch(a.photos, a.regions)
    packed, meta = pack_ragged(photos)
    packed = packed.to(dev)
    host = ops._quad_crop_plan(packed, meta, regions)
    table, tiles = host["table"], host["tiles"]
    R, n_tiles = table.shape[0], tiles.shape[0]

    # the launch alone: everything it reads is uploaded once, the output is allocated once
    d_table, d_tiles = torch.from_numpy(table).to(dev), torch.from_numpy(tiles).to(dev)
    out = torch.zeros(host["out_bytes"], dtype=torch.uint8, device=dev)
    call = lambda: check(lib.dpmn_quad_crop_u8(packed.data_ptr(), packed.numel(), d_table.data_ptr(), table.ctypes.data, R, d_tiles.data_ptr(),
                                               n_tiles, out.data_ptr(), out.numel(), stream()))
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
    res = {"photos": a.photos, "regions": R, "tiles": n_tiles, "reps": a.reps, "kernel_reps": a.kernel_reps, "input_bytes": int(packed.numel()),
           "region_bytes": host["out_bytes"], "quad_crop_us": round(med, 2), "quad_crop_best_us": round(min(t), 2),
           "quad_crop_spread": round((max(t) - min(t)) / med, 3)}
    res["same_as_ops"] = bool(torch.equal(out, ops.quad_crop_u8(packed, meta, regions)[0]))

    host_ms = []
    for _ in range(a.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.quad_crop_u8(packed, meta, regions)
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    res["quad_crop_host_ms"] = round(statistics.median(host_ms[2:]), 3)

    pil_photos = [Image.fromarray(p) for p in photos]
    transform = lambda: [np.asarray(pil_photos[b].transform((w, h), Image.PERSPECTIVE, tuple(float(c) for c in co), Image.BICUBIC))
                         for b, h, w, co in regions]
    pil_ms = []
    for _ in range(a.reps + 2):
        t0 = time.perf_counter()
        ref = transform()
        pil_ms.append((time.perf_counter() - t0) * 1e3)
    res["pil_transform_ms"] = round(statistics.median(pil_ms[2:]), 3)
    flat = out.cpu().numpy()
    res["differing_bytes"] = int(sum((flat[off:off + h * w * 3].reshape(h, w, 3) != r).sum() for (off, h, w), r in zip(host["meta"].tolist(), ref)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
