#!/usr/bin/env python3
"""What pasting polygon regions back costs (main.py --demo_paste_polygons, csrc/paste_poly.hip) on one MI355X: prints ONE JSON line.

One enlarged photo of 2048 x 2048 and --regions 14-point arcs (k = 7) of about 400 x 64 enlarged pixels each, SR images of 64 x 400,
next to as many slanted quadrilaterals of the same area with the same SR images, in one run:
  mixed_polygons_us  -- dpmn_paste_mixed_u8 alone on the arcs (one launch), every table already on the device
  mixed_quads_us     -- dpmn_paste_mixed_u8 alone on the quadrilaterals: the same kernel on its perspective branch
  ops_*_ms           -- ops.paste_mixed_u8 / ops.paste_regions_u8 as the demo calls them (host plan, one upload, launch), synchronised
  numpy_polygons_ms  -- utils.paste_poly.paste_mixed_np on the host, the arcs
The kernels are timed with HIP events around --kernel-reps back-to-back calls after 10 warm-up calls, --reps times, the two
alternating: median, best and spread = (max - min) / median over the repetitions; the ops figures are medians of --reps runs after 2
warm-up runs, the numpy figure the median of 3.  *_px_inside counts the pixels a region claims; differing_bytes the bytes of the GPU's
photo that differ from the restatement's (expected: 0).  The measurement runs in a child process under a time limit of its own
(--timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHOTO, SCALE, SR = (1024, 1024), 2, (64, 400)


def make_scene(n_regions, feather, seed=9):
    """(enlarged photo, SR images, polygon regions, quadrilateral regions): per region a cell of a 4-column grid of the photo holds an arc
    of 7 + 7 points, chord about 200 and height 32 photo pixels, and a slanted quadrilateral of 200 x 32."""
    import numpy as np
    from dpmn_amd.utils import paste, paste_poly, quad
    rng = np.random.RandomState(seed)
    photo2 = rng.randint(0, 256, (SCALE * PHOTO[0], SCALE * PHOTO[1], 3)).astype(np.uint8)
    srs = [rng.randint(0, 256, SR + (3,)).astype(np.uint8) for _ in range(n_regions)]
    rows = -(-n_regions // 4)
    polys, quads = [], []
    for i in range(n_regions):
        cx, cy = 128 + 256 * (i % 4) + rng.uniform(-8, 8), (PHOTO[0] / rows) * (i // 4 + 0.5) + rng.uniform(-4, 4)
        r, down = rng.uniform(260, 340), rng.rand() < 0.5
        a = np.linspace(-100.0 / r, 100.0 / r, 7)
        s = -1.0 if down else 1.0      # the centre below the text (a rainbow) or above it (a smile)
        r_t, r_b = (r + 16, r - 16) if down else (r - 16, r + 16)
        y0 = cy - s * r
        t = np.stack([cx + r_t * np.sin(a), y0 + s * r_t * np.cos(a)], 1)
        b = np.stack([cx + r_b * np.sin(a), y0 + s * r_b * np.cos(a)], 1)
        polys.append((i, paste_poly.strip_table(np.concatenate([t, b[::-1]]), SCALE, SR[1], SR[0]), feather))
        th = rng.uniform(-0.12, 0.12)
        base = np.array([[-100, -16], [100, -16], [100, 16], [-100, 16]], np.float64)
        q = base @ np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).T + [cx, cy] + rng.uniform(-1.5, 1.5, (4, 2))
        quad.check_quad(q)
        quads.append((i, paste.paste_coeffs(q, SCALE, SR[1], SR[0]), feather))
    return photo2, srs, polys, quads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=32)
    ap.add_argument("--feather", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=300.0, help="time limit of the measuring child process, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        import subprocess
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print("bench_paste_poly: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import numpy as np
    import torch
    from dpmn_amd import ops
    from dpmn_amd._abi import check, lib, stream
    from dpmn_amd.utils import paste, paste_poly
    from dpmn_amd.utils.resize import pack_ragged
    if not torch.cuda.is_available():
        print("bench_paste_poly: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    photo2, srs, polys, quads = make_scene(a.regions, a.feather)
    H2, W2 = photo2.shape[:2]
    sr_packed, sr_meta = pack_ragged(srs)
    sr_packed = sr_packed.to(dev)
    fresh = lambda: torch.from_numpy(photo2).to(dev)
    work = fresh()

    def mixed_call(regions):
        host = ops._paste_mixed_plan(work, sr_packed, sr_meta, regions)
        table = host["table"]
        d = [torch.from_numpy(np.ascontiguousarray(host[k])).to(dev) for k in ("table", "strips", "tiles", "list")]
        S, n_tiles, n_list = host["strips"].shape[0], host["tiles"].shape[0], host["list"].size
        return host, lambda: check(lib.dpmn_paste_mixed_u8(work.data_ptr(), H2, W2, sr_packed.data_ptr(), sr_packed.numel(), d[0].data_ptr(),
                                                           table.ctypes.data, table.shape[0], d[1].data_ptr() if S else None, S,
                                                           d[2].data_ptr(), n_tiles, d[3].data_ptr(), n_list, stream()))

    # the launches alone (pasting again and again over the same photo: the same work each time), the two alternating
    calls = {"mixed_polygons": mixed_call(polys), "mixed_quads": mixed_call(quads)}
    times = {k: [] for k in calls}
    for _, call in calls.values():
        for _ in range(10):
            call()
    for _ in range(a.reps):
        for name, (_, call) in calls.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(a.kernel_reps):
                call()
            ev1.record()
            torch.cuda.synchronize()
            times[name].append(ev0.elapsed_time(ev1) * 1e3 / a.kernel_reps)
    res = {"enlarged_photo": [H2, W2], "regions": a.regions, "sr_size": list(SR), "feather": a.feather, "reps": a.reps,
           "kernel_reps": a.kernel_reps, "photo_tiles": -(-H2 // 8) * -(-W2 // 32)}
    for name, t in times.items():
        med = statistics.median(t)
        res[name + "_us"], res[name + "_best_us"], res[name + "_spread"] = round(med, 2), round(min(t), 2), round((max(t) - min(t)) / med, 3)
        res[name + "_tiles"], res[name + "_list_entries"] = int(calls[name][0]["tiles"].shape[0]), int(calls[name][0]["list"].size)
    res["strips"] = int(calls["mixed_polygons"][0]["strips"].shape[0])

    def timed(fn, sync, reps, warm):
        ms = []
        for _ in range(reps + warm):
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            if sync:
                torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms[warm:]), 3), out

    res["ops_mixed_polygons_ms"], _ = timed(lambda: ops.paste_mixed_u8(work, sr_packed, sr_meta, polys), True, a.reps, 2)
    res["ops_regions_quads_ms"], _ = timed(lambda: ops.paste_regions_u8(work, sr_packed, sr_meta, quads), True, a.reps, 2)
    res["numpy_polygons_ms"], expected = timed(lambda: paste_poly.paste_mixed_np(photo2, srs, polys), False, 3, 0)
    got = ops.paste_mixed_u8(fresh(), sr_packed, sr_meta, polys).cpu().numpy()
    res["differing_bytes"] = int((got != expected).sum())
    res["polygons_px_inside"] = int((expected != photo2).any(axis=2).sum())
    res["quads_px_inside"] = int((paste.paste_regions_np(photo2, srs, quads) != photo2).any(axis=2).sum())
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
