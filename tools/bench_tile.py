#!/usr/bin/env python3
"""What the two device steps of the tiled demo path (main.py --demo_tile, csrc/tile.hip) cost on one MI355X: prints ONE JSON line.

A batch of --batch text lines of mixed sizes (word crops of one window up to 7 x 500 signs of 24) goes through
  resize_windows_us -- dpmn_resize_windows_u8 alone (its three launches), items, windows and tables already on the device
  stitch_us         -- dpmn_stitch_windows_u8 alone (one launch) on the T SR windows of the same plan
each timed with HIP events around --kernel-reps back-to-back calls after 10 warm-up calls, --reps times: median, best and
spread = (max - min) / median over the repetitions.  resize_windows_host_ms is ops.resize_windows_u8 as the loader calls it (host
plan, one upload, launches, synchronise).  The measurement runs in a child process under a time limit of its own (--timeout seconds);
the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(16, 64), (33, 70), (9, 40), (20, 300), (7, 500), (24, 180), (31, 420), (12, 260)]


def make_batch(n, seed=7):
    """n (h, w, 3) uint8 images, the eight shapes in turn."""
    import numpy as np
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, SHAPES[j % len(SHAPES)] + (3,)).astype(np.uint8) for j in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
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
            print("bench_tile: the measurement did not finish in %.0f s" % a.timeout, file=sys.stderr)
            return 124
    import torch
    from dpmn_amd import ops
    from dpmn_amd.utils.resize import pack_ragged
    if not torch.cuda.is_available():
        print("bench_tile: no GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    lr_h, lr_w, scale = 16, 64, 2
    packed, meta = pack_ragged(make_batch(a.batch))
    packed = packed.to(dev)
    plan, host = ops._resize_windows_plan(packed, meta, lr_h, lr_w)
    T = len(plan)
    sr = torch.rand(T, 3, scale * lr_h, scale * lr_w, device=dev)

    def events(call):
        for _ in range(10):
            call()
        out = []
        for _ in range(a.reps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(a.kernel_reps):
                call()
            ev1.record()
            torch.cuda.synchronize()
            out.append(ev0.elapsed_time(ev1) * 1e3 / a.kernel_reps)
        return out

    # the launches alone: everything they read is uploaded once, the outputs are allocated once
    import numpy as np
    from dpmn_amd._abi import check, lib, stream
    items, windows, tables = host["items"], host["windows"], host["tables"]
    B = items.shape[0]
    d_items, d_win, d_tab = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (items, windows, tables))
    ws = torch.empty(lib.dpmn_resize_windows_workspace_bytes(host["sum_h_w_line"], host["sum_w_line"], lr_h), dtype=torch.uint8, device=dev)
    out_w = torch.empty(T, lr_h, lr_w, 3, dtype=torch.uint8, device=dev)
    resize_call = lambda: check(lib.dpmn_resize_windows_u8(packed.data_ptr(), packed.numel(), d_items.data_ptr(), B, d_tab.data_ptr(), tables.size,
                                                           d_win.data_ptr(), T, host["max_mid_bytes"], host["max_w_line"], out_w.data_ptr(), lr_h,
                                                           lr_w, ws.data_ptr(), ws.numel(), stream()))
    from dpmn_amd.utils.tile import plan_lines
    lines = plan_lines(plan, lr_w)
    sizes = [scale * lr_h * scale * l[2] * 3 for l in lines]
    offs = np.concatenate(([0], np.cumsum(sizes[:-1])))
    d_lines = torch.from_numpy(np.array([(o, l[2], l[0], l[1]) for o, l in zip(offs, lines)], np.int64)).to(dev)
    out_s = torch.zeros(int(sum(sizes)), dtype=torch.uint8, device=dev)
    stitch_call = lambda: check(lib.dpmn_stitch_windows_u8(sr.data_ptr(), sr.stride(0), sr.stride(1), T, scale * lr_h, scale * lr_w, scale,
                                                           d_lines.data_ptr(), B, d_win.data_ptr(), max(l[2] for l in lines), out_s.data_ptr(),
                                                           out_s.numel(), stream()))
    res = {"batch": a.batch, "windows": T, "reps": a.reps, "kernel_reps": a.kernel_reps, "input_bytes": int(packed.numel()),
           "table_bytes": int(tables.size * 4), "line_bytes": int(sum(sizes))}
    for tag, call in (("resize_windows", resize_call), ("stitch", stitch_call)):
        t = events(call)
        med = statistics.median(t)
        res[tag + "_us"], res[tag + "_best_us"], res[tag + "_spread"] = round(med, 2), round(min(t), 2), round((max(t) - min(t)) / med, 3)
    same = torch.equal(out_w, ops.resize_windows_u8(packed, meta, lr_h, lr_w)[0]) and torch.equal(out_s, ops.stitch_windows_u8(sr, plan, scale)[0])
    res["same_as_ops"] = bool(same)
    host_ms = []
    for _ in range(a.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.resize_windows_u8(packed, meta, lr_h, lr_w)
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    res["resize_windows_host_ms"] = round(statistics.median(host_ms[2:]), 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
