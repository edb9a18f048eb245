"""Times ops.detect_text_u8(local=128) -- the locally adaptive threshold, csrc/detect.hip k_detect_cell_otsu and
k_detect_hsmooth_local -- against ops.detect_text_u8() in the same process on the same photos: B = 8 of 2400 x 1600 and B = 48 of
640 x 480, the photos of tools/bench_detect_oriented.py.  Warm-up, then repeated timed calls of the two in turn (each ends with a
synchronous copy to the host); median, minimum and the quartiles of each, and the ratio of the medians.  Also timed, between events: the
two new launches alone (the cell-Otsu launch; the label entry point in local mode, whose first launch is the new one, beside the global
label entry point).  Writes one JSON object (default profiles/detect_local_bench.json).

    python tools/bench_detect_local.py [--out FILE] [--repeat N] [--local C]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_detect_oriented import SETS, photos, stats      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_local_bench.json"))
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--local", type=int, default=128)
    args = ap.parse_args()
    import torch
    from dpmn_amd import _abi, ops
    from dpmn_amd.utils import resize
    assert torch.cuda.is_available(), "bench_detect_local needs a GPU"
    dev = torch.device("cuda:0")
    sets, lib, C = [], _abi.lib, args.local
    for n, h, w in SETS:
        packed, meta = resize.pack_ragged(photos(n, h, w))
        packed = packed.to(dev)
        off, sizes = meta[:, 0], meta[:, 1:]
        one = lambda: ops.detect_text_u8(packed, off, sizes)
        cells = lambda: ops.detect_text_u8(packed, off, sizes, local=C)
        boxes, boxes_local = one(), cells()
        for _ in range(args.warmup):
            one()
            cells()
        torch.cuda.synchronize()
        t_one, t_cells = [], []
        for _ in range(args.repeat):      # in turn: drift of the clocks or of the host touches both alike
            for fn, ts in ((one, t_one), (cells, t_cells)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
        # the launches alone, between events, on the batch's own gradient maps
        kernels = {}
        hosts = {k: ops._detect_plan(packed, off, sizes, "bench", k) for k in (0, C)}
        state = {k: ops._detect_thresholds(packed, hosts[k], 24) for k in (0, C)}
        host, (d, d_items, d_tiles, g, hist, table) = hosts[C], state[C]
        items = host["items"]
        tmp, smooth = torch.empty_like(g), torch.empty_like(g)
        labels = torch.empty(g.numel(), dtype=torch.int32, device=dev)
        label = lambda k: (lambda: ops._detect_label(hosts[k], state[k][1], state[k][2], state[k][3], state[k][5], 12, 2, tmp, smooth, labels))
        otsu = lambda: _abi.check(lib.dpmn_detect_cell_otsu_i32(g.data_ptr(), host["map_px"], d_items, items.ctypes.data, items.shape[0], C, 24,
                                                                table.data_ptr(), host["n_cells"], _abi.stream()))
        for name, call in (("cell_otsu", otsu), ("label_local_3_launches", label(C)), ("label_global_3_launches", label(0))):
            ts = []
            for i in range(args.warmup + args.repeat):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ts.append(e0.elapsed_time(e1))
            kernels[name + "_ms"] = stats(ts)
        sets.append(dict(photos=n, shape=[h, w], cell_side=C, cells=host["n_cells"], boxes=int(sum(len(b) for b in boxes)),
                         boxes_local=int(sum(len(b) for b in boxes_local)), global_ms=stats(t_one), local_ms=stats(t_cells),
                         ratio_of_medians=round(statistics.median(t_cells) / statistics.median(t_one), 3), **kernels))
    res = dict(bench="detect_text_u8(local=%d) against detect_text_u8()" % C, sets=sets, repeat=args.repeat, warmup=args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
