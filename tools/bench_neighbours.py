"""Exact L2 nearest-neighbour search (gr_l2_nearest_dev, neighbours.hip) on the shapes of the issue that added it:
  a) n = 200 000, d = 1024,  q = 16, k = 1      b) n = 200 000, d = 12288, q = 16, k = 1 (9.8 GB)      c) n = 200 000, d = 1024, q = 64, k = 8
Per shape: ms per search from HIP events on the library's stream after warm-up (median, min, max over --reps), the fraction of 8 TB/s
(table bytes x passes over it / time), and - for reference only - torch on the same device doing the same search non-exactly
((x - q)^2).sum + topk, in row slices).  The per-kernel split comes from a separate rocprofv3 --kernel-trace --stats run of this script.

    python tools/bench_neighbours.py [--shapes a,b,c] [--reps 10] [--no-torch] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gan-reverser_amd"))

SHAPES = {"a": (200000, 1024, 16, 1), "b": (200000, 12288, 16, 1), "c": (200000, 1024, 64, 8)}
HBM = 8.0e12


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args(argv)
    import torch
    import ganrev._lib as L
    ctx = L.default_context()
    dev = torch.device("cuda:0")
    out = []
    for name in a.shapes.split(","):
        n, d, q, k = SHAPES[name]
        g = torch.Generator(device=dev); g.manual_seed(1)
        x = torch.rand((n, d), device=dev, dtype=torch.float32, generator=g)
        qs = torch.rand((q, d), device=dev, dtype=torch.float32, generator=g)
        torch.cuda.synchronize()
        qh = qs.cpu().numpy()
        idx = np.empty((q, k), np.int64); dist = np.empty((q, k), np.float64)

        def search():
            ctx.check(ctx.lib.gr_l2_nearest_dev(ctx.h, L._ptr(x.data_ptr()), n, d, L._ptr(qs.data_ptr()), q, k, L._ptr(idx), L._ptr(dist)), "gr_l2_nearest_dev")
        for _ in range(a.warmup):
            search()
        ms = []
        for _ in range(a.reps):
            ctx.event_record(0); search(); ctx.event_record(1)
            ms.append(ctx.event_elapsed_ms(0, 1))
        passes = -(-q // 16)
        med = float(np.median(ms))
        row = {"shape": name, "n": n, "d": d, "q": q, "k": k, "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
               "hbm_frac": 4.0 * n * d * passes / (med * 1e-3) / HBM, "passes": passes}
        if not a.no_torch:
            def tsearch():
                best_d, best_i = [], []
                for s in range(0, n, 16384):
                    part = x[s:s + 16384]
                    dd = ((part[None, :, :] - qs[:, None, :]) ** 2).sum(-1) if d <= 1024 else torch.stack([((part - qq) ** 2).sum(-1) for qq in qs])
                    v, i = torch.topk(dd, min(k, len(part)), dim=1, largest=False)
                    best_d.append(v); best_i.append(i + s)
                v, i = torch.topk(torch.cat(best_d, 1), k, dim=1, largest=False)
                return torch.gather(torch.cat(best_i, 1), 1, i)
            ti = tsearch(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tms = []
            for _ in range(max(3, a.reps // 3)):
                e0.record(); tsearch(); e1.record(); torch.cuda.synchronize(); tms.append(e0.elapsed_time(e1))
            row["torch_ms_median"] = float(np.median(tms))
            row["torch_top1_agrees"] = float((ti[:, 0].cpu().numpy() == idx[:, 0]).mean())
        print(json.dumps(row), flush=True)
        out.append(row)
        del x, qs
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
