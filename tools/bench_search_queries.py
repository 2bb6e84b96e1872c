#!/usr/bin/env python3
"""Search by example (gr_cosine_topk_queries_dev) against the row-index search (gr_cosine_topk_dev) at the shapes DESIGN.md quotes, tables
resident in HBM:
    small    1 M x 100, k 50, 5 needles
    batched  1 M x 100, k 50, 1024 needles
    filter   2^17 x 12288 (64 x 64 rgb pixels), k 50, 5 needles   (2^17 rows, not 1 M: 6.4 GB instead of 49 GB, twice for row (c))
Three rows per shape, the needles being the same vectors in all three (table rows i * 100):
    (a) the row-index search of the PARENT commit's library (tools/build_base.sh -> tools/probe/libganrev_base.so) - and of this build, so that
        the row-index search is seen not to have moved;
    (b) this build's search by example with those rows' vectors in a device array of their own;
    (c) what a caller had to do until now: the needles concatenated in front of the table (a second copy of the table: its one-off device
        copy is reported apart), the row-index search with k + Q, the needles' own hits filtered out on the host.  k + Q must stay <= 128 for
        the batched path (<= 1024 at all), so 1024 needles go in chunks of 78.
Every figure: the median [min, max] of 30 calls after a warm-up, timed by a pair of events on the context's stream around the call (event_ms)
and by the host clock around it (wall_ms: what the caller waits); per-kernel rows from gr_kernel_times of one more call.  The two libraries
run in child processes of their own (GANREV_LIB), alternating base / new / base / new on the same box; the samples of an arm are pooled.
   python tools/bench_search_queries.py [out.json]"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, ROUNDS = 30, 2
SHAPES = [("small", 1_000_000, 100, 50, 5), ("batched", 1_000_000, 100, 50, 1024), ("filter", 1 << 17, 12288, 50, 5)]
BASE = os.path.join(ROOT, "tools", "probe", "libganrev_base.so")
NEW = os.path.join(ROOT, "gan-reverser_amd", "ganrev", "libganrev.so")


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "n": len(ms)}


def child(arm):
    sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
    import numpy as np
    import ganrev._lib as L
    import ctypes as C
    have_queries = hasattr(C.CDLL(L.LIB_PATH), "gr_cosine_topk_queries_dev")
    if not have_queries:                                   # the parent commit's library: bind what it has
        for name in ("gr_cosine_topk_queries_dev", "gr_cosine_topk_queries_host"):
            L._SIGS.pop(name, None)
    ctx = L.default_context()
    out = {"arm": arm, "device": ctx.info(), "shapes": {}}

    def timed(fn):
        fn()                                               # the warm-up, discarded
        ev, wall = [], []
        for i in range(REPS):
            ctx.event_record(2 * i)
            t0 = time.perf_counter(); fn(); wall.append((time.perf_counter() - t0) * 1e3)
            ctx.event_record(2 * i + 1)
        ctx.synchronize()
        ev = [ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS)]
        r0 = ctx.search_reruns()
        ctx.set_timing(2); fn(); ctx.synchronize()
        kt = [{"kernel": k["kernel"], "launches": k["launches"], "total_ms": round(k.get("total_ms", 0.0), 4)} for k in ctx.kernel_times() if k.get("launches")]
        ctx.set_timing(0)
        return {"event_ms": ev, "wall_ms": wall, "kernels": kt, "reruns_in_timed_call": ctx.search_reruns() - r0}

    for name, N, d, k, Q in SHAPES:
        emb = ctx.malloc(4 * N * d)
        ctx.fill_normal(emb, N * d, 42)
        rows = (np.arange(Q, dtype=np.int64) * 100 + 100) % N
        res = {"N": N, "d": d, "k": k, "Q": Q}
        want = ctx.cosine_topk(None, rows, k, emb_dev=emb, n=N, d=d)
        res["rows"] = timed(lambda: ctx.cosine_topk(None, rows, k, emb_dev=emb, n=N, d=d))
        if have_queries:
            nd = ctx.malloc(4 * Q * d)
            for q, r in enumerate(rows.tolist()):          # the needles' vectors, gathered on the device
                ctx.copy2d(nd + 4 * d * q, d, emb + 4 * d * r, d, 1, d)
            got = ctx.cosine_topk_queries(None, None, k, emb_dev=emb, n=N, d=d, queries_dev=nd, q=Q)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
            res["queries"] = timed(lambda: ctx.cosine_topk_queries(None, None, k, emb_dev=emb, n=N, d=d, queries_dev=nd, q=Q))
            # (c): [needles of a chunk ; table] as one device table, rows 0 .. Qc - 1 searched with k + Qc, their own hits dropped on the host
            Qc = min(Q, 128 - k)
            aug = ctx.malloc(4 * (N + Qc) * d)
            t0 = time.perf_counter()
            ctx.copy2d(aug + 4 * d * Qc, d, emb, d, N, d); ctx.synchronize()
            res["concat_table_copy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)

            def concat_search():
                oi = np.empty((Q, k), np.int64); os_ = np.empty((Q, k), np.float32)
                for lo in range(0, Q, Qc):
                    n_ = min(Qc, Q - lo)
                    ctx.copy2d(aug + 4 * d * (Qc - n_), d, nd + 4 * d * lo, d, n_, d)      # this chunk's needles right in front of the table
                    base = aug + 4 * d * (Qc - n_)
                    idx, sc = ctx.cosine_topk(None, np.arange(n_, dtype=np.int64), k + n_, emb_dev=base, n=N + n_, d=d)
                    for q in range(n_):
                        keep = idx[q] >= n_
                        oi[lo + q] = idx[q][keep][:k] - n_; os_[lo + q] = sc[q][keep][:k]
                return oi, os_
            ci, cs = concat_search()
            assert np.array_equal(ci, want[0]) and np.array_equal(cs, want[1]), name + " (concatenation)"
            res["concat"] = dict(timed(concat_search), needles_per_call=Qc, calls=-(-Q // Qc))
            ctx.free(aug); ctx.free(nd)
        ctx.free(emb)
        out["shapes"][name] = res
    print("RESULT " + json.dumps(out), flush=True)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_search_queries.json")
    if not os.path.exists(BASE):
        sys.exit("tools/probe/libganrev_base.so is missing: tools/build_base.sh HEAD~ (the parent commit) builds it")
    runs = []
    for rnd in range(ROUNDS):
        for arm, lib in (("base", BASE), ("new", NEW)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm], env=dict(os.environ, GANREV_LIB=lib),
                               capture_output=True, text=True, timeout=420)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"arm {arm}, round {rnd}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            runs.append(json.loads(line[0][7:]))
    res = {"device": runs[0]["device"], "reps_per_round": REPS, "rounds": ROUNDS, "order": [r["arm"] for r in runs], "shapes": {}}
    for name, N, d, k, Q in SHAPES:
        row = {"N": N, "d": d, "k": k, "Q": Q}
        pool = lambda arm, what, clock: [v for r in runs if r["arm"] == arm and what in r["shapes"][name] for v in r["shapes"][name][what][clock]]
        last = lambda arm, what: [r for r in runs if r["arm"] == arm][-1]["shapes"][name][what]
        for label, arm, what in (("a_rows_parent", "base", "rows"), ("a_rows_this_build", "new", "rows"), ("b_queries", "new", "queries"), ("c_concat", "new", "concat")):
            row[label] = {"event": stats(pool(arm, what, "event_ms")), "wall": stats(pool(arm, what, "wall_ms")), "kernels": last(arm, what)["kernels"],
                          "reruns_in_timed_call": last(arm, what)["reruns_in_timed_call"]}
        row["c_concat"].update(needles_per_call=last("new", "concat")["needles_per_call"], calls=last("new", "concat")["calls"],
                               table_copy_ms_once=[r["shapes"][name]["concat_table_copy_ms"] for r in runs if r["arm"] == "new"])
        a, b = row["a_rows_parent"]["event"], row["b_queries"]["event"]
        row["b_median_inside_a_band"] = bool(a["ms_min"] <= b["ms_median"] <= a["ms_max"])
        row["b_minus_a_median_ms"] = round(b["ms_median"] - a["ms_median"], 4)
        res["shapes"][name] = row
        print(name, json.dumps({k_: (v["event"] if isinstance(v, dict) and "event" in v else v) for k_, v in row.items()}), flush=True)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
