#!/usr/bin/env python
"""bench.py — images/sec of the gan-reverser hot path step on MI355X:
   noise -> G forward (evaluate) -> R forward/backward (training) -> [RCCL all-reduce] -> L2+clamp+Adam
   (reference train_r.lua:138-170) at BASELINE.json configs[1]: 32x32 grayscale, noise=32, batch=256 per GPU.

python bench.py --gpus N --steps K --warmup W [--full]
  N > 1 without a torch.distributed.run environment: this process (which never touches a GPU) starts the N ranks itself
  (python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same arguments>) and exits with their code.
  N > 1 under torch.distributed.run (RANK / WORLD_SIZE set): one rank per GPU, gradients over RCCL.
A plain run times the headline only: the headline workload in the headline arithmetic (W untimed steps, then K timed ones), and rank 0
prints ONE compact JSON line on stdout with the contract's keys.
--full adds everything else the benchmark measures or checks: the other arithmetic modes, the cfg3 rider, the per-kernel tables and
roofline (with rocprofv3 traffic children and the bare MFMA loop), the cfg5 search and embedding pipeline, the GAN batch and the CPU
baselines.  Its line also carries `roofline`, `cpu_baseline`, `f32_row`, `cfg3` and `search_cfg5` summaries (< 4 KB); the full result
(per arithmetic mode tables, per-kernel tables, notes) goes to the --detail file.  The --no-* switches, --modes, --traffic and
--embed-* only shape a --full run.
--dump-outputs DIR writes what the last timed step of each timed mode computed as .npy files (same arguments = same inputs), so that two
builds can be compared output for output.  It writes the files of a --full run in a plain run too: every mode and workload is stepped
as --full steps it, and only the headline is reported.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(ROOT, "gan-reverser_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU x 256 FLOP/clk x 2.4 GHz
PEAK_BF16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense bf16 MFMA (the 5 PF marketing figure is 2:1 sparse)
BF16X6_PASSES = 6                  # bf16x6 mode: six bf16 MFMA products per fp32-accurate product
F16X3_PASSES = 3                   # f16x3 mode: three f16 MFMA products per fp32-accurate product
PEAK_HBM_GBS = 8000.0
MODES = ("f16x3", "bf16x6", "f32")
DTYPE = {"f32": "f32", "bf16x6": "f32 via bf16x6 (3-term bf16 split, 6 MFMA products, fp32 accumulate)",
         "f16x3": "f32 via f16x3 (2-term fp16 split of power-of-two-scaled operands, 3 MFMA products, fp32 accumulate)"}

WORKLOADS = {
    # BASELINE.json configs[1] / configs[2]
    "cfg2": dict(dims=(1, 32, 32), nd=32, batch=256, name="32x32 grayscale, noise=32, batch=256/GPU: G fwd + R fwd/bwd + Adam"),
    "cfg3": dict(dims=(3, 64, 64), nd=100, batch=512, name="64x64 RGB, noise=100, batch=512/GPU: G fwd + R fwd/bwd + Adam"),
}
ELEMENTWISE = ("post_forward", "post_backward", "bn_stats", "bias_grad", "gen_mask", "absmax_kernel")


def step_flops_per_image(dims, nd):
    """Algorithmic FLOPs (multiply-add = 2) of one image through the step: G fwd + 3 x R fwd.
    Also returns R's 3x3 convolutions alone (forward): the "R's 3x3 convs at bs256" figure of north_star is 3 x that x batch."""
    c, h, w = dims
    h4, w4 = h // 4, w // 4
    conv = lambda ci, co, hh, ww: 2.0 * 9 * ci * co * hh * ww
    g = 2.0 * nd * 512 * h4 * w4 + conv(512, 256, h // 2, w // 2) + conv(256, 128, h, w) + conv(128, c, h, w)
    r_conv = conv(c, 64, h, w) + 2 * conv(64, 64, h, w) + conv(64, 128, h // 2, w // 2) + 2 * conv(128, 128, h // 2, w // 2)
    r = r_conv + 2.0 * 128 * h4 * w4 * 512 + 2.0 * 512 * nd
    return g + 3 * r, g, r, r_conv


# ----------------------------------------------------------------------------------------------------------------------
# launch: `python bench.py --gpus N` starts its own ranks
def spawn_ranks(args):
    """Called before anything in this process has touched a GPU (no torch.cuda / HIP call has run): start N ranks as CHILD
    processes through torch.distributed.run and relay their output; never re-exec a process that has initialised the GPU."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


# ----------------------------------------------------------------------------------------------------------------------
# HBM traffic of the dominant kernel, measured in this run: two rocprofv3 --pmc children (FETCH_SIZE / WRITE_SIZE in separate
# passes, MI355X_MICROARCH.md section HBM), each a short run of this same script.  They are started BEFORE this process
# initialises the GPU.
def measure_traffic(args, workload):
    import csv, glob, shutil, tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    out, base = {}, tempfile.mkdtemp(prefix="ganrev_pmc_")
    child = [sys.executable, os.path.abspath(__file__), "--full", "--workload", workload, "--steps", "2", "--warmup", "1", "--conv-mode", args.conv_mode,
             "--modes", args.conv_mode, "--traffic", "off", "--no-cpu-baseline", "--no-search", "--no-gan", "--no-sustained", "--quiet-child"]
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(base, counter)
            cmd = ["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "--"] + child
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=240)
            files = glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None, f"rocprofv3 --pmc {counter} failed (rc {r.returncode}): {r.stderr.decode(errors='replace')[-200:]}"
            agg = {}
            for row in csv.DictReader(open(files[0])):
                if row["Counter_Name"] != counter:
                    continue
                k = row["Kernel_Name"].replace("void ", "").replace("gr::", "").split("(")[0]
                a = agg.setdefault(k, [0, 0.0]); a[0] += 1; a[1] += float(row["Counter_Value"])
            out[counter] = {k: v / n for k, (n, v) in agg.items()}
    except Exception as e:  # noqa: BLE001 - reported in the line, never silent
        return None, f"traffic measurement failed: {e}"
    finally:
        shutil.rmtree(base, ignore_errors=True)
    # KiB -> bytes; gfx950: FETCH_SIZE reports half the bytes of a wide streaming read -> doubled (the guide's correction)
    kernels = set(out["FETCH_SIZE"]) | set(out["WRITE_SIZE"])
    return {k: round(2 * 1024 * out["FETCH_SIZE"].get(k, 0.0) + 1024 * out["WRITE_SIZE"].get(k, 0.0)) for k in kernels}, \
        ("measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over 3 steps of this script; per launch, 2 x FETCH + WRITE "
         "(the factor 2 calibrated per load shape against known byte counts - profiles/r04_fetch_calibration.txt - and cross-checked per kernel against "
         "the request-size counters TCC_EA0_RDREQ_32B/64B/128B - profiles/r04_traffic_two_ways_*.txt: they agree within 1 % for every kernel of the step)")


# ----------------------------------------------------------------------------------------------------------------------
def cpu_baseline(dims, nd, ctx=None):
    """The oracle (CPU restatement of the Torch7 nn path, OpenMP) timed on this box's host cores at BASELINE.json configs[0]
    (32x32 grayscale, noise 32, batch 16 - train_r.lua's own CPU case) on a bounded sample: with the reference's default thread
    count (8, train_r.lua:21) and with the thread count that measured fastest on this box class; convolutions as im2col +
    blocked sgemm (the reported value) and as the parity oracle's direct loops (beside it)."""
    import numpy as np
    from ganrev import models, synth
    from oracle import oracle
    B = 16
    G = models.create_G(dims, nd); synth.init_params(G, 1)
    R = models.create_R(dims, nd); synth.init_params(R, 2)
    oG, oR = oracle.from_model(G, (nd, 1, 1)), oracle.from_model(R, dims)
    for m in R.leaves():
        if m.typename in ("nn.Dropout", "nn.SpatialDropout"):
            li = oR.layer_index[id(m)]
            oR.set_mask(li, synth.bernoulli_keep((oR.mask_size(li, B),), 7 + li, m.p))
    mm = np.zeros(oR.n_params, np.float32); vv = np.zeros_like(mm)
    noise = synth.normal((B, nd), 9)

    def run(threads, budget, impl):
        oracle.set_conv_impl(impl)
        threads = oracle.set_threads(threads)      # libgomp is already initialised (torch): the env var would be ignored
        oracle.train_r_step(oG, oR, noise, oracle.GoHyper(), mm, vv, 1)          # warm-up (page-in, thread pool)
        t0 = time.perf_counter(); n = 0
        while True:
            oracle.train_r_step(oG, oR, noise, oracle.GoHyper(), mm, vv, 2 + n)
            n += 1
            dt = time.perf_counter() - t0
            if dt > budget or n >= 60:
                break
        return threads, n, dt
    best = min(32, os.cpu_count() or 1)    # 16-32 OpenMP threads measured fastest for the oracle on the 2x64-core box (tools/cpu_baseline_sweep.py)
    try:
        # "mm": im2col + blocked sgemm per sample (oracle/oracle_mm.c) - the structure of THNN's SpatialConvolutionMM, which is what
        # SURVEY.md 8d specifies for this column; "direct": the parity oracle's 9-tap loop nests, kept beside it
        t8, n8, dt8 = run(8, 5.0, "mm")
        tb, nb, dtb = run(best, 5.0, "mm")
        d8, dn8, ddt8 = run(8, 4.0, "direct")
        db, dnb, ddtb = run(best, 4.0, "direct")
    finally:
        oracle.set_conv_impl("direct")
    # the headline value is the best of the thread counts actually run here, with its thread count; both runs ride beside it
    runs = {t8: (n8, dt8), tb: (nb, dtb)}
    tbest = max(runs, key=lambda t: runs[t][0] / runs[t][1])
    nbest, dtbest = runs[tbest]
    out = dict(value=round(B * nbest / dtbest, 2), unit="images/sec", cores=tbest, kind="port",
               sample=f"{nbest} steps of the same step at batch {B} = BASELINE configs[0] ({dtbest:.1f} s); oracle = C restatement of the Torch7 nn CPU "
                      "path with im2col + blocked-sgemm convolutions per sample (THNN SpatialConvolutionMM's structure; plain C, OpenMP over samples), "
                      "not Torch7 itself; value = the faster of the thread counts run (by_threads)",
               by_threads={str(t): round(B * n / dt, 2) for t, (n, dt) in sorted(runs.items())},
               reference_default_threads=dict(value=round(B * n8 / dt8, 2), cores=t8, sample=f"{n8} steps ({dt8:.1f} s), --threads 8 = train_r.lua:21"),
               direct_loop_convolutions=dict(value=round(B * max(dnb / ddtb, dn8 / ddt8), 2), cores=db if dnb / ddtb >= dn8 / ddt8 else d8,
                                             by_threads={str(d8): round(B * dn8 / ddt8, 2), str(db): round(B * dnb / ddtb, 2)},
                                             note="the parity oracle's own 9-tap loop nests (oracle_blas.c): what every parity test compares with; slower than the im2col path"))
    out["torch_cpu"] = torch_cpu_column(dims, nd, B)
    if ctx is not None:
        # second half of BASELINE.json's metric - "cosine top-50 exact-match vs ref" - at the size north_star names (10k x 32-d
        # embeddings, apply_r.lua:266-282): the HIP search against the oracle's, index lists compared element by element
        N, d, k, needles = 10000, 32, 50, [99, 199, 299, 399, 499]
        emb = synth.normal((N, d), 77)
        t0 = time.perf_counter(); ridx, rsc = oracle.cosine_topk(emb, needles, k); t_cpu = time.perf_counter() - t0
        ctx.cosine_topk(emb, needles, k)                                          # warm-up (workspace allocation)
        t0 = time.perf_counter(); idx, sc = ctx.cosine_topk(emb, needles, k); t_gpu = time.perf_counter() - t0
        out["search_top50"] = dict(n=N, d=d, k=k, needles=len(needles), exact_match=bool(np.array_equal(idx, ridx) and np.array_equal(sc, rsc)),
                                   gpu_ms_incl_h2d=round(t_gpu * 1e3, 3), cpu_ms=round(t_cpu * 1e3, 3))
    return out


def torch_cpu_column(dims, nd, B):
    """A second CPU column for orientation: the same G forward + R forward / backward + Adam step written
    with stock PyTorch CPU modules (oneDNN / im2col + sgemm convolutions - the structure Torch7's nn CPU path has, which the
    oracle's direct loops do not), timed at 8 threads and at the box's best of (16, 32).  Timing only: its numerics are not
    compared with anything, and it is not the oracle."""
    try:
        import torch
        import torch.nn as tnn
    except Exception as e:  # noqa: BLE001
        return dict(error=f"torch not importable: {e}")
    c, h, w = dims
    sh, sw = h // 4, w // 4
    G = tnn.Sequential(tnn.Linear(nd, 512 * sh * sw), tnn.BatchNorm1d(512 * sh * sw), tnn.ReLU(), tnn.Unflatten(1, (512, sh, sw)),
                       tnn.Upsample(scale_factor=2), tnn.Conv2d(512, 256, 3, padding=1), tnn.BatchNorm2d(256), tnn.ReLU(),
                       tnn.Upsample(scale_factor=2), tnn.Conv2d(256, 128, 3, padding=1), tnn.BatchNorm2d(128), tnn.ReLU(),
                       tnn.Conv2d(128, c, 3, padding=1), tnn.Sigmoid()).eval()
    layers = []
    for i, (ci, co) in enumerate([(c, 64), (64, 64), (64, 64), (64, 128), (128, 128), (128, 128)]):
        layers += [tnn.Conv2d(ci, co, 3, padding=1), tnn.BatchNorm2d(co), tnn.ELU()]
        if i == 2: layers += [tnn.MaxPool2d(2), tnn.Dropout()]
        elif i == 5: layers += [tnn.Dropout2d(0.25), tnn.MaxPool2d(2)]
        else: layers += [tnn.Dropout()]
    R = tnn.Sequential(*layers, tnn.Flatten(), tnn.Linear(128 * sh * sw, 512), tnn.BatchNorm1d(512), tnn.ELU(), tnn.Dropout(0.5), tnn.Linear(512, nd)).train()
    opt = torch.optim.Adam(R.parameters(), lr=1e-3)
    crit = tnn.MSELoss()
    res = {}
    prev = torch.get_num_threads()
    try:
        for threads in (8, 16, 32):
            if threads > (os.cpu_count() or 1):
                continue
            torch.set_num_threads(threads)

            def one():
                noise = torch.randn(B, nd)
                with torch.no_grad():
                    img = G(noise)
                opt.zero_grad()
                loss = crit(R(img), noise)
                loss.backward()
                for p_ in R.parameters():
                    p_.grad.add_(p_.detach(), alpha=1e-4).clamp_(-5, 5)      # train_r.lua:153-165 (L2 + clamp), cost only
                opt.step()
            one(); one()
            t0 = time.perf_counter(); n = 0
            while time.perf_counter() - t0 < 3.0 and n < 200:
                one(); n += 1
            res[str(threads)] = round(B * n / (time.perf_counter() - t0), 1)
    finally:
        torch.set_num_threads(prev)
    best = max(res, key=lambda k: res[k]) if res else None
    return dict(images_per_sec_by_threads=res, best_threads=int(best) if best else None, batch=B,
                note="stock PyTorch CPU modules (oneDNN convolutions), same layer lists and step; timing only, numerics unchecked")


def search_cfg5(ctx):
    """BASELINE.json configs[4]: 1M x 100-d embeddings (generated on the device), top-50 for the five needles of apply_r.lua:267,
    timed with HIP events on the library's stream, checked element by element against the oracle's search of the same corpus."""
    import numpy as np
    from oracle import oracle
    N, d, k = 1_000_000, 100, 50
    needles = np.array([100, 200, 300, 400, 500], dtype=np.int64)
    dev = ctx.malloc(4 * N * d)
    ctx.fill_normal(dev, N * d, 4242)
    ctx.cosine_topk(None, needles, k, emb_dev=dev, n=N, d=d)                  # warm-up
    reps = 5
    ctx.event_record(60000)
    for _ in range(reps):
        idx, sc = ctx.cosine_topk(None, needles, k, emb_dev=dev, n=N, d=d)
    ctx.event_record(60001)
    ms = ctx.event_elapsed_ms(60000, 60001) / reps
    # many needles at once (the batched path: fp16 MFMA candidates + exact re-score): 1024 needles, the five above among them
    many = np.concatenate([needles, (np.arange(1019, dtype=np.int64) * 977 + 13) % N])
    ctx.cosine_topk(None, many, k, emb_dev=dev, n=N, d=d)
    r0 = ctx.search_reruns()
    ctx.event_record(60002)
    for _ in range(3):
        midx, msc = ctx.cosine_topk(None, many, k, emb_dev=dev, n=N, d=d)
    ctx.event_record(60003)
    ms_many = ctx.event_elapsed_ms(60002, 60003) / 3
    batched = dict(needles=int(many.size), ms=round(ms_many, 4), mfma_tflops=round(2.0 * N * d * many.size / ms_many / 1e9, 1),
                   us_per_needle=round(ms_many * 1e3 / many.size, 3), reruns_unbatched=int(ctx.search_reruns() - r0),
                   first5_equal_single_path=bool(np.array_equal(midx[:5], idx) and np.array_equal(msc[:5], sc)),
                   note="approximate cosines on v_mfma_f32_32x32x16_f16 (error bound 2^-10 + 2^-13) pick candidates, the exact TH-order re-score decides: bit-identical results")
    emb = ctx.download(dev, (N, d)); ctx.free(dev)
    oracle.set_threads(min(32, os.cpu_count() or 1))
    t0 = time.perf_counter(); ridx, rsc = oracle.cosine_topk(emb, needles, k); t_cpu = time.perf_counter() - t0
    return dict(n=N, d=d, k=k, needles=int(needles.size), ms=round(ms, 4), hbm_gbs=round(N * d * 4 / ms / 1e6, 1),
                hbm_frac=round(N * d * 4 / (ms * 1e-3) / (PEAK_HBM_GBS * 1e9), 4),
                exact_match=bool(np.array_equal(idx, ridx) and np.array_equal(sc, rsc)), cpu_ms=round(t_cpu * 1e3, 1),
                batched_1024=batched,
                note="ms = one gr_cosine_topk_dev call: three launches (fp32 filter over a strided sample with the bound folded in, fp32 filter over "
                     "the table by LDS-DMA tiles, exact re-score + sort of the survivors), the 5 x 50 results written by the last kernel into pinned "
                     "host memory behind one completion word per needle, which the host polls")


def embed_cfg5(ctx, rows, with_oracle=True, train_steps=300):
    """BASELINE.json configs[4] as stated: "1M generated 64x64 faces -> 100-d embeddings, top-50".  apply_r.lua:145-153 resident on the
    GPU (gr_embed_dev): noise drawn on the device -> G forward (evaluate) -> R forward (evaluate) in chunks of 512, every chunk's
    recovered noise written straight into the [rows x 100] table, no host copies; then apply_r.lua:265-282's search on the table the
    pipeline produced, checked element by element against the oracle's search of the same table.  HIP events on the library's stream."""
    import numpy as np
    import ganrev._lib as L
    from ganrev import models, nn_utils, synth
    dims, nd, batch, k = WORKLOADS["cfg3"]["dims"], WORKLOADS["cfg3"]["nd"], 512, 50
    needles = np.array([100, 200, 300, 400, 500], dtype=np.int64)
    # apply_r.lua:62-104 loads a TRAINED G and the R that train_r.lua trained against it.  G: synthetic trained-looking weights and running
    # statistics.  R: models.create_R's initialisation, then `train_steps` iterations of train_r.lua:138-170 at batch 512 on the device
    # (the reference's own workflow, shortened: README "2000 batches") - an untrained R maps every face to nearly the same direction
    # (all cosines 0.9999.., ties broken by row index), which is no search corpus
    from ganrev.parallel import DeviceTrainer
    G = models.create_G(dims, nd); synth.init_params(G, 1)
    R = models.create_R(dims, nd, seed=1)
    G._ctx = R._ctx = ctx
    G.evaluate(); R.training()
    gnet, rnet = G.device_net((nd,)), R.device_net(dims)
    rnet.set_seed(99); rnet.adam_reset()
    trainer = DeviceTrainer(ctx, gnet, rnet, L.Hyper(), batch)
    loss0 = loss1 = None
    ctx.event_record(61990)
    for i in range(train_steps):
        trainer.new_noise(7_000_000 + i)
        l_ = trainer.step(want_loss=(i == 0 or i == train_steps - 1))
        loss0 = l_ if i == 0 else loss0
        loss1 = l_ if i == train_steps - 1 else loss1
    ctx.event_record(61991)
    train_ms = ctx.event_elapsed_ms(61990, 61991) if train_steps else 0.0
    trainer.close()
    G.evaluate(); R.evaluate()
    gnet, rnet = G.device_net((nd,)), R.device_net(dims)
    noise = nn_utils.createNoiseInputsDev(ctx, rows, nd, "normal", seed=4242)
    table = nn_utils.DeviceTensor(ctx, (rows, nd))
    L.embed_dev(gnet, [rnet], noise.ptr, min(rows, 2 * batch), batch, [table.ptr])          # warm-up: allocation, weight images
    ctx.synchronize()
    ctx.event_record(62000)
    L.embed_dev(gnet, [rnet], noise.ptr, rows, batch, [table.ptr])
    ctx.event_record(62001)
    ms = ctx.event_elapsed_ms(62000, 62001)
    fl_g, fl_r = step_flops_per_image(dims, nd)[1:3]
    # per-kernel table of four instrumented chunks
    nprof = 4
    ctx.set_timing(2)
    L.embed_dev(gnet, [rnet], noise.ptr, min(rows, nprof * batch), batch, [table.ptr])
    ctx.synchronize()
    kt, pseudo = split_pseudo_rows(ctx.kernel_times())
    ctx.set_timing(0)
    by = {}
    for kk in kt:
        a = by.setdefault(kk["kernel"], dict(kernel=kk["kernel"], launches=0, total_ms=0.0, flops=0.0, bytes=0.0))
        for f in ("launches", "total_ms", "flops", "bytes"):
            a[f] += kk[f]
    chunks = -(-min(rows, nprof * batch) // batch)
    mfma = [r for r in by.values() if r["kernel"].startswith("conv3x3_") and r["flops"] > 1e9 and "fewout" not in r["kernel"] and "fewin" not in r["kernel"]]
    dom = max(mfma, key=lambda r: r["total_ms"])
    avg_ms = dom["total_ms"] / dom["launches"]
    ach = dom["flops"] / dom["launches"] / (avg_ms * 1e-3) / 1e12
    peak, passes = kernel_ceiling_tflops(dom["kernel"])
    kernels = {}
    for r in sorted(by.values(), key=lambda r: -r["total_ms"])[:12]:
        tf, why = checked_tflops(r["kernel"], r["flops"], r["total_ms"])
        kernels[r["kernel"]] = dict(ms_per_chunk=round(r["total_ms"] / chunks, 4), launches_per_chunk=round(r["launches"] / chunks, 2), tflops=tf,
                                    gbs=round(r["bytes"] / max(r["total_ms"], 1e-9) / 1e6, 1) if r["bytes"] else None, **({"rejected": why} if why else {}))
    phase_ms = {}
    for kk in kt:
        phase_ms[kk.get("phase") or "other"] = phase_ms.get(kk.get("phase") or "other", 0.0) + kk["total_ms"] / chunks
    embed = dict(rows=rows, chunk=batch, images_per_sec=round(rows / ms * 1e3, 1), ms_total=round(ms, 2), ms_per_chunk=round(ms / (rows / batch), 4),
                 algorithmic_gflop_per_image=round((fl_g + fl_r) / 1e9, 3), tflops=round((fl_g + fl_r) * rows / ms / 1e9, 2),
                 frac_of_fp32_mfma_peak=round((fl_g + fl_r) * rows / ms / 1e9 / PEAK_FP32_MFMA_TFLOPS, 4),
                 kernel_ms_per_chunk={p_: round(v, 4) for p_, v in phase_ms.items()},
                 roofline=dict(bound="mfma", kernel=dom["kernel"], achieved=round(ach, 2), peak=round(peak, 1), unit="TFLOP/s", frac=round(ach / peak, 4),
                               avg_launch_ms=round(avg_ms, 4), launches_per_chunk=dom["launches"] / chunks,
                               algorithmic_gflop_per_launch=round(dom["flops"] / dom["launches"] / 1e9, 3)),
                 kernels=kernels, timer_failed_samples=pseudo.get("timer_failed_samples", dict(count=0))["count"], dtype=DTYPE[ctx.conv_mode()],
                 r_trained=dict(steps=train_steps, batch=batch, mse_first=loss0, mse_last=loss1, ms=round(train_ms, 1),
                                note="R trained here against the fixed G with gr_train_r_step before it is applied (train_r.lua -> apply_r.lua)"),
                 note="evaluate()-mode G + R forward (apply_r.lua:146,152), noise and the embedding table resident in HBM, no host copies inside the timed region")
    # the search on the table the pipeline wrote
    ctx.cosine_topk(None, needles, k, emb_dev=table.ptr, n=rows, d=nd)
    r0 = ctx.search_reruns()
    reps = 5
    ctx.event_record(62002)
    for _ in range(reps):
        idx, sc = ctx.cosine_topk(None, needles, k, emb_dev=table.ptr, n=rows, d=nd)
    ctx.event_record(62003)
    sms = ctx.event_elapsed_ms(62002, 62003) / reps
    search = dict(n=rows, d=nd, k=k, needles=int(needles.size), ms=round(sms, 4), hbm_gbs=round(rows * nd * 4 / sms / 1e6, 1),
                  reruns_unfiltered=int(ctx.search_reruns() - r0))
    if with_oracle:
        from oracle import oracle
        emb = table.numpy()
        oracle.set_threads(min(32, os.cpu_count() or 1))
        t0 = time.perf_counter(); ridx, rsc = oracle.cosine_topk(emb, needles, k); t_cpu = time.perf_counter() - t0
        search.update(exact_match=bool(np.array_equal(idx, ridx) and np.array_equal(sc, rsc)), cpu_ms=round(t_cpu * 1e3, 1),
                      distinct_rows=int(len(np.unique(emb[:: max(1, rows // 4096)].round(6), axis=0))),
                      top1_is_self=bool((idx[:, 0] == needles).all()))
    noise.free(); table.free()
    gnet.close(); rnet.close(); G._net = R._net = None
    return dict(embed=embed, search_on_pipeline_corpus=search)


def gan_step(ctx, with_cpu=True):
    """one batch of the GAN game (adversarial.lua:139-201: D on half real / half generated images, then G
    through D) with models.create_G / create_D2 at 32x32 gray, device-resident (ganrev.adversarial.DeviceGame), timed with HIP
    events; at train.lua's default batch (32) and at cfg2's batch (256).  Beside it the same batch on the CPU oracle, composed
    part by part.  Not the headline metric: a measured row for the component next to the path."""
    import numpy as np
    from ganrev import adversarial, models, synth
    dims, nd = (1, 32, 32), 100                                              # train.lua:26 noiseDim default
    rows = {}
    for B in (32, 256):
        G = models.create_G(dims, nd, seed=1); synth.init_params(G, 2)
        D = models.create_D2(dims, seed=2); synth.init_params(D, 3)
        env = adversarial.make_env(G, D, dims, batchSize=B, noiseDim=nd)
        game = adversarial.DeviceGame(env)
        real = synth.uniform((B // 2,) + dims, 40, 0, 1)
        for _ in range(3):
            game.batch(real)
        reps = 20
        ctx.event_record(61000)
        for _ in range(reps):
            game.batch(real)
        ctx.event_record(61001)
        ms = ctx.event_elapsed_ms(61000, 61001) / reps
        ld, lg = game.batch(real, want_loss=True)
        ctx.set_timing(2)
        game.batch(real)
        ctx.synchronize()
        kt = ctx.kernel_times()
        ctx.set_timing(0)
        kt, pseudo = split_pseudo_rows(kt)
        by = {}
        for k in kt:
            a = by.setdefault(k["kernel"], dict(kernel=k["kernel"], launches=0, total_ms=0.0, flops=0.0))
            a["launches"] += k["launches"]; a["total_ms"] += k["total_ms"]; a["flops"] += k["flops"]
        top = sorted(by.values(), key=lambda r: -r["total_ms"])[:8]
        rows[f"batch{B}"] = dict(ms_per_batch=round(ms, 4), generated_images_per_sec=round(B / ms * 1e3, 1), loss_d=round(ld, 5), loss_g=round(lg, 5),
                                 kernel_ms_sum=round(sum(r["total_ms"] for r in by.values()), 4), launches=int(sum(r["launches"] for r in by.values())),
                                 timer_failed_samples=pseudo.get("timer_failed_samples", dict(count=0))["count"],
                                 top_kernels=[dict(kernel=r["kernel"], launches=r["launches"], ms=round(r["total_ms"], 4),
                                                   **dict(zip(("tflops", "rejected"), checked_tflops(r["kernel"], r["flops"], r["total_ms"])))) for r in top])
        ctx.synchronize()
        game.close()
        for m in (G, D):
            for ch, _, _ in m._param_chunks():
                ch._net.close(); ch._net = None
    out = dict(config=dict(G="models.create_G3", D="models.create_D2", dims=list(dims), noiseDim=nd, optimizer="adam", D_L2=1e-4, D_clamp=1, G_clamp=5),
               **rows, note="device-resident batch (ganrev.adversarial.DeviceGame): the only host traffic is the upload of the real half batch")
    if with_cpu:
        from oracle import oracle
        B = 32
        oracle.set_threads(min(8, os.cpu_count() or 1))
        G = models.create_G(dims, nd, seed=1); synth.init_params(G, 2)
        D = models.create_D2(dims, seed=2); synth.init_params(D, 3)
        oG = oracle.from_model(G, (nd, 1, 1)); oG.set_training(True)
        trunk, concat, head = D.parts()
        shapes = [dims, (128, 16, 16), (128, 16, 16), (1024, 1, 1)]
        ons = [oracle.from_model(pt, sh) for pt, sh in zip([trunk, concat.modules[0], concat.modules[1], head], shapes)]
        for o, pt in zip(ons, [trunk, concat.modules[0], concat.modules[1], head]):
            o.set_training(True)
            for m in pt.leaves():
                if m.typename in ("nn.Dropout", "nn.SpatialDropout"):
                    li = o.layer_index[id(m)]
                    o.set_mask(li, synth.bernoulli_keep((o.mask_size(li, B),), 7 + li, m.p))

        def d_fwd_bwd(x, want_gin):
            t_out = ons[0].forward(x)
            l, r = ons[1].forward(t_out), ons[2].forward(t_out)
            cat = np.concatenate([l, r], axis=1)
            out_ = ons[3].forward(cat)
            _, df = oracle.bce(out_.reshape(-1), np.ones(B, np.float32))
            gcat = ons[3].backward(cat, df.reshape(out_.shape))
            gt = ons[1].backward(t_out, np.ascontiguousarray(gcat[:, :512])) + ons[2].backward(t_out, np.ascontiguousarray(gcat[:, 512:]))
            return ons[0].backward(x, gt, want_gin=want_gin)
        noise = synth.normal((B, nd), 3)
        t0 = time.perf_counter()
        x = np.concatenate([synth.uniform((B // 2,) + dims, 40, 0, 1), oG.forward(noise[:B // 2])])
        d_fwd_bwd(x, False)
        img = oG.forward(noise)
        gin = d_fwd_bwd(img, True)
        oG.backward(noise, gin)
        t_cpu = time.perf_counter() - t0
        out["cpu_baseline"] = dict(ms_per_batch=round(t_cpu * 1e3, 1), batch=B, cores=min(8, os.cpu_count() or 1), kind="port",
                                   sample="one batch of 32 (both network passes of the D step and of the G step; the Adam sweeps, ~10 ms, not included)")
    return out


# ----------------------------------------------------------------------------------------------------------------------
PSEUDO_ROWS = ("timer_failed_samples", "range_guard_fallback")      # counts the library reports beside the kernels (gr_kernel_times)


def kernel_ceiling_tflops(kname):
    """Ceiling for the ALGORITHMIC FLOP rate of a kernel, from its symbol: split kernels issue `passes` 16-bit MFMA products per
    fp32-accurate multiply-add (dense 16-bit peak / passes); everything else is priced at the fp32 rate of the pipe it runs on
    (fp32 MFMA = packed-fp32 VALU = 157.3 TFLOP/s).  The fused up-sampling kernel issues 4/9 of the reference's taps."""
    passes = 0
    if "_split_" in kname or "_pre_" in kname:
        targs = [t.strip() for t in kname[kname.index("<") + 1:kname.rindex(">")].split(",")]
        nterm = int(targs[2]) if ("split_wide" in kname or kname.startswith("conv3x3_split_kernel")) else int(targs[-1])
        passes = {3: BF16X6_PASSES, 2: F16X3_PASSES}.get(nterm, 0)
    elif "f16x3" in kname or "_p16_" in kname:        # operand-ready kernels (conv3x3_p16_*, conv3x3_wgrad_p16_*), gemm_f16x3_*: fp16 hi/lo, 3 products
        passes = F16X3_PASSES
    peak = PEAK_BF16_MFMA_TFLOPS / passes if passes else PEAK_FP32_MFMA_TFLOPS
    if "up2" in kname:
        peak *= 9.0 / 4.0
    return peak, passes


def split_pseudo_rows(kt):
    """-> (kernel rows, {pseudo row name: count}).  A timer that could not read a sample says so in a row of its own."""
    counts = {k["kernel"]: dict(count=int(k["launches"]), detail=k.get("phase", "")) for k in kt if k["kernel"] in PSEUDO_ROWS}
    return [k for k in kt if k["kernel"] not in PSEUDO_ROWS], counts


def checked_tflops(kname, flops, ms):
    """TFLOP/s of a row, or (None, reason) when it exceeds the kernel's ceiling: a rate above the ceiling means the timer did not
    time the work (a 1885 TFLOP/s row from unfinished events) - such a figure is never printed."""
    if not flops or ms <= 0:
        return None, None
    tf = flops / ms / 1e9
    peak, _ = kernel_ceiling_tflops(kname)
    if tf > peak * 1.02:
        return None, f"{tf:.1f} TFLOP/s exceeds the kernel's ceiling {peak:.1f}: timing rejected"
    return round(tf, 2), None


def kernel_report(kt, nprof, dims, nd, B, traffic=None):
    """Per-kernel table + the roofline object of the dominant MFMA kernel + R's convolutions / element-wise shares."""
    kt, pseudo = split_pseudo_rows(kt)
    by_name = {}
    for k in kt:
        a = by_name.setdefault(k["kernel"], dict(kernel=k["kernel"], launches=0, total_ms=0.0, flops=0.0, bytes=0.0))
        for f in ("launches", "total_ms", "flops", "bytes"):
            a[f] += k[f]
    rows = list(by_name.values())
    mfma = [k for k in rows if k["kernel"].startswith("conv3x3_") and k["flops"] > 1e9 and "reduce" not in k["kernel"]
            and "fewout" not in k["kernel"] and "fewin" not in k["kernel"] and "small" not in k["kernel"]]
    dom = max(mfma, key=lambda k: k["total_ms"])
    avg_ms = dom["total_ms"] / dom["launches"]
    achieved = dom["flops"] / dom["launches"] / (avg_ms * 1e-3) / 1e12
    # kernel names are the symbols rocprofv3 prints; the split kernels carry their number of terms as a template argument
    # (conv3x3_split_wide_kernel<TW, NI, NTERM, DB>, conv3x3_split_kernel<TW, MT, NTERM>, conv3x3_wgrad_split_*<..., NTERM>)
    kname = dom["kernel"]
    peak, passes = kernel_ceiling_tflops(kname)
    split = passes > 0
    up2 = "up2" in kname
    if achieved > peak * 1.02:
        raise SystemExit(f"bench.py: dominant kernel {kname} measures {achieved:.1f} TFLOP/s, above its ceiling {peak:.1f}: the timer is not timing the work")
    roofline = dict(bound="mfma", kernel=kname, achieved=round(achieved, 2), peak=round(peak, 1), unit="TFLOP/s",
                    frac=round(achieved / peak, 4), traffic=(traffic or {}).get(kname),
                    peak_note=(f"dense bf16/f16 MFMA 2500 TFLOP/s / {passes} products per fp32-accurate multiply-add "
                               f"({'f16x3' if passes == 3 else 'bf16x6'} split); issued MFMA rate = {passes} x achieved"
                               + (" x 4/9 (up-sampling taps pre-summed: four 2x2 convolutions)" if up2 else "")) if split else "fp32 MFMA v_mfma_f32_32x32x2_f32",
                    frac_of_fp32_mfma_peak=round(achieved / PEAK_FP32_MFMA_TFLOPS, 4),
                    avg_launch_ms=round(avg_ms, 4), launches_per_step=dom["launches"] / nprof,
                    algorithmic_gflop_per_launch=round(dom["flops"] / dom["launches"] / 1e9, 3))
    kernels = {}
    for k in sorted(rows, key=lambda k: -k["total_ms"]):
        tf, why = checked_tflops(k["kernel"], k["flops"], k["total_ms"])
        row = dict(ms_per_step=round(k["total_ms"] / nprof, 4), launches_per_step=round(k["launches"] / nprof, 2), tflops=tf,
                   gbs=round(k["bytes"] / max(k["total_ms"], 1e-9) / 1e6, 1) if k["bytes"] else None)
        if why:
            row = dict(launches_per_step=row["launches_per_step"], rejected=why)
        kernels[k["kernel"]] = row
    total_ms = sum(k["total_ms"] for k in rows) / nprof
    # north_star: ">= 40 % of MFMA roofline on R's 3x3 convs at bs256" - every conv3x3_* launch of R's forward and backward
    # (forward, data gradient, weight gradient incl. its slab reductions) against 3 x R's forward conv FLOPs x batch
    r_ms = sum(k["total_ms"] for k in kt if k["kernel"].startswith("conv3x3_") and k.get("phase") in ("R forward", "R backward")) / nprof
    r_gflop = 3 * step_flops_per_image(dims, nd)[3] * B / 1e9
    if r_ms > 0:
        r_convs = dict(ms_per_step=round(r_ms, 4), algorithmic_gflop=round(r_gflop, 1), tflops=round(r_gflop / r_ms, 2),
                       frac_of_fp32_mfma_peak=round(r_gflop / r_ms / PEAK_FP32_MFMA_TFLOPS, 4))
    else:      # kernels launched outside gr_train_r_step carry no phase tag (the shared-GPU test hook's decomposed step)
        r_convs = dict(ms_per_step=None, algorithmic_gflop=round(r_gflop, 1), tflops=None, frac_of_fp32_mfma_peak=None)
    ew_ms = sum(k["total_ms"] for k in rows if k["kernel"].startswith(ELEMENTWISE)) / nprof
    conv_ms = sum(k["total_ms"] for k in mfma) / nprof
    conv_fl = sum(k["flops"] for k in mfma) / nprof
    extra = dict(conv_kernels_tflops=round(conv_fl / max(conv_ms * 1e-3, 1e-12) / 1e12, 2), r_convs=r_convs,
                 elementwise=dict(ms_per_step=round(ew_ms, 4), share_of_kernel_time=round(ew_ms / max(total_ms, 1e-9), 4)),
                 kernel_ms_per_step=round(total_ms, 4), timer_failed_samples=pseudo.get("timer_failed_samples", dict(count=0))["count"])
    if "timer_failed_samples" in pseudo:
        extra["timer_error"] = pseudo["timer_failed_samples"]["detail"]
    return roofline, kernels, extra


def percentiles(ms):
    s = sorted(ms)
    q = lambda f: round(s[min(len(s) - 1, max(0, int(round(f * (len(s) - 1)))))], 4)
    return dict(p10=q(0.10), p50=q(0.50), p90=q(0.90), min=round(s[0], 4), max=round(s[-1], 4))


# ----------------------------------------------------------------------------------------------------------------------
# --dump-outputs DIR: what the timed path computed in its LAST timed step, as a caller of gr_train_r_step receives it - R's updated
# parameters, its clamped gradient, Adam's moments and BatchNorm running statistics, G's images and R's predictions of that step -
# as DIR/<workload>_<mode>_<name>.npy (float32).  An array above DUMP_MAX_ELEMS elements is stored as a fixed seeded sample of its
# flattened elements (the indices depend on the array's size only), which keeps a run's dump under DUMP_MAX_BYTES.
DUMP_MAX_ELEMS = 1 << 19
DUMP_MAX_BYTES = 64 * 10 ** 6
DUMP_SAMPLE_SEED = 20240601
_dump_bytes = [0]


def dump_sample(a):
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size <= DUMP_MAX_ELEMS:
        return a
    return a.reshape(-1)[np.sort(np.random.RandomState(DUMP_SAMPLE_SEED).permutation(a.size)[:DUMP_MAX_ELEMS])]


def dump_step_outputs(dirpath, prefix, ctx, gnet, rnet, B, dims, nd):
    import numpy as np
    m, v = rnet.adam_state()
    bn = [np.concatenate(rnet.get_bn_running(i)) for i in range(rnet.n_bn())]      # per BatchNorm: running_mean, then running_var
    arrays = dict(r_params=rnet.get_params(), r_grads=rnet.get_grads(), adam_m=m, adam_v=v,
                  r_bn_running=np.concatenate(bn) if bn else np.zeros(0, np.float32),
                  g_images=ctx.download(gnet.lib.gr_net_output_dev(gnet.h), (B,) + tuple(dims)),
                  r_output=ctx.download(rnet.lib.gr_net_output_dev(rnet.h), (B, nd)))
    os.makedirs(dirpath, exist_ok=True)
    for name, a in arrays.items():
        path = os.path.join(dirpath, f"{prefix}_{name}.npy")
        np.save(path, dump_sample(a))
        _dump_bytes[0] += os.path.getsize(path)
    if _dump_bytes[0] > DUMP_MAX_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs wrote {_dump_bytes[0]} bytes (limit {DUMP_MAX_BYTES})")


def every_mode(args):
    """Whether this run steps every mode and workload: --full times and reports them all; --dump-outputs runs the same steps without
    the reports, so that it writes the same files, with the same contents, as a --full run.  The sequence of steps matters: a mode's
    dropout noise continues the Philox counter of the steps before it (gr_net_set_seed restarts it once, at the net's creation)."""
    return args.full or bool(args.dump_outputs)


def run_workload(args, wl_key, modes, ctx, rank, world, shared_gpu, traffic, traffic_from, dist, torch):
    """One workload (cfg2 / cfg3) through the timed loop in every requested arithmetic mode.  Returns the line's fields for
    it (rank 0) or None."""
    import ganrev._lib as L
    from ganrev import models, synth
    from ganrev.parallel import DeviceTrainer, host_allreduce_grads
    wl = WORKLOADS[wl_key]
    dims, nd, B = wl["dims"], wl["nd"], wl["batch"]
    # random-init weights of the named architectures: G is a TRAINED net in the reference (train_r.lua:68 loads it) - synthetic
    # trained-looking weights and non-trivial running statistics; R is what train_r.lua:106 creates - models.create_R's own initialisation
    # (weight-init.lua heuristic, biases 0, BatchNorm gamma ~ U(0, 1), beta 0), unless --init synth asks for the parity tests' weights
    G = models.create_G(dims, nd); synth.init_params(G, 1)
    R = models.create_R(dims, nd, seed=args.seed)
    if args.init == "synth":
        synth.init_params(R, 2)
    G._ctx = R._ctx = ctx
    # compile the nets with one small forward each (allocation happens at the first full-size step, in warm-up)
    G.evaluate(); G.forward(synth.normal((2, nd), 1))
    R.training(); R.forward(synth.uniform((2,) + dims, 2, 0, 1)); R.push_params()
    gnet, rnet = G._net, R._net
    rnet.set_seed(1 + rank)                                              # independent dropout noise per rank
    rnet.adam_reset()
    theta0 = rnet.get_params()
    host_reduce = shared_gpu
    if world > 1 and not shared_gpu:
        rnet.broadcast_params(0)
    hyper = L.Hyper()
    GB = B * world
    trainer = DeviceTrainer(ctx, gnet, rnet, hyper, B, world, rank)

    def barrier():
        if world > 1:
            dist.barrier()
        ctx.synchronize()
        torch.cuda.synchronize()

    t_adam = 0

    def step(want_loss=False):
        nonlocal t_adam
        t_adam += 1
        trainer.new_noise((t_adam << 8) + rank)                          # createNoiseInputs (utils/nn_utils.lua:39-51), on device
        if host_reduce:  # test hook only (ranks share GPU 0: RCCL refuses duplicate devices): reduce through gloo
            return trainer.step_decomposed(host_allreduce_grads(dist))
        return trainer.step(want_loss=want_loss)

    tripped = {}                                                          # mode -> arithmetic the context ended on, when the range guard moved it

    def timed(mode):
        """W untimed steps, then EXACTLY K steps between barrier + device sync on both sides (max over ranks); one HIP event per
        step on the library's stream for the percentiles; then 3 instrumented steps for the per-kernel table."""
        nonlocal t_adam
        ctx.set_tuning("range_guard", 0); ctx.set_tuning("range_guard", 1)    # every mode starts with an untripped f16x3 range guard
        ctx.set_conv_mode(mode)
        falls0 = ctx.range_guard_stats()[1]
        rnet.set_params(theta0); rnet.adam_reset(); t_adam = 0            # every mode starts from the same state
        trainer.t = 0
        for _ in range(args.warmup):
            step()
        barrier()
        t0 = time.perf_counter()
        ctx.event_record(0)
        for i in range(args.steps):
            step()
            ctx.event_record(i + 1)
        barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        per_step = [ctx.event_elapsed_ms(i, i + 1) for i in range(args.steps)]
        if args.dump_outputs and rank == 0:
            dump_step_outputs(args.dump_outputs, f"{wl_key}_{mode}", ctx, gnet, rnet, B, dims, nd)
        loss = step(want_loss=True) if every_mode(args) else None         # the loss the --full tables report costs one more step
        # the timed steps must have run the arithmetic the line names: a tripped range guard moves the context to bf16x6 (csrc/net.hip)
        # (reported, not fatal: the row is then labelled with what ran)
        if ctx.conv_mode() != mode or ctx.range_guard_stats()[1] != falls0:
            tripped[mode] = ctx.conv_mode()
            if rank == 0:
                print(f"bench.py: the f16x3 range guard moved the context from {mode} to {ctx.conv_mode()} during the timed steps "
                      f"({ctx.range_guard_stats()[1] - falls0} fallbacks): the {mode} row of {wl_key} is labelled accordingly", file=sys.stderr)
        if not every_mode(args):
            return dt, per_step, loss, None
        # roofline leg: per-kernel HIP events (on the launch stream) over extra steps of the same workload.  Every rank runs
        # these steps (they contain the collective); only rank 0 instruments and reports.
        nprof = 3
        if rank == 0:
            ctx.set_timing(2)
        for _ in range(nprof):
            step()
        barrier()
        rep = None
        if rank == 0:
            kt = ctx.kernel_times()
            ctx.set_timing(0)
            rep = kernel_report(kt, nprof, dims, nd, B, traffic if mode == args.conv_mode else None) if args.full else None
        return dt, per_step, loss, rep

    results = {m: timed(m) for m in modes}
    ctx.set_conv_mode(args.conv_mode)
    out = None
    if rank == 0 and args.full and "f16x3" in results and not args.no_sustained:
        # What the chip's clock under MFMA load leaves of the spec ceiling, on THIS device in THIS run: the bare f16x3 inner loop
        # (LDS reads + three fp16 MFMA products per accumulate, two waves per SIMD, random data; csrc/mfmaloop.hip) right after the
        # timed steps.  `peak` and `frac` stay priced at the guide's dense peak; the sustained figure is reported beside them.
        roof = results["f16x3"][3][0]
        s32, s16 = ctx.bench_mfma_loop(0, 100), ctx.bench_mfma_loop(1, 100)
        up2 = 9.0 / 4.0 if "up2" in roof["kernel"] else 1.0
        roof["sustained"] = dict(bare_loop_tflops_32x32x16=round(s32 * up2, 1), bare_loop_tflops_16x16x32=round(s16 * up2, 1),
                                 frac_of_bare_loop=round(roof["achieved"] / (s32 * up2), 4),
                                 note="fp32-accurate TFLOP/s of a bare LDS-read + f16x3 MFMA loop (no staging, no epilogue) on this device after a warm-up under load, "
                                      "same units as `peak`: the chip does not hold 2.4 GHz under MFMA load on random data (MI355X_MICROARCH.md, DVFS give-back); "
                                      "32x32x16 is the instruction the convolution kernels issue, 16x16x32 the shape the chip clocks higher on")

    def moved(m):
        return f"{DTYPE[tripped[m]]} (the f16x3 range guard moved the context from {m} to {tripped[m]} during the timed steps)"
    if rank == 0:
        dt = results[args.conv_mode][0]
        out = dict(images_per_sec=round(GB * args.steps / dt, 1), ms_per_step=round(dt / args.steps * 1e3, 4),
                   workload=wl["name"], global_batch=GB, per_gpu_batch=B)
        if args.full:
            fl_img = step_flops_per_image(dims, nd)[0]
            _, per_step, loss, (roofline, kernels, extra) = results[args.conv_mode]
            if roofline.get("traffic") is not None or traffic_from:
                roofline["traffic_from"] = traffic_from
            mode_rows = {}
            for m, (mdt, mps, mloss, (mroof, _, mextra)) in results.items():
                mode_rows[m] = dict(images_per_sec=round(GB * args.steps / mdt, 1), ms_per_step=round(mdt / args.steps * 1e3, 4), dtype=DTYPE[m],
                                    step_ms_events=percentiles(mps), last_loss=mloss,
                                    roofline={k: mroof[k] for k in ("kernel", "achieved", "peak", "unit", "frac", "frac_of_fp32_mfma_peak", "avg_launch_ms", "sustained") if k in mroof},
                                    r_convs=mextra["r_convs"], elementwise=mextra["elementwise"])
                if m in tripped:
                    mode_rows[m]["dtype"] = moved(m)
                    mode_rows[m]["range_guard_tripped"] = True
            out.update(step_ms_events=percentiles(per_step),
                       step_tflops=round(fl_img * GB * args.steps / dt / 1e12 / world, 2),
                       step_frac_of_fp32_mfma_peak=round(fl_img * GB * args.steps / dt / 1e12 / world / PEAK_FP32_MFMA_TFLOPS, 4),
                       last_loss=loss, roofline=roofline, **extra, modes=mode_rows, kernels=kernels)
        out["host_reduce"] = host_reduce
        if args.conv_mode in tripped:
            out["range_guard_tripped"] = moved(args.conv_mode)
    trainer.close()
    gnet.close(); rnet.close()
    return out



# ----------------------------------------------------------------------------------------------------------------------
# The line the driver parses.  VERDICT round 4: a 23 KB line was cut by the driver's 8 KB stdout tail and left BENCH_r04.parsed null.
# Rank 0 therefore prints ONE compact stdout line (< 4 KB, strict JSON); everything else (mode tables, per-kernel tables, notes)
# goes to gpurun_out/bench_detail.json (--detail PATH); stderr carries only a one-line pointer to it.
HEADLINE_MAX_BYTES = 4096
DETAIL_FILE = os.path.join(ROOT, "gpurun_out", "bench_detail.json")
_SHORT_DTYPE = {"f16x3": "f32 via f16x3 split (3 fp16 MFMA products, fp32 accumulate)", "bf16x6": "f32 via bf16x6 split (6 bf16 MFMA products, fp32 accumulate)", "f32": "f32"}


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def headline(out, conv_mode="f16x3"):
    """The compact line: exactly the contract's keys, and for a --full result roofline + cpu_baseline + the strict-precision row, cfg3 and
    cfg5 summaries.  Pure function of the result dict (tests/test_host_logic.py feeds it canned ones)."""
    cfgkeys = ("workload", "global_batch", "per_gpu_batch", "parallelism", "bn")
    line = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline")}
    line["dtype"] = out["dtype"] if len(str(out.get("dtype", ""))) <= 100 else _SHORT_DTYPE.get(conv_mode, conv_mode)
    if out.get("range_guard_tripped") or "range guard" in str(out.get("dtype", "")):
        line["dtype"] = "f32 via bf16x6 split (range guard moved the context off f16x3 during the timed steps)"
    line["data"] = out.get("data", "synthetic")
    line["config"] = _pick(out.get("config", {}), cfgkeys)
    line["rccl_ranks"] = out.get("rccl_ranks", 1)
    if "roofline" not in out:          # a plain run: the headline measurement and nothing else
        return line
    roof = out.get("roofline") or {}
    line["roofline"] = _pick(roof, ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "launches_per_step", "algorithmic_gflop_per_launch"))
    if isinstance(roof.get("sustained"), dict):
        line["roofline"]["frac_of_bare_loop"] = roof["sustained"].get("frac_of_bare_loop")
    line["r_convs"] = _pick(out.get("r_convs") or {}, ("ms_per_step", "algorithmic_gflop", "tflops"))
    if line["r_convs"].get("tflops") and roof.get("peak"):
        line["r_convs"]["frac"] = round(line["r_convs"]["tflops"] / roof["peak"], 4)
    line["elementwise_ms"] = (out.get("elementwise") or {}).get("ms_per_step")
    cb = out.get("cpu_baseline")
    line["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "by_threads")) if cb else None
    if cb:
        line["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:120]
    f32 = out.get("f32_row")
    line["f32_row"] = _pick(f32, ("images_per_sec", "ms_per_step", "roofline_kernel", "roofline_frac", "r_convs_frac_of_fp32_mfma_peak")) if f32 else None
    c3 = out.get("cfg3")
    if c3:
        r3 = c3.get("roofline") or {}
        line["cfg3"] = dict(_pick(c3, ("images_per_sec", "ms_per_step")), roofline_kernel=r3.get("kernel"), roofline_frac=r3.get("frac"),
                            roofline_avg_launch_ms=r3.get("avg_launch_ms"), traffic=r3.get("traffic"),
                            r_convs_ms=(c3.get("r_convs") or {}).get("ms_per_step"), elementwise_ms=(c3.get("elementwise") or {}).get("ms_per_step"))
    s5 = out.get("search_cfg5")
    if s5:
        emb, bat = s5.get("embed") or {}, s5.get("batched_1024") or {}
        line["search_cfg5"] = dict(_pick(s5, ("n", "d", "k", "ms", "hbm_frac", "exact_match")), embed_images_per_sec=emb.get("images_per_sec"),
                                   embed_error=(str(emb["error"])[:120] if emb.get("error") else None), batched_ms=bat.get("ms"), batched_tflops=bat.get("mfma_tflops"),
                                   pipeline_corpus_exact_match=(s5.get("search_on_pipeline_corpus") or {}).get("exact_match"))
    g = out.get("gan_step")
    if g:
        line["gan_step"] = {"error": str(g["error"])[:120]} if "error" in g else {b: (g.get(b) or {}).get("ms_per_batch") for b in ("batch32", "batch256")}
    line["detail"] = "gpurun_out/bench_detail.json: mode tables, per-kernel tables, notes (a copy of the builder's run: profiles/r06_bench_default.json)"
    return line


def headline_text(out, conv_mode="f16x3"):
    line = headline(out, conv_mode)
    text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    for drop in ("gan_step", "elementwise_ms", "r_convs", "detail"):      # never reached with today's keys; a guard, not a plan
        if len(text) < HEADLINE_MAX_BYTES:
            break
        line.pop(drop, None)
        text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    if len(text) >= HEADLINE_MAX_BYTES:
        raise SystemExit(f"bench.py: headline is {len(text)} bytes (limit {HEADLINE_MAX_BYTES})")
    return text


def _finite(o):
    """NaN / Infinity are not JSON: they become null with the path recorded (the line must parse strictly)."""
    import math
    if isinstance(o, float) and not math.isfinite(o):
        return None
    if isinstance(o, dict):
        return {str(k): _finite(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_finite(v) for v in o]
    return o


import contextlib


@contextlib.contextmanager
def _stdout_to_stderr():
    """torch's gloo transport prints "[Gloo] Rank r is connected to ..." on the process's STDOUT (file descriptor 1, from C++) when a group forms: the contract is ONE
    JSON line on stdout, so fd 1 points at stderr while the group is being set up."""
    sys.stdout.flush()
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def emit(out, args):
    out = _finite(out)
    if args.full:                      # a plain run's line is its whole result: no detail file
        detail = json.dumps(out, allow_nan=False)
        try:
            os.makedirs(os.path.dirname(os.path.abspath(args.detail)), exist_ok=True)
            with open(args.detail, "w") as f:
                f.write(detail + "\n")
        except OSError as e:
            print(f"bench.py: could not write {args.detail}: {e}", file=sys.stderr)
        # (the 23 KB detail is NOT echoed to stderr: a driver that merges the streams and keeps a tail would be back to parsing around it - round 4's failure)
        print(f"bench.py: full result ({len(detail)} bytes: mode tables, per-kernel tables, notes) written to {args.detail}", file=sys.stderr)
        sys.stderr.flush()
    print(headline_text(out, args.conv_mode))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: the other arithmetic modes, the cfg3 rider, per-kernel tables and "
                         "roofline, the cfg5 search and embedding pipeline, the GAN batch, the CPU baselines, and the --detail file")
    ap.add_argument("--workload", default="both", choices=sorted(WORKLOADS) + ["both"],
                    help="both (default): cfg2 is the headline (BASELINE configs[1], the size north_star's bs256 target is quoted on) and, with --full, "
                         "cfg3 (configs[2] = the per-GPU shard of configs[3]) rides in the same line as the `cfg3` object")
    ap.add_argument("--init", default="reference", choices=["reference", "synth"], help="R's initial weights: models.create_R's (the reference's initialisation) or synth.init_params")
    ap.add_argument("--seed", type=int, default=1, help="seed of R's initialisation (train_r.lua:18 default 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-search", action="store_true", help="skip the cfg5 (1M x 100, top-50) search leg")
    ap.add_argument("--embed-rows", type=int, default=1_000_000, help="rows of the cfg5 corpus the device-resident G -> R pipeline produces (BASELINE configs[4]: 1M)")
    ap.add_argument("--embed-train-steps", type=int, default=300, help="train_r.lua iterations (batch 512) R gets before the cfg5 pipeline applies it")
    ap.add_argument("--sync-bn", action="store_true", help="synchronised BatchNorm over the ranks (gr_set_tuning sync_bn: per-channel batch sums all-reduced, "
                    "forward and backward); default: per-rank batch statistics")
    ap.add_argument("--no-sustained", action="store_true", help="skip the bare f16x3 MFMA loop (roofline.sustained): profiling runs, whose kernel statistics it would dominate")
    ap.add_argument("--no-gan", action="store_true", help="skip the GAN-game leg (SURVEY.md 8f rank 4: G + D2, one adversarial batch)")
    ap.add_argument("--conv-mode", default=os.environ.get("GR_CONV_MODE", "f16x3"), choices=list(MODES),
                    help="arithmetic of the headline line (all meet the 1e-4 parity bar; see DESIGN.md)")
    ap.add_argument("--modes", default=",".join(MODES), help="arithmetic modes a --full run times (the headline mode is always run)")
    ap.add_argument("--traffic", default="live", choices=["live", "file", "off"],
                    help="roofline.traffic: measured in this run by rocprofv3 --pmc children (N = 1), read from profiles/traffic.json, or omitted")
    ap.add_argument("--detail", default=DETAIL_FILE, help="file a --full run writes its FULL result (mode tables, per-kernel tables, notes) to; stdout carries the compact headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after each timed mode, write what its last timed step computed (R's parameters, gradient, Adam moments, BatchNorm running "
                         "statistics, G's images, R's predictions) as DIR/<workload>_<mode>_<name>.npy, float32; arrays above "
                         f"{DUMP_MAX_ELEMS} elements as a fixed seeded sample; at most {DUMP_MAX_BYTES // 10 ** 6} MB in all; the files of a --full run "
                         "in a plain run too (every mode and workload is stepped, only the headline reported)")
    ap.add_argument("--quiet-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))                       # this process has not touched a GPU
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    shared_gpu = bool(os.environ.get("GANREV_ALL_RANKS_ON_DEVICE0")) and world > 1   # test hook: the N>1 control flow on a 1-GPU box
    if shared_gpu:
        local_rank = 0
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a line for a different job size")

    if os.environ.get("GANREV_BENCH_DRY_RUN"):
        # launcher rehearsal for boxes without a GPU (tests/test_host_logic.py): the ranks rendezvous over gloo, rank 0 reports
        # who showed up, nothing touches a device
        import torch.distributed as dist
        seen = [(rank, local_rank)]
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            with _stdout_to_stderr():
                dist.init_process_group("gloo", rank=rank, world_size=world)
                seen = [None] * world
                dist.all_gather_object(seen, (rank, local_rank))
                dist.destroy_process_group()
        if rank == 0:
            wl = WORKLOADS["cfg2" if args.workload == "both" else args.workload]
            print(json.dumps({"dry_run": True, "n_gpus": world, "ranks": sorted(seen), "scaling": "weak",
                              "config": {"workload": wl["name"], "per_gpu_batch": wl["batch"], "global_batch": wl["batch"] * world,
                                         "parallelism": f"dp{world}"}}))
        return

    head = "cfg2" if args.workload == "both" else args.workload
    workloads = [head] + (["cfg3"] if args.workload == "both" and every_mode(args) else [])
    traffic_src = args.traffic if args.full else "off"     # roofline.traffic belongs to the --full tables
    traffic, traffic_from = {}, {}
    for w in workloads:
        t, tf = None, None
        if world == 1 and traffic_src == "live":
            t, tf = measure_traffic(args, w)              # children first: this process has not initialised the GPU yet
        if t is None and traffic_src != "off":
            tfile = os.path.join(ROOT, "profiles", "traffic.json")
            note = tf
            if os.path.exists(tfile):
                try:
                    t = json.load(open(tfile)).get(w)
                    tf = "profiles/traffic.json (committed rocprofv3 --pmc summary of an earlier run, NOT measured in this run)" + (f"; live: {note}" if note else "")
                except Exception:  # noqa: BLE001
                    t = None
        traffic[w], traffic_from[w] = t, tf

    import numpy as np  # noqa: F401
    import torch
    import torch.distributed as dist
    import ganrev._lib as L

    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        with _stdout_to_stderr():
            dist.init_process_group("gloo", rank=rank, world_size=world)     # control plane only; gradients go over RCCL
            dist.barrier()                                                   # (the transport connects lazily: its chatter belongs to this block too)
    os.environ["LOCAL_RANK"] = str(local_rank)
    ctx = L.default_context()          # THE context of this process: the side legs' modules (default_context()) launch on the stream the timers watch
    ctx.set_conv_mode(args.conv_mode)
    rccl_ranks = 1
    if world > 1 and not shared_gpu:
        uid = [ctx.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        ctx.comm_init(uid[0], world, rank)                                # RCCL over xGMI, inside libganrev.so; raises on failure
        rccl_ranks, rccl_rank = ctx.comm_ranks()
        if rccl_ranks != world or rccl_rank != rank:
            raise SystemExit(f"bench.py: RCCL communicator has {rccl_ranks} ranks (this is {rccl_rank}), expected {world} / {rank}")

    if args.sync_bn:
        ctx.set_tuning("sync_bn", 1)                                          # takes effect with a communicator (N > 1)
    modes = [args.conv_mode] + ([m for m in args.modes.split(",") if m in MODES and m != args.conv_mode] if every_mode(args) else [])
    res = {}
    for w in workloads:
        # the second workload of a --full run is timed in the headline arithmetic only (its other modes: --full --workload cfg3)
        res[w] = run_workload(args, w, modes if w == head else [args.conv_mode], ctx, rank, world, shared_gpu,
                              traffic[w], traffic_from[w], dist, torch)

    out = None
    if rank == 0:
        h = res[head]
        host_reduce = h.pop("host_reduce")
        out = {
            "metric": "images/sec G+R fwd/bwd", "value": h.pop("images_per_sec"), "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": h.pop("ms_per_step"),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": h.pop("range_guard_tripped", None) or DTYPE[args.conv_mode],
            "data": "synthetic",
            "config": {"workload": h.pop("workload"), "global_batch": h.pop("global_batch"), "per_gpu_batch": h.pop("per_gpu_batch"),
                       "parallelism": f"dp{world}" + ("" if world == 1 else (" (RCCL all-reduce of R's flat gradient)" if not host_reduce else
                                                      " (TEST HOOK: ranks share one GPU, gradients reduced through gloo on the host)")),
                       "bn": ("sync (per-channel batch sums all-reduced over the ranks, forward and backward: the global batch's statistics)"
                              if (args.sync_bn and world > 1 and not host_reduce) else "per-rank batch statistics"),
                       "init": ("G: synthetic trained-looking weights and running statistics (the reference loads a trained G); R: " +
                                (f"models.create_R's own initialisation, seed {args.seed} (weight-init.lua heuristic, BatchNorm gamma ~ U(0, 1))" if args.init == "reference"
                                 else "synth.init_params (the parity tests' weights)"))},
            "rccl_ranks": rccl_ranks,
            **h,
        }
        # the strict-precision reading of the line at a fixed key: exact fp32 on v_mfma_f32_32x32x2_f32 (no narrower than the reference's
        # fp32 operands), same workload, same steps / warmup, priced against the fp32 MFMA peak
        f32 = out.get("modes", {}).get("f32")
        if f32 is not None:
            out["f32_row"] = dict(images_per_sec=f32["images_per_sec"], ms_per_step=f32["ms_per_step"], dtype=f32["dtype"],
                                  roofline_kernel=f32["roofline"]["kernel"], roofline_frac=f32["roofline"]["frac"], roofline_peak=f32["roofline"]["peak"],
                                  r_convs_frac_of_fp32_mfma_peak=f32["r_convs"]["frac_of_fp32_mfma_peak"],
                                  note="the same workload in exact-fp32 arithmetic (modes.f32); the headline `value` runs fp32-accurate f16x3 (22-bit operand splits)")
        if "cfg3" in res and head != "cfg3" and args.full:
            c3 = res["cfg3"]; c3.pop("host_reduce")
            c3["note"] = ("BASELINE configs[2] (64x64 RGB, noise 100, batch 512 per GPU) = the per-GPU shard of configs[3] (global batch 4096 over 8 GPUs): "
                          "same run, same steps / warmup, headline arithmetic; at n_gpus = 8 this object IS configs[3]")
            out["cfg3"] = c3
        if args.full:                 # the side legs
            if world == 1 and not args.no_search:
                out["search_cfg5"] = search_cfg5(ctx)
                try:                      # configs[4] as stated: the corpus produced by the device-resident G -> R pipeline, then searched
                    out["search_cfg5"].update(embed_cfg5(ctx, args.embed_rows, with_oracle=not args.no_cpu_baseline, train_steps=args.embed_train_steps))
                except Exception as e:  # noqa: BLE001
                    out["search_cfg5"]["embed"] = {"error": f"{type(e).__name__}: {e}"}
            if world == 1 and not args.no_gan:
                try:                      # a side leg: its failure is reported in the line, it never takes the headline measurement down
                    out["gan_step"] = gan_step(ctx, with_cpu=not args.no_cpu_baseline)
                except Exception as e:  # noqa: BLE001
                    out["gan_step"] = {"error": f"{type(e).__name__}: {e}"}
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(WORKLOADS["cfg2"]["dims"], WORKLOADS["cfg2"]["nd"], ctx)
            else:
                out["cpu_baseline"] = None
    if world > 1:
        dist.barrier()
        if not shared_gpu:
            ctx.comm_destroy()
        dist.destroy_process_group()
    if out is not None and not args.quiet_child:
        emit(out, args)


if __name__ == "__main__":
    main()
