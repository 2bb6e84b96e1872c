"""python -m ganrev.compare: which pair reconstructs an image better - the GAN's (G, R) or the VAE's (decoder, encoder mean)?

The reference's README puts "Compare to Autoencoders, especially VAEs" first under further research; ganrev.train_vae writes the VAE as an ordinary
G / R pair, and this script runs both pairs through the same images and scores x against G(R(x)) with SSIM, MSE and PSNR (ganrev.quality).  MSE alone
would be the wrong judge: a model trained on MSE regresses to the mean and wins a pixel-wise comparison for exactly that.

Two experiments per pair (A = --G / --R, B = --vaeG / --vaeR):
  own    x = G(z), z ~ N(0, 1) drawn on the device; x^ = G(R(x)): the fix-faces loop of the README, every pair on its own samples
  real   x = the first --nbImages files of --dataset, as apply_r --real loads them (without --dataset: ganrev.synth's stand-in images); x^ = G(R(x))

Written under --out: compare_{own,real}_{a,b}_{ssim,mse,psnr}.npy and summary.json - mean / median / 5 % / 95 % of every score, the device's own
mean SSIM, and on the real images the share of images on which A's SSIM exceeds B's and the share on which A's MSE is below B's, so that a reader
sees where the two metrics disagree.  --render adds compare_real.png: rows of (image, A's reconstruction, B's reconstruction) for the 16 images with
the largest SSIM(A) - SSIM(B), then the 16 with the smallest.  The image tables never visit the host.

    python -m ganrev.train_vae --save logs ... && python -m ganrev.compare --G logs/adversarial.net --R logs/r_3x32x32_nd32_normal.net
"""
import numpy as np

from . import _lib as L
from . import quality, scripts
from .nn_utils import DeviceScope, DeviceTensor, createNoiseInputsDev, forwardBatchedDev

NB_EXTREMES = 16


def parse(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="compare the reconstructions of a GAN pair (G, R) and a VAE pair on the same images")
    p.add_argument("--G", default="logs/adversarial.net", help="pair A's generator (apply_r's default)")
    p.add_argument("--R", default="logs/r_3x32x32_nd32_normal.net", help="pair A's reverser")
    p.add_argument("--vaeG", default="logs/vae_3x32x32_nd100.net", help="pair B's generator: the decoder train_vae saved")
    p.add_argument("--vaeR", default="logs/vae_r_3x32x32_nd100.net", help="pair B's reverser: the encoder's mean half train_vae saved")
    p.add_argument("--synthetic", default="", help="CxHxWxND, e.g. 1x32x32x32: random-initialised pairs instead of checkpoints")
    p.add_argument("--nbImages", type=int, default=1000)
    p.add_argument("--batchSize", type=int, default=512)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--out", default="compare_results", metavar="DIR")
    p.add_argument("--render", action="store_true", help="also write compare_real.png (ganrev.render)")
    p.add_argument("--win", type=int, default=quality.WIN, help="side of the SSIM window (odd, 3 .. 11)")
    p.add_argument("--sigma", type=float, default=quality.SIGMA, help="sigma of the Gaussian SSIM window (<= 0: uniform)")
    p.add_argument("--conv-mode", default="f16x3", choices=["f32", "bf16x6", "f16x3"])
    p.add_argument("--quiet", action="store_true")
    scripts.add_dataset_options(p)
    OPT = p.parse_args(argv)
    if OPT.nbImages < 1 or OPT.batchSize < 1:
        p.error("--nbImages and --batchSize: at least 1")
    if OPT.render and OPT.nbImages < 2 * NB_EXTREMES:
        p.error(f"--render shows the {NB_EXTREMES} best and the {NB_EXTREMES} worst images: --nbImages at least {2 * NB_EXTREMES}")
    if OPT.win < 3 or OPT.win > L.SSIM_MAX_WIN or OPT.win % 2 == 0:
        p.error(f"--win: an odd window of 3 .. {L.SSIM_MAX_WIN}")
    if OPT.synthetic:
        parts = OPT.synthetic.split("x")
        if len(parts) != 4 or not all(v.isdigit() and int(v) > 0 for v in parts):
            p.error("--synthetic: CxHxWxND")
        _, h, w, _ = (int(v) for v in parts)
        if min(h, w) < OPT.win or max(h, w) > L.SSIM_MAX_HW:
            p.error(f"--synthetic: SSIM scores images of {OPT.win} .. {L.SSIM_MAX_HW} pixels a side")
    return OPT


def a_wins_share(a, b):
    """the share of rows on which a's score is strictly above b's"""
    return float((np.asarray(a) > np.asarray(b)).mean())


def extreme_rows(ssim_a, ssim_b, k=NB_EXTREMES):
    """(the k rows with the largest SSIM(A) - SSIM(B), largest first; the k with the smallest, smallest first); ties by row"""
    diff = np.asarray(ssim_a, np.float64) - np.asarray(ssim_b, np.float64)
    return [int(r) for r in np.argsort(-diff, kind="stable")[:k]], [int(r) for r in np.argsort(diff, kind="stable")[:k]]


def load_pairs(OPT):
    """-> ({"a": (G, R, noiseDim), "b": ...}, dims, colorSpace): the checkpoints, or with --synthetic random-initialised nets - pair B built as
    train_vae builds and saves it (the decoder, and the encoder cut to its mean half)"""
    from . import models, synth, train_vae, vae
    if OPT.synthetic:
        c, h, w, nd = (int(v) for v in OPT.synthetic.split("x"))
        dims = (c, h, w)
        G = models.create_G(dims, nd, seed=OPT.seed); synth.init_params(G, OPT.seed)
        R = models.create_R(dims, nd, "normal", False, seed=OPT.seed + 1); synth.init_params(R, OPT.seed + 1)
        enc, dec = train_vae.build(dims, nd, OPT.seed + 2)
        synth.init_params(enc, OPT.seed + 3); synth.init_params(dec, OPT.seed + 4)
        return dict(a=(G, R, nd), b=(dec, vae.mean_reverser(enc), nd)), dims, "y" if c == 1 else "rgb"
    pairs, geometry = {}, {}
    for key, gpath, rpath in (("a", OPT.G, OPT.R), ("b", OPT.vaeG, OPT.vaeR)):
        ck = scripts.load_checkpoint(gpath)
        o = ck.get("opt", {})
        colorSpace = o.get("colorSpace", "rgb")
        geometry[key] = (scripts.image_dims(colorSpace, o.get("height", 32), o.get("width", 32)), colorSpace)
        pairs[key] = (ck["G"], scripts.load_checkpoint(rpath)["R"], int(o.get("noiseDim", 32 if key == "a" else 100)))
    if geometry["a"] != geometry["b"]:
        raise L.GanrevError(f"the pairs see different images: A {geometry['a']}, B {geometry['b']}")
    return pairs, geometry["a"][0], geometry["a"][1]


def real_images(OPT, ctx, dims, colorSpace):
    """the first --nbImages files of --dataset as apply_r --real loads them, where they land on the device; without --dataset ganrev.synth's
    stand-in images, uploaded -> (DeviceTensor, "dataset" | "synthetic")"""
    DATASET = scripts.open_dataset(OPT, colorSpace, dims[1], dims[2], ctx=ctx, reads=True)
    if DATASET is None:
        from . import synth
        t = DeviceTensor(ctx, (OPT.nbImages,) + tuple(dims))
        ctx.upload(synth.synthetic_images(OPT.nbImages, dims, OPT.seed * 7919), t.ptr)
        return t, "synthetic"
    have = len(DATASET.paths if DATASET.paths is not None else DATASET.loadPaths())
    if have < OPT.nbImages:
        raise L.GanrevError(f"--dataset holds {have} matching files, --nbImages asks for {OPT.nbImages}")
    res = DATASET.loadImages(1, OPT.nbImages, ctx=ctx)
    if tuple(res.images.shape[1:]) != tuple(dims):
        shape = res.images.shape[1:]; res.free()
        raise L.GanrevError(f"--dataset images are {shape} in colour space {colorSpace}, the nets take {tuple(dims)}")
    return res.images, "dataset"


def compare_grid(images, recon_a, recon_b, rows, from_space="rgb", path=None):
    """rows of (image, A's reconstruction, B's reconstruction), four triples to a picture row, for the image rows given: gathered into one sheet
    on the device (as render.cluster_grid does) and drawn by one gr_image_grid_dev launch"""
    from . import render
    ctx = images.ctx
    d = images.size // images.shape[0]
    with DeviceTensor(ctx, (3 * len(rows),) + tuple(images.shape[1:])) as sheet:
        for j, r in enumerate(rows):
            for s, t in enumerate((images, recon_a, recon_b)):
                ctx.copy2d(sheet.ptr + 4 * d * (3 * j + s), d, t.ptr + 4 * d * int(r), d, 1, d)
        return render.grid(sheet, np.arange(3 * len(rows)), 12, from_space, path=path)


def main(argv=None):
    OPT = parse(argv)
    try:
        return run(OPT)
    finally:
        if OPT.dataset != "NONE":                                             # --cacheDataset: the files' bytes go back with the run, however it ends
            from . import dataset
            dataset.uncache()


def run(OPT):
    import json
    import os
    ctx = L.Context(OPT.gpu) if OPT.gpu != int(os.environ.get("LOCAL_RANK", "0")) else L.default_context()
    ctx.set_conv_mode(OPT.conv_mode)
    say = (lambda *a: None) if OPT.quiet else print
    pairs, dims, colorSpace = load_pairs(OPT)
    L.ssim_check_args(OPT.nbImages, dims[0], dims[1], dims[2], OPT.win, quality.DATA_RANGE)
    for G, R, _ in pairs.values():
        for m in (G, R):
            m._ctx = ctx
            m.evaluate()
    os.makedirs(OPT.out, exist_ok=True)
    out = lambda name: os.path.join(OPT.out, name)
    N = OPT.nbImages
    summary = dict(dims=list(dims), nbImages=N, batchSize=OPT.batchSize, win=OPT.win, sigma=OPT.sigma, data_range=quality.DATA_RANGE)

    def score(exp, key, x, xhat):
        rows, mse, mean = quality.ssim(x, xhat, win=OPT.win, sigma=OPT.sigma)
        peak = quality.psnr(mse)
        for name, v in (("ssim", rows), ("mse", mse), ("psnr", peak)):
            np.save(out(f"compare_{exp}_{key}_{name}.npy"), v)
        summary.setdefault(exp, {})[key] = dict(ssim=quality.score_summary(rows), mse=quality.score_summary(mse), psnr=quality.score_summary(peak),
                                                ssim_mean_dev=mean)
        return rows, mse

    say("Own samples: x = G(z), x^ = G(R(x))...")
    for key, (G, R, nd) in pairs.items():
        with DeviceScope(ctx) as own:
            z = own.adopt(createNoiseInputsDev(ctx, N, nd, "normal", seed=OPT.seed + 1))
            x = own.adopt(forwardBatchedDev(G, z, OPT.batchSize))
            score("own", key, x, own.adopt(quality.reconstruct(G, R, x, OPT.batchSize)))

    say("Real images: x^ = G(R(x))...")
    recon, scores = {}, {}
    with DeviceScope(ctx) as own:
        x, corpus = real_images(OPT, ctx, dims, colorSpace)
        own.adopt(x)
        summary["real"] = dict(corpus=corpus)
        for key, (G, R, _) in pairs.items():
            recon[key] = own.adopt(quality.reconstruct(G, R, x, OPT.batchSize))
            scores[key] = score("real", key, x, recon[key])
        summary["real"]["a_wins_ssim"] = a_wins_share(scores["a"][0], scores["b"][0])
        summary["real"]["a_wins_mse"] = a_wins_share(-scores["a"][1].astype(np.float64), -scores["b"][1].astype(np.float64))     # a lower error wins
        if OPT.render:
            best, worst = extreme_rows(scores["a"][0], scores["b"][0])
            compare_grid(x, recon["a"], recon["b"], best + worst, colorSpace, path=out("compare_real.png"))
            summary["real"]["rendered_rows"] = best + worst
    json.dump(summary, open(out("summary.json"), "w"), indent=1)
    say("<compare> results in", OPT.out, summary)
    return summary


if __name__ == "__main__":
    main()
