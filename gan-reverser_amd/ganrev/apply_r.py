"""Mirror of the analysis steps of the reference's apply_r.lua that sit on (or right next to) the hot path.

  embed                        apply_r.lua:145-153   images = G(noise); attributes = R(images)   (forwardBatched, batch 32)
  createSimilaritySearch       apply_r.lua:265-318   needle rows i*100, cosine top-n on recovered noise / on raw pixels
  cosineSimilarity             apply_r.lua:396-400
  fixFaces                     apply_r.lua:324-352   noise -> G -> image -> R_fixer -> noise -> G -> image
  detectAnomalies              apply_r.lua:355-390   1 - torch.dist(image, fixed image), lowest `threshold` share = anomalies
                                                     (--anomalyMetric ssim: the structural similarity of the two instead, ganrev.quality)
  createClusterImages          apply_r.lua:197-231   unsup.kmeans on the recovered noise, nearest-centroid pass, per-cluster lists
  main, run                    apply_r.lua:25-193    the whole analysis as one run (parse: its options, apply_r.lua:13-23)

  embed_dev, embedImagesDev    apply_r.lua:145-153   the same where the tables stay on the GPU: G(noise), or R over an image table (--real, --needles)
  createSimilaritySearchDev    apply_r.lua:265-318   ... the needle rows searched where the embeddings were written
  searchByExample              -                     ... needles from outside the corpus (--needles)
  createClusterImagesDev       apply_r.lua:197-243   ... clusters and average faces; its parts: checkClusterCount, initialCentroids,
                                                     selectClusterMembers, clusterTableDev, clusterHostTable
  analyseDev, renderAnalysis   apply_r.lua:158-191   ... clusters, fixed faces and anomalies (--resident), with the pictures (--render)
  lowestShare, anomalyMetric   apply_r.lua:368-372   the anomaly rule on any per-image score
  principalAxesOfTable, mapOfTable, mixtureOfTable   --pca, --map, --mixture: ganrev.pca, ganrev.tsne, ganrev.mixture over the attribute table
  silhouetteStep, silhouetteSweep                    --silhouette, --silhouetteSweep: ganrev.silhouette over the labellings of that table
  outlierStep, mapNeighboursKept                     --outliers, --mapNeighbours: ganrev.knn, the neighbour graph of that table - outlier factors, and
                                                     how much of every row's neighbourhood the map (the whitened projection) kept
  densityStep                                        --density: ganrev.density, DBSCAN over that table - the cluster count it finds, and the rows
                                                     that belong to no cluster
  hierarchyStep                                      --hierarchy: ganrev.hierarchy, HDBSCAN over that table - no eps: the spanning tree on the device,
                                                     the linkage, the labels and the membership strengths read off it
  clusterOptions, pcaOptions, mapOptions, mixtureOptions, silhouetteOptions, outlierOptions, mapNeighbourOptions, densityOptions, hierarchyOptions   what a run's options say about each, with the defaults

These functions return the tensors / index lists the reference renders; the pictures themselves (image.toDisplayTensor plus the
frames and fields apply_r.lua draws) come from ganrev.render, on the GPU, and main() writes them with --render.
"""
import contextlib
import json
import math
import os
import time

import numpy as np

from . import _lib as L
from . import render, scripts
from .nn_utils import DeviceScope, DeviceTensor, createNoiseInputs, createNoiseInputsDev, deviceTable, forwardBatched, forwardBatchedDev


def embed(model_g, model_r, noise, batchSize=32, model_r_fixer=None):
    """apply_r.lua:145-153.  Returns (images, attributes[, attributesFixer])."""
    model_g.evaluate()
    images = forwardBatched(model_g, noise, batchSize)                      # :146
    model_r.evaluate()
    attributes = forwardBatched(model_r, images, batchSize)                 # :152
    if model_r_fixer is None:
        return images, attributes
    model_r_fixer.evaluate()                                                # the fixer's first Dropout stays on (models.lua:402-405)
    return images, attributes, forwardBatched(model_r_fixer, images, batchSize)   # :153


def embed_dev(model_g, model_r, noise, batchSize=512, model_r_fixer=None, keep_images=False, dims=None):
    """apply_r.lua:145-153 resident on the GPU (gr_embed_dev): `noise` is a DeviceTensor [N x noiseDim] (nn_utils.createNoiseInputsDev);
    per chunk of batchSize rows  G:forward -> R:forward [-> R_fixer:forward], the recovered noise written straight into [N x nd] device
    tables.  -> (images or None, attributes[, attributesFixer]) as DeviceTensors.  The images are a chunk-sized intermediate unless
    keep_images (the pixel-wise search and fix-faces want them: N x C x H x W floats).  dims = (C, H, W) of the images; taken from
    model_g's compiled net when it has run before.  Same kernels, same chunking as forwardBatched with this batchSize: same bits."""
    ctx = noise.ctx
    model_g.evaluate(); model_r.evaluate()
    gnet = model_g.device_net(noise.shape[1:])
    dims = tuple(dims) if dims is not None else gnet.out_dims
    rs = [model_r] + ([model_r_fixer] if model_r_fixer is not None else [])
    if model_r_fixer is not None:
        model_r_fixer.evaluate()                                            # its first Dropout stays on (models.lua:402-405)
    rnets = [m.device_net(dims) for m in rs]
    N = noise.shape[0]
    if ctx.conv_mode() == "f16x3":
        for n in [gnet] + rnets:          # the *_dev calls are not range-guarded (include/ganrev.h): one synchronous scan per net
            n.range_guard_scan()
    images = DeviceTensor(ctx, (N,) + tuple(dims)) if keep_images else None
    attrs = [DeviceTensor(ctx, (N,) + L.Net._shape(n.out_dims)) for n in rnets]
    L.embed_dev(gnet, rnets, noise.ptr, N, batchSize, [a.ptr for a in attrs], images.ptr if images is not None else None)
    return (images,) + tuple(attrs)


def createSimilaritySearchDev(nbSimilarNeedles, nbShowMax, attributes, images=None):
    """apply_r.lua:265-318 on device-resident tables (DeviceTensors from embed_dev): the needles' rows are searched where the embeddings
    were written.  -> (idx_by_attributes, idx_by_pixels or None)."""
    N = attributes.shape[0]
    needles = np.array([i * 100 - 1 for i in range(1, nbSimilarNeedles + 1)], dtype=np.int64)
    if needles.max() >= N:
        raise IndexError(f"needle row {needles.max() + 1} out of range for {N} rows")
    n = min(nbShowMax, N)
    ctx = attributes.ctx
    by_attr, _ = ctx.cosine_topk(None, needles, n, emb_dev=attributes.ptr, n=N, d=attributes.size // N)
    by_pix = None
    if images is not None:
        by_pix, _ = ctx.cosine_topk(None, needles, n, emb_dev=images.ptr, n=N, d=images.size // N)
    return by_attr, by_pix


def embedImagesDev(models_r, images, batchSize=512):
    """apply_r.lua:152-153 over an image table that is already on the GPU (`images` a DeviceTensor [N x C x H x W]: a --dataset's files, any
    table that did not come from G): attributes_k = R_k:forward(images) in chunks of batchSize, in evaluate() mode, where embed_dev leaves
    them.  -> one DeviceTensor [N x nd_k] per model."""
    ctx = images.ctx
    outs = []
    for m in models_r:
        m.evaluate()
        net = m.device_net(images.shape[1:])
        if ctx.conv_mode() == "f16x3":
            net.range_guard_scan()        # the *_dev calls are not range-guarded (include/ganrev.h): one synchronous scan per net, as in embed_dev
        outs.append(forwardBatchedDev(m, images, batchSize))
    return outs


def searchByExample(nbShowMax, attributes, needle_attributes, images=None, needle_images=None):
    """Search by example, the counterpart of createSimilaritySearchDev for needles that are not rows of the corpus: every row of
    `needle_attributes` [Q x nd] (R over some other images - a photo) against the corpus table `attributes` [N x nd], and - with both image
    tables - every needle image against the corpus images pixel-wise.  All four are DeviceTensors; nothing but the index lists leaves the
    GPU (gr_cosine_topk_queries_dev).  -> (idx_by_attributes, idx_by_pixels or None): per needle the min(nbShowMax, N) most similar corpus
    rows, best first, ties by ascending index; there is no self hit."""
    N, Q = attributes.shape[0], needle_attributes.shape[0]
    n = min(nbShowMax, N)
    ctx = attributes.ctx
    d = attributes.size // N
    if needle_attributes.size != Q * d:
        raise L.GanrevError(f"searchByExample: needles of {needle_attributes.size // max(Q, 1)} attributes against a table of {d}")
    by_attr, _ = ctx.cosine_topk_queries(None, None, n, emb_dev=attributes.ptr, n=N, d=d, queries_dev=needle_attributes.ptr, q=Q)
    by_pix = None
    if images is not None and needle_images is not None:
        chw = images.size // N
        if needle_images.size != Q * chw:
            raise L.GanrevError(f"searchByExample: needle images of {needle_images.size // max(Q, 1)} values against images of {chw}")
        by_pix, _ = ctx.cosine_topk_queries(None, None, n, emb_dev=images.ptr, n=N, d=chw, queries_dev=needle_images.ptr, q=Q)
    return by_attr, by_pix


def cosineSimilarity(v1, v2):
    """apply_r.lua:396-400."""
    return L.default_context().cosine_similarity(v1, v2)


def createSimilaritySearch(nbSimilarNeedles, nbShowMax, images, attributes):
    """apply_r.lua:265-318.  -> (idx_by_attributes, idx_by_pixels): for needle i (row i*100, 1-based in the reference) the
    row indices (0-based here) of the min(nbShowMax, N) most similar rows, best first, ties by ascending index."""
    N = len(attributes)
    needles = np.array([i * 100 - 1 for i in range(1, nbSimilarNeedles + 1)], dtype=np.int64)   # face_i_idx = i*100 (1-based)
    if needles.max() >= N:
        raise IndexError(f"needle row {needles.max() + 1} out of range for {N} rows")           # the reference would index nil
    n = min(nbShowMax, N)
    ctx = L.default_context()
    by_attr, _ = ctx.cosine_topk(attributes, needles, n)                                        # similarityMeasureAttributes
    by_pix, _ = ctx.cosine_topk(np.asarray(images, np.float32).reshape(N, -1), needles, n)      # similarityMeasurePixelwise
    return by_attr, by_pix


def fixFaces(nbFixedImages, model_g, attributesFixer, batchSize=32):
    """apply_r.lua:344-351: the G(R_fixer(G(z))) images of the first nbFixedImages rows."""
    model_g.evaluate()
    return forwardBatched(model_g, attributesFixer[:nbFixedImages], batchSize)


def detectAnomalies(nbImagesCalculations, threshold, images, model_g, attributesFixer, batchSize=32):
    """apply_r.lua:355-390.  -> (distances, anomalyBelow, isAnomaly) with distances[i] = 1 - torch.dist(images[i], fixed[i]).
    The reference forwards each row in a batch of two (:361-363, BatchNorm needs a batch) — G is in evaluate() mode, so the
    result does not depend on the batch composition and the rows are forwarded in normal batches here."""
    n = nbImagesCalculations
    model_g.evaluate()
    fixed = forwardBatched(model_g, attributesFixer[:n], batchSize)
    dist = 1.0 - L.default_context().l2_distance_rows(images[:n], fixed)
    return (dist,) + lowestShare(dist, threshold)                           # :368-372


def lowestShare(score, threshold):
    """apply_r.lua:368-372 on any per-image score: (anomalyBelow, isAnomaly) - the floor(n * threshold)-th lowest value (1-based, at least the
    first) and every row at or below it"""
    srt = np.sort(score)                                                    # table.sort(distancesForSort)
    below = srt[max(int(math.floor(len(srt) * threshold)) - 1, 0)]          # distancesForSort[floor(#*threshold)]  (1-based)
    return below, score <= below


def anomalyMetric(OPT):
    """--anomalyMetric of a run: dist, the reference's 1 - torch.dist, unless asked otherwise"""
    return getattr(OPT, "anomalyMetric", "dist")


def initialCentroids(nbClusters, nDims, seed=1):
    """unsup.kmeans draws its initial centroids as `x.new(k, ndims):normal()` and divides each row by its norm.  Torch's
    Mersenne-twister stream is not reproducible here; the same distribution from the package's counter RNG."""
    from . import synth
    c = synth.normal((nbClusters, nDims), seed).astype(np.float32)
    return c / np.linalg.norm(c.astype(np.float64), axis=1, keepdims=True).astype(np.float32)


def selectClusterMembers(label, sim, nbClusters, nbMaxPerCluster):
    """apply_r.lua:218-227 on host arrays: per cluster the rows sorted by similarity descending (table.sort with a[2] > b[2]; ties by row, a NaN
    last: a stable argsort of -similarity) and the first nbMaxPerCluster of them -> [row index arrays], one per cluster"""
    keeps = []
    for j in range(nbClusters):
        rows = np.nonzero(label == j)[0]
        order = np.argsort(-sim[rows], kind="stable")                                               # :221 (a[2] > b[2]); ties by row
        keeps.append(rows[order][:nbMaxPerCluster])                                                 # :223-227
    return keeps


MAX_CLUSTERS, NARROW_MAX_CLUSTERS, MAX_PER_CLUSTER = 4096, 32, 128      # gr_cluster_dev's limits; the k the three older calls take


def checkClusterCount(nbClusters):
    if not 1 <= int(nbClusters) <= MAX_CLUSTERS:
        raise L.GanrevError(f"nbClusters {nbClusters}: 1 to {MAX_CLUSTERS} clusters")
    return int(nbClusters)


def clusterTableDev(ctx, table_ptr, N, d, k, nbIterations, m, centroids0, closest, faces_of=None, labels_into=None):
    """apply_r.lua:198-227 on a device table [N x d].  Up to 32 clusters: gr_kmeans_dev, gr_cosine_assign_dev, gr_cluster_members_dev, as ever;
    above: gr_cluster_dev, one enqueue.  faces_of = (images pointer, rows of that table, values per image, output pointer) adds gr_cluster_faces_dev
    (apply_r.lua:233-243) while the lists are still on the device.  labels_into: a list that receives the [N] int32 labels of the cosine
    assignment (:205-217), which no list keeps beyond the m best rows of a cluster.  -> (centroids, counts, clusters)"""
    sizes = [4 * k, 4 * N, 4 * N, 8 * k * m, 4 * k * m, 4 * k, 4 * k]               # counts, labels, sims, rows, their sims, kept, cluster sizes
    with DeviceScope(ctx) as bufs:
        cent = bufs.upload(np.ascontiguousarray(centroids0, np.float32).reshape(k, d))
        tot, lab, sim, rows, rsim, kept, csize = [bufs.malloc(b) for b in sizes]
        if k <= NARROW_MAX_CLUSTERS:
            ctx.kmeans_dev(table_ptr, N, d, k, nbIterations, cent, tot, lab)                    # :198
            ctx.cosine_assign_dev(table_ptr, N, d, cent, k, not closest, lab, sim)              # :205-217
            ctx.cluster_members_dev(lab, sim, N, k, m, rows, rsim, kept, csize)                 # :218-227
        else:
            ctx.cluster_dev(table_ptr, N, d, k, nbIterations, cent, not closest, m, tot, lab, sim, rows, rsim, kept, csize)
        if faces_of is not None:
            images_ptr, n_rows, chw, faces_ptr = faces_of
            ctx.cluster_faces_dev(images_ptr, n_rows, chw, rows, kept, k, m, faces_ptr)         # :233-243 (zeros for an empty cluster)
        centroids, counts = ctx.download(cent, (k, d)), ctx.download(tot, (k,))
        hrows, hsim, hkept = ctx.download(rows, (k, m), np.int64), ctx.download(rsim, (k, m)), ctx.download(kept, (k,), np.int32)
        if labels_into is not None:
            labels_into.append(ctx.download(lab, (N,), np.int32))
    clusters = [[(int(r), float(v)) for r, v in zip(hrows[j, :hkept[j]], hsim[j, :hkept[j]])] for j in range(k)]
    return centroids, counts, clusters


def clusterHostTable(ctx, attributes, k, nbIterations, m, centroids0, closest, faces_of=None):
    """clusterTableDev for a host attribute table: uploaded to a temporary buffer first (more than 32 clusters: gr_cluster_dev has no host variant)"""
    with deviceTable(ctx, attributes) as (table, N, d):
        return clusterTableDev(ctx, table, N, d, k, nbIterations, m, centroids0, closest, faces_of)


def clusterHostRoute(ctx, attributes, k, nbIterations, m, centroids0, closest):
    """apply_r.lua:198-227 for a host table of up to 32 clusters -> (centroids, counts, label, sim, [kept row index arrays])"""
    centroids, counts, _ = ctx.kmeans(attributes, k, nbIterations, centroids0)                     # :198
    label, sim = ctx.cosine_assign(attributes, centroids, take_min=not closest)                     # :205-217
    return centroids, counts, label, sim, selectClusterMembers(label, sim, k, m)                    # :218-227


def clusterInputs(nbClusters, nbMaxPerCluster, attributes, centroids0, seed):
    """-> (k, m, the attribute table - a DeviceTensor as it is, anything else as a float32 array -, the initial centroids: drawn unless given)"""
    k = checkClusterCount(nbClusters)
    if not isinstance(attributes, DeviceTensor):
        attributes = np.asarray(attributes, np.float32)
    if centroids0 is None:
        centroids0 = initialCentroids(k, attributes.size // attributes.shape[0], seed)
    return k, int(nbMaxPerCluster), attributes, centroids0


def createClusterImages(nbClusters, nbIterations, nbMaxPerCluster, images, attributes, centroids0=None, seed=1, closest=False):
    """apply_r.lua:197-231 without the image writing.  -> (centroids, counts, clusters, averageFaces): clusters[j] is the list
    of (row index, similarity) kept for cluster j, sorted like the reference (similarity descending, first nbMaxPerCluster);
    averageFaces[j] the mean image of those rows (zeros / NaN-free for an empty cluster: the reference divides by zero there
    and skips the cluster when saving, :243,:251).

    Reference behaviour preserved: a row joins the centroid with the MINIMUM cosine similarity (:207-214 keep `dist <
    minDist` of a similarity).  closest=True assigns to the most similar centroid instead.

    Up to 4096 clusters.  The reference's 20, and anything up to 32, run as ever; above 32 the attribute table is uploaded and clustered by
    gr_cluster_dev (lists of at most 128 rows), and the faces are averaged from its lists the same way."""
    k, m, attributes, centroids0 = clusterInputs(nbClusters, nbMaxPerCluster, attributes, centroids0, seed)
    ctx = L.default_context()
    if k > NARROW_MAX_CLUSTERS:
        centroids, counts, clusters = clusterHostTable(ctx, attributes, k, nbIterations, m, centroids0, closest)
    else:
        centroids, counts, _, sim, keeps = clusterHostRoute(ctx, attributes, k, nbIterations, m, centroids0, closest)
        clusters = [[(int(r), float(sim[r])) for r in keep] for keep in keeps]
    images = np.asarray(images, np.float32)
    faces = [images[[r for r, _ in cl]].mean(axis=0, dtype=np.float64).astype(np.float32) if cl else np.zeros(images.shape[1:], np.float32)
             for cl in clusters]                                                                    # :233-243
    return centroids, counts, clusters, faces


def createClusterImagesDev(nbClusters, nbIterations, nbMaxPerCluster, images, attributes, centroids0=None, seed=1, closest=False):
    """createClusterImages with the images resident on the GPU (`images` a DeviceTensor [N x C x H x W]; `attributes` [N x nd] the small
    host table or the DeviceTensor embed_dev wrote): k-means and the assignment as there, the average faces by gr_rows_mean_dev's
    arithmetic - the cluster's rows added in the cluster's order in fp32 and divided once, as the reference's face:add / face:div
    (apply_r.lua:233-243).  createClusterImages averages in float64 on the host: the faces may differ from it in the last bits.
    With a device table nothing of size N crosses the bus: gr_kmeans_dev, gr_cosine_assign_dev, gr_cluster_members_dev and
    gr_cluster_faces_dev run where the table lies, and the [k x m] lists, the centroids and the counts come back - the same tuple, bit for bit.
    Up to 4096 clusters: above 32, gr_cluster_dev stands for the first three calls (a host table is uploaded for it), lists of at most 128 rows.
    -> (centroids, counts, clusters, faces) with faces a DeviceTensor [nbClusters x C x H x W] (the caller frees it)."""
    ctx = images.ctx
    chw = images.size // images.shape[0]
    k, m, attributes, centroids0 = clusterInputs(nbClusters, nbMaxPerCluster, attributes, centroids0, seed)
    faces = DeviceTensor(ctx, (k,) + tuple(images.shape[1:]))
    try:
        if isinstance(attributes, DeviceTensor) or k > NARROW_MAX_CLUSTERS: # (a host table of more than 32 clusters is uploaded: gr_cluster_dev)
            with deviceTable(ctx, attributes) as (table, N, d):
                centroids, counts, clusters = clusterTableDev(ctx, table, N, d, k, nbIterations, m, centroids0, closest, (images.ptr, images.shape[0], chw, faces.ptr))
        else:
            centroids, counts, _, sim, keeps = clusterHostRoute(ctx, attributes, k, nbIterations, m, centroids0, closest)
            clusters = [[(int(r), float(sim[r])) for r in keep] for keep in keeps]
            for j, keep in enumerate(keeps):
                ctx.rows_mean_dev(images.ptr, images.shape[0], chw, keep, faces.ptr + 4 * chw * j)      # :233-243 (zeros for an empty cluster)
    except Exception:
        faces.free()
        raise
    return centroids, counts, clusters, faces


def principalAxesOfTable(ctx, attributes, K, whitened=False):
    """--pca K: the principal axes of the attribute table (ganrev.pca) - a DeviceTensor [N x nd] where gr_embed_dev left it, or the host table,
    uploaded to a temporary buffer first as clusterHostTable does.  -> (PrincipalAxes, which the caller closes; the [N x K] coordinates along
    the first K axes on the host, not whitened; the whitened [N x K] table as a DeviceTensor the caller frees, or None)"""
    from . import pca as P
    with deviceTable(ctx, attributes) as (table, N, d):
        axes = P.principalAxes(ctx, table, N, d)
        try:
            with P.project(ctx, axes, table, N, K, whiten=False) as plain:
                coords = plain.numpy()
            return axes, coords, P.project(ctx, axes, table, N, K, whiten=True) if whitened else None
        except Exception:
            axes.close()
            raise


def analyseDev(OPT, MODEL_G, images, attributes, attributesFixer, out=None, colorSpace=None, by_attr=None, by_pix=None, mixture=None):
    """The analysis of apply_r.lua:158-191 on the device-resident tables (`images` [N x C x H x W] and `attributesFixer` [N x nd] as
    DeviceTensors, `attributes` [N x nd] a DeviceTensor or the host table): the clusters (createClusterImagesDev), the fixed faces and the
    anomaly distance.  Only the rows a step needs are read; the image table stays where it is.  With `out` (name -> path) the reference's
    pictures are written as PNG files on the way (ganrev.render): cluster_%02d, similar_attributes_%02d / similar_pixelwise_%02d,
    fixed_pairs, fixed_images_<n>[_unfixed] and anomalies; nothing but the finished pictures and the per-image distances leaves the GPU.
    -> what the run's arrays and summary are written from: dict(clusters = createClusterImagesDev's tuple with the faces on the host,
    fixed = the fixed images [nbFixed x C x H x W], anomalies = detectAnomalies' tuple).  mixture: the steps that follow the clustering in its
    table (--mixture, --silhouette), called with the final centroids while the tables are still where they are.  --anomalyMetric ssim: the same rows are also scored with quality.ssim(images, fixed
    images) where they lie, the lowest 15 % of THAT score are the anomalies (anomalies = (ssim, below, flags)), and the distances come back
    beside them as `distances`."""
    ctx, N = images.ctx, images.shape[0]
    chw = images.size // N
    nbClusters, nbIterations, nbMaxPerCluster, closest = clusterOptions(OPT)                                            # :159-161: 20, 15, 64 + 7
    centroids, counts, clusters, faces = createClusterImagesDev(nbClusters, nbIterations, nbMaxPerCluster, images, attributes, seed=OPT.seed, closest=closest)      # :158-163
    with faces:
        for j, cl in enumerate(clusters):
            if cl and out:                                                                                              # :249
                render.cluster_grid(images, [r for r, _ in cl], colorSpace, face_dev=faces.rows(j, j + 1), path=out("cluster_%02d.png" % (j + 1)))
        faces_host = faces.numpy()
    if by_attr is not None and out:                                                                                     # :170-172
        for i in range(len(by_attr)):
            render.similar_grid(images, by_attr[i], colorSpace, path=out("similar_attributes_%02d.png" % (i + 1)))
            render.similar_grid(images, by_pix[i], colorSpace, path=out("similar_pixelwise_%02d.png" % (i + 1)))
    MODEL_G.evaluate()
    nbFixed, nbCalc = min(512 + 16, N), min(1024, N)
    with forwardBatchedDev(MODEL_G, attributesFixer.rows(0, nbFixed), OPT.batchSize) as fixed:                          # :349
        if out:
            render.fixed_pairs_grid(images, fixed, min(52, N), colorSpace, path=out("fixed_pairs.png"))                 # :325-342
            render.fixed_images_grid(images, nbFixed, path=out("fixed_images_%d_unfixed.png" % nbFixed))                # :345-347
            render.fixed_images_grid(fixed, nbFixed, path=out("fixed_images_%d.png" % nbFixed))                         # :350-351
        # (one transfer per batch, as every other step here moves batches; the host array is nbFixed images either way)
        fixed_host = np.concatenate([fixed.rows(lo, min(lo + OPT.batchSize, nbFixed)).numpy() for lo in range(0, nbFixed, OPT.batchSize)])
    with forwardBatchedDev(MODEL_G, attributesFixer.rows(0, nbCalc), OPT.batchSize) as fixedCalc:                       # :360-363
        dist = 1.0 - ctx.l2_distance_rows_dev(images.ptr, fixedCalc.ptr, nbCalc, chw)                                   # :366, scored where the images lie
        score = dist
        if anomalyMetric(OPT) == "ssim":
            from . import quality
            score, _, _ = quality.ssim(images.rows(0, nbCalc), fixedCalc)
    below, is_anom = lowestShare(score, 0.15)                                                                           # :371-372
    if out:
        render.anomalies_grid(images, is_anom[:min(512 + 16, nbCalc)], colorSpace, path=out("anomalies.png"))           # :374-389
    if mixture is not None:
        mixture(attributes, centroids, images)
    return dict(clusters=(centroids, counts, clusters, list(faces_host)), fixed=fixed_host, anomalies=(score, below, is_anom), distances=dist)


def renderAnalysis(OPT, out, colorSpace, MODEL_G, images, attributes, attributesFixer, by_attr, by_pix, mixture=None):
    """analyseDev with the pictures of apply_r.lua:158-191 written as PNG files out(name)."""
    return analyseDev(OPT, MODEL_G, images, attributes, attributesFixer, out, colorSpace, by_attr, by_pix, mixture)


def clusterOptions(OPT):
    """(nbClusters, nbIterations, nbMaxPerCluster, closest) of a run: the options given, else what apply_r.lua:159-163 hard-codes"""
    return (getattr(OPT, "nbClusters", 20), getattr(OPT, "nbIterations", 15), getattr(OPT, "nbMaxPerCluster", 64 + 7), bool(getattr(OPT, "closest", False)))


def pcaOptions(OPT):
    """(K, pcaSpace) of a run: --pca K and --pcaSpace when given, else (0, False): off"""
    return int(getattr(OPT, "pca", 0)), bool(getattr(OPT, "pcaSpace", False))


def mixtureOptions(OPT):
    """EM iterations of a --mixture run; None without --mixture"""
    return int(OPT.mixture) if hasattr(OPT, "mixture") else None


MAX_COMPONENTS = L.Context.MIXTURE_MAX_K     # gr_mixture_dev's limit


def mixtureOfTable(ctx, table, centroids, iterations, column_variances=None, needle_rows=None):
    """--mixture ITER: a diagonal Gaussian mixture (ganrev.mixture) fitted to the table the clustering read - a DeviceTensor, or the host table,
    uploaded to a temporary buffer first as clusterHostTable does - by ITER EM iterations from the clustering's final centroids; then every row,
    and every needle row [Q x d] if given, scored under it -> (Mixture, (labels, posterior, row log-likelihood), the needles' triple or None)"""
    from . import mixture as MX
    with deviceTable(ctx, table) as (ptr, N, d):
        fitted = MX.fit(ctx, ptr, N, d, centroids, iterations, column_variances=column_variances)
        rows = MX.score(ctx, fitted, ptr, N)
        needles = None
        if needle_rows is not None:
            with deviceTable(ctx, needle_rows) as (q, Q, _):
                needles = MX.score(ctx, fitted, q, Q)
        return fitted, rows, needles


SILHOUETTE_MAX_ROWS = L.Context.SILHOUETTE_MAX_N     # gr_silhouette_dev's limit (GR_SILHOUETTE_MAX_N)
SILHOUETTE_METRICS = ("euclidean", "cosine")


def silhouetteOptions(OPT):
    """(rows, [the K of --silhouetteSweep]) of a run with --silhouette or --silhouetteSweep: the first `rows` rows are scored, the option given,
    else min(nbImages, 100000); None without either"""
    if not (getattr(OPT, "silhouette", False) or hasattr(OPT, "silhouetteSweep")):
        return None
    sweep = [int(v) for v in OPT.silhouetteSweep.split(",")] if hasattr(OPT, "silhouetteSweep") else []
    return int(getattr(OPT, "silhouetteRows", min(OPT.nbImages, 100000))), sweep


def silhouetteOfLabels(ctx, table, rows, labels, k):
    """ganrev.silhouette of the first `rows` rows of a device table (pointer, N, d) under labels [N] (later rows are nobody's member), in both
    metrics -> {metric: Silhouette}"""
    from . import silhouette as SIL
    return {metric: SIL.score(ctx, table, labels[:rows], k, metric, rows=rows) for metric in SILHOUETTE_METRICS}


OUTLIER_MAX_ROWS, OUTLIER_MAX_K = L.Context.KNN_MAX_N, L.Context.KNN_MAX_K     # gr_knn_dev's limits (GR_KNN_MAX_N, GR_KNN_MAX_K)
OUTLIER_METRICS = ("cosine", "euclidean")


def outlierMetric(OPT):
    """--outlierMetric: the distance of the neighbour graphs; cosine, the search's geometry, unless asked otherwise"""
    return getattr(OPT, "outlierMetric", "cosine")


def outlierOptions(OPT):
    """(K, rows, metric) of a run with --outliers K: the graph of the first `rows` rows, the option given, else min(nbImages, 100000); None
    without --outliers"""
    if not hasattr(OPT, "outliers"):
        return None
    return int(OPT.outliers), int(getattr(OPT, "outlierRows", min(OPT.nbImages, 100000))), outlierMetric(OPT)


def mapNeighbourOptions(OPT):
    """(K, metric of the table's graph) of a run with --mapNeighbours K; None without it"""
    return (int(OPT.mapNeighbours), outlierMetric(OPT)) if hasattr(OPT, "mapNeighbours") else None


def mapNeighboursKept(ctx, table, y, M, K, metric):
    """--mapNeighbours K: the graph of the first M rows of the table the map was made from against the graph of the map y [M x 2] (euclidean: the
    picture's own geometry) -> (kept [M] int32: how many of a row's K nearest rows in the table are among its K nearest in the map, the mean share)"""
    from . import knn as KNN
    with KNN.graph(ctx, table, K, metric, rows=M, keep=True) as there, KNN.graph(ctx, y, K, "euclidean", keep=True) as here:
        return KNN.overlap(ctx, there, here)


DENSITY_MAX_ROWS = L.Context.DBSCAN_MAX_N     # gr_eps_graph_dev's limit (GR_DBSCAN_MAX_N)
DENSITY_MAX_MINPTS_BY_QUANTILE = L.Context.KNN_MAX_K + 1     # the quantile route reads the distance to the (minPts - 1)-th of at most 128 neighbours
DENSITY_METRICS = ("cosine", "euclidean")
DENSITY_OPTIONS = ("densityMinPts", "densityEps", "densityQuantile", "densityRows", "densityMetric")


def densityOptions(OPT):
    """(minPts, eps or None, quantile or None, rows, metric) of a run with --density: DBSCAN of the first `rows` rows, the option given, else
    min(nbImages, 100000); eps as given, else the quantile (0.75 unless given) of the rows' distances to their (minPts - 1)-th neighbour; None
    without --density"""
    if not getattr(OPT, "density", False):
        return None
    eps = float(OPT.densityEps) if hasattr(OPT, "densityEps") else None
    quantile = None if eps is not None else float(getattr(OPT, "densityQuantile", 0.75))
    return (int(getattr(OPT, "densityMinPts", 10)), eps, quantile, int(getattr(OPT, "densityRows", min(OPT.nbImages, 100000))),
            getattr(OPT, "densityMetric", "cosine"))


HIERARCHY_MAX_ROWS = L.Context.MST_MAX_N      # gr_mst_dev's limit (GR_MST_MAX_N)
HIERARCHY_MAX_MINSAMPLES = L.Context.KNN_MAX_K + 1     # the core distance is the distance to the (S - 1)-th of at most 128 neighbours
HIERARCHY_METRICS = ("cosine", "euclidean")
HIERARCHY_OPTIONS = ("hierarchyMinSamples", "hierarchyMinClusterSize", "hierarchyRows", "hierarchyMetric", "hierarchyCut")


def hierarchyOptions(OPT):
    """(minSamples, minClusterSize, rows, metric, cut or None) of a run with --hierarchy: HDBSCAN of the first `rows` rows, the options given,
    else 10, 25, min(nbImages, 100000), cosine and no cut; None without --hierarchy"""
    if not getattr(OPT, "hierarchy", False):
        return None
    return (int(getattr(OPT, "hierarchyMinSamples", 10)), int(getattr(OPT, "hierarchyMinClusterSize", 25)),
            int(getattr(OPT, "hierarchyRows", min(OPT.nbImages, 100000))), getattr(OPT, "hierarchyMetric", "cosine"),
            float(OPT.hierarchyCut) if hasattr(OPT, "hierarchyCut") else None)


MAP_MAX_ROWS = L.Context.TSNE_MAX_N     # gr_tsne_*_dev's limit (GR_TSNE_MAX_N)


def mapOptions(OPT):
    """(rows, perplexity, iterations, grid) of a --map run: the options given, else min(nbImages, 10000), 30, 1000, 32; None without --map"""
    if not getattr(OPT, "map", False):
        return None
    return (int(getattr(OPT, "mapRows", min(OPT.nbImages, 10000))), float(getattr(OPT, "mapPerplexity", 30.0)), int(getattr(OPT, "mapIterations", 1000)),
            int(getattr(OPT, "mapGrid", 32)))


def mapOfTable(ctx, table, M, perplexity, iterations, grid):
    """--map: the t-SNE map (ganrev.tsne) of the first M rows of the attribute table - a DeviceTensor where gr_embed_dev left it, or the host
    table, uploaded to a temporary buffer first as principalAxesOfTable does -> (y [M x 2], (iterations, KL values), cell rows [grid x grid],
    the summary entry)"""
    from . import tsne as T
    with deviceTable(ctx, table, rows=M) as (ptr, _, d), contextlib.closing(T.embed(ctx, ptr, M, d, perplexity=perplexity, iterations=iterations)) as e:
        cells = T.mapCells(ctx, e.y_dev, M, grid, grid)
        entry = dict(rows=M, d=d, perplexity=perplexity, iterations=iterations, grid=grid, eta=e.eta, beta_updates_max=e.tries, beta_capped_rows=e.capped,
                     kl_first=float(e.kl[0]), kl_last=float(e.kl[-1]), cells_filled=int((cells >= 0).sum()))
        return e.y, (np.asarray(e.kl_iterations, np.int64), e.kl), cells, entry


def parse(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="apply_r.lua options (apply_r.lua:13-23)")
    p.add_argument("--batchSize", type=int, default=32)                       # apply_r.lua:14 (the device-resident pipeline likes 512)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--G", default="logs/adversarial.net")
    p.add_argument("--R", default="logs/r_3x32x32_nd32_normal.net")
    p.add_argument("--R_fixer", default="logs/r_3x32x32_nd32_normal_fixer.net")
    p.add_argument("--writeTo", default="r_results")
    p.add_argument("--nbImages", type=int, default=10000)                     # apply_r.lua:145
    p.add_argument("--synthetic", default="", help="CxHxWxND, e.g. 1x32x32x32: random-initialised G / R / R_fixer instead of checkpoints")
    p.add_argument("--host", action="store_true", help="the host-tensor loop (forwardBatched per chunk, as apply_r.lua spells it) instead of the device-resident pipeline")
    scripts.add_dataset_options(p)                                            # apply_r.lua:16 --dataset (configured as there; read by --needles / --real only)
    p.add_argument("--needles", type=int, default=0, metavar="N", help="search by example: the first N files of --dataset (DATASET.loadPaths() order) are embedded with R and searched in the corpus by attributes and by pixels (device-resident pipeline only)")
    p.add_argument("--real", action="store_true", help="the corpus is the first --nbImages files of --dataset (apply_r.lua:144, commented out there) instead of G(noise) (device-resident pipeline only)")
    p.add_argument("--conv-mode", default="f16x3", choices=["f32", "bf16x6", "f16x3"])
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--resident", action="store_true", help="device-resident pipeline only: analyse the tables where the embedding wrote them; the image table is never copied to the host")
    p.add_argument("--render", action="store_true", help="also write the reference's pictures as PNG files (ganrev.render; colour space: the checkpoint's, y / rgb for 1- / 3-channel --synthetic nets)")
    # absent from the namespace unless given: anomalyMetric() supplies dist, and a run without the option writes the summary it wrote before it existed
    p.add_argument("--anomalyMetric", choices=["dist", "ssim"], default=argparse.SUPPRESS, help="the per-image score whose lowest 15 %% are the anomalies: dist, the reference's 1 - torch.dist(image, fixed image) (default), or ssim, the structural similarity of the two (ganrev.quality, 11 x 11 Gaussian window: images of 11 .. 128 pixels a side), scored where the tables lie: needs --resident or --render; writes anomaly_ssim.npy beside anomaly_distances.npy")
    p.add_argument("--refine", type=int, default=0, metavar="STEPS", help="refine the recovered noise through G: STEPS Adam steps per image on the MSE between G(z) and the image, starting at R's estimate (ganrev.refine; 0, the reference's behaviour: R's estimate is final)")
    p.add_argument("--refine_lr", type=float, default=0.01, help="Adam learning rate of --refine")
    # the principal-axes options: absent from the namespace unless given, like the clustering options below - pcaOptions() supplies "off"
    p.add_argument("--pca", type=int, default=argparse.SUPPRESS, metavar="K", help="principal axes of the recovered noise (ganrev.pca; K <= noiseDim): writes pca_mean, pca_eigenvalues, pca_axes [K x noiseDim] and pca_projection [nbImages x K] (.npy), and with --render variations_pca.png along the first K axes (0, the reference's behaviour: off)")
    p.add_argument("--pcaSpace", action="store_true", default=argparse.SUPPRESS, help="with --pca K: the similarity search by attributes and the clustering run on the whitened [nbImages x K] projection instead of the attribute table")
    # the map options: absent from the namespace unless given - mapOptions() supplies the defaults
    p.add_argument("--map", action="store_true", default=argparse.SUPPRESS, help="a two-dimensional t-SNE map of the recovered noise, on the device (ganrev.tsne; of the whitened projection with --pcaSpace): writes map_y [mapRows x 2], map_kl and map_cells [mapGrid x mapGrid] (.npy), and with --render map.png, the faces drawn where they land, ringed by cluster")
    p.add_argument("--mapRows", type=int, default=argparse.SUPPRESS, metavar="M", help=f"with --map: the first M rows are mapped (default min(nbImages, 10000); at most {MAP_MAX_ROWS}: the rows are independent draws, a prefix is a fair sample)")
    p.add_argument("--mapPerplexity", type=float, default=argparse.SUPPRESS, help="with --map: the perplexity (default 30; at most (mapRows - 1) / 3)")
    p.add_argument("--mapIterations", type=int, default=argparse.SUPPRESS, help="with --map: gradient iterations (default 1000)")
    p.add_argument("--mapGrid", type=int, default=argparse.SUPPRESS, metavar="G", help="with --map: map_cells and map.png have G x G cells (default 32)")
    # the silhouette options: absent from the namespace unless given - silhouetteOptions() supplies the defaults
    p.add_argument("--silhouette", action="store_true", default=argparse.SUPPRESS, help="silhouette coefficients of the clustering, on the device (ganrev.silhouette), in the table the clustering read: the cosine-assignment labels, and with --mixture the mixture's, each under the euclidean and the cosine distance; writes silhouette_{clusters,mixture}_{euclidean,cosine}.npy, silhouette_clusters_labels.npy and the means per labelling, metric and cluster into summary.json")
    p.add_argument("--silhouetteRows", type=int, default=argparse.SUPPRESS, metavar="M", help=f"with --silhouette / --silhouetteSweep: the first M rows are scored, later rows are nobody's member (default min(nbImages, 100000); at most {SILHOUETTE_MAX_ROWS}: every pair of rows is visited, the rows are independent draws, a prefix is a fair sample)")
    p.add_argument("--silhouetteSweep", default=argparse.SUPPRESS, metavar="K1,K2,...", help="which --nbClusters: the clustering is run again for each K (same seed, --nbIterations and --closest; no faces, no pictures) and scored; writes silhouette_sweep.json: K, the mean silhouette under both distances, the number of empty clusters")
    # the neighbour-graph options: absent from the namespace unless given - outlierOptions() and mapNeighbourOptions() supply the defaults
    p.add_argument("--outliers", type=int, default=argparse.SUPPRESS, metavar="K", help=f"local outlier factors of the recovered noise, on the device (ganrev.knn): every row's K nearest rows (at most {OUTLIER_MAX_K}) in the table the clustering read, and from them the rows that lie in a sparser neighbourhood than their neighbours do; writes knn_idx, knn_dist [outlierRows x K], outlier_lof and outlier_lrd (.npy), with --render outliers_lof.png, the highest factor first; with --pca K2 --pcaSpace also the share of every row's neighbours in the attribute table that the whitened projection kept (kept_by_pca in summary.json)")
    p.add_argument("--outlierRows", type=int, default=argparse.SUPPRESS, metavar="M", help=f"with --outliers: the graph of the first M rows (default min(nbImages, 100000); at most {OUTLIER_MAX_ROWS}: every pair of rows is visited, the rows are independent draws, a prefix is a fair sample)")
    p.add_argument("--outlierMetric", choices=list(OUTLIER_METRICS), default=argparse.SUPPRESS, help="with --outliers / --mapNeighbours: the distance of the table's neighbour graph (default cosine, the search's geometry)")
    p.add_argument("--mapNeighbours", type=int, default=argparse.SUPPRESS, metavar="K", help=f"with --map: how many of every mapped row's K nearest rows in the table (at most {OUTLIER_MAX_K}) are still among its K nearest in the map (ganrev.knn); writes map_neighbours_kept.npy [mapRows] and the mean share into summary.json")
    # the density options: absent from the namespace unless given - densityOptions() supplies the defaults
    p.add_argument("--density", action="store_true", default=argparse.SUPPRESS, help="density-based clustering of the recovered noise, on the device (ganrev.density: DBSCAN), in the table the clustering read: it finds the number of clusters itself, follows groups of any shape and labels the rows that belong nowhere as noise; writes density_labels (int32, -1 = noise), density_core, density_count (.npy), with the quantile route density_kdist.npy, with --silhouette silhouette_density_{euclidean,cosine}.npy, with --render density_noise.png and density_%%02d.png, the largest clusters")
    p.add_argument("--densityMinPts", type=int, default=argparse.SUPPRESS, metavar="M", help="with --density: a row is core when its eps-neighbourhood holds M rows, itself included (default 10)")
    p.add_argument("--densityEps", type=float, default=argparse.SUPPRESS, metavar="E", help="with --density: the neighbourhood radius, a literal distance (not with --densityQuantile)")
    p.add_argument("--densityQuantile", type=float, default=argparse.SUPPRESS, metavar="Q", help=f"with --density: eps is the Q-quantile of the rows' distances to their (M - 1)-th nearest row (ganrev.knn), so that about that share of the rows is core (default 0.75; 2 <= M <= {DENSITY_MAX_MINPTS_BY_QUANTILE}; not with --densityEps)")
    p.add_argument("--densityRows", type=int, default=argparse.SUPPRESS, metavar="N", help=f"with --density: the first N rows are clustered (default min(nbImages, 100000); at most {DENSITY_MAX_ROWS}: every pair of rows is visited, the rows are independent draws, a prefix is a fair sample)")
    p.add_argument("--densityMetric", choices=list(DENSITY_METRICS), default=argparse.SUPPRESS, help="with --density: the distance (default cosine, the search's geometry)")
    # the hierarchy options: absent from the namespace unless given - hierarchyOptions() supplies the defaults
    p.add_argument("--hierarchy", action="store_true", default=argparse.SUPPRESS, help="clustering without an eps (ganrev.hierarchy: HDBSCAN), in the table the clustering read: the exact minimum spanning tree of the first rows under the mutual-reachability distance, built on the device, and the hierarchy read off it; writes hierarchy_mst_{u,v,w}, hierarchy_core, hierarchy_linkage (SciPy's format), hierarchy_labels (int32, -1 = noise), hierarchy_prob (.npy), with --silhouette silhouette_hierarchy_{euclidean,cosine}.npy, with --render hierarchy_noise.png and hierarchy_%%02d.png, the largest clusters")
    p.add_argument("--hierarchyMinSamples", type=int, default=argparse.SUPPRESS, metavar="S", help=f"with --hierarchy: a row's core distance is the distance to its (S - 1)-th nearest row - DBSCAN's minPts, the row itself included; 1: plain single linkage (default 10; at most {HIERARCHY_MAX_MINSAMPLES})")
    p.add_argument("--hierarchyMinClusterSize", type=int, default=argparse.SUPPRESS, metavar="M", help="with --hierarchy: a side of a split with fewer than M rows falls out of its cluster instead of founding one (default 25)")
    p.add_argument("--hierarchyRows", type=int, default=argparse.SUPPRESS, metavar="N", help=f"with --hierarchy: the first N rows are clustered (default min(nbImages, 100000); at most {HIERARCHY_MAX_ROWS}: every pair of rows is visited once per round)")
    p.add_argument("--hierarchyMetric", choices=list(HIERARCHY_METRICS), default=argparse.SUPPRESS, help="with --hierarchy: the distance (default cosine, the search's geometry)")
    p.add_argument("--hierarchyCut", type=float, default=argparse.SUPPRESS, metavar="E", help="with --hierarchy: also write hierarchy_cut_labels.npy, the tree cut at height E - DBSCAN*'s labels at eps = E, minPts = S")
    p.add_argument("--mixture", type=int, default=argparse.SUPPRESS, metavar="ITER", help="a diagonal Gaussian mixture of the recovered noise, on the device (ganrev.mixture): ITER EM iterations from the clustering's final centroids, --nbClusters components (at most 256), in the table the clustering read; writes mixture_weights, mixture_means, mixture_variances, mixture_loglik [ITER + 1], mixture_labels, mixture_posterior, mixture_row_loglik (.npy), with --render mixture_%%02d.png and mixture_outliers.png, with --needles needle_mixture.npy")
    # the clustering options (apply_r.lua:159-161 hard-codes 20, 15, 64 + 7): absent from the namespace unless given - clusterOptions() supplies the defaults
    p.add_argument("--nbClusters", type=int, default=argparse.SUPPRESS, help="clusters of the recovered noise (default 20, apply_r.lua:159; up to 4096, above 32 through gr_cluster_dev)")
    p.add_argument("--nbIterations", type=int, default=argparse.SUPPRESS, help="k-means iterations (default 15, apply_r.lua:160)")
    p.add_argument("--nbMaxPerCluster", type=int, default=argparse.SUPPRESS, help="rows kept per cluster, the most similar first (default 71 = 64 + 7, apply_r.lua:161; at most 128)")
    p.add_argument("--closest", action="store_true", default=argparse.SUPPRESS, help="a row joins its most similar centroid instead of the least similar one the reference keeps (apply_r.lua:207-214)")
    OPT = p.parse_args(argv)
    if OPT.resident and OPT.host:
        p.error("--resident applies to the device-resident pipeline: not with --host")
    if OPT.refine and OPT.host:
        p.error("--refine runs on the device-resident tables: not with --host")
    if OPT.refine < 0:
        p.error("--refine: a step count")
    if anomalyMetric(OPT) == "ssim":
        if OPT.host:
            p.error("--anomalyMetric ssim scores the device-resident tables: not with --host")
        if not (OPT.resident or OPT.render):
            p.error("--anomalyMetric ssim scores the tables where they lie: give --resident (or --render)")
        if OPT.synthetic:
            _, sh, sw, _ = (int(v) for v in OPT.synthetic.split("x"))
            if min(sh, sw) < 11 or max(sh, sw) > L.SSIM_MAX_HW:
                p.error(f"--anomalyMetric ssim: images of 11 .. {L.SSIM_MAX_HW} pixels a side")
    if OPT.needles < 0:
        p.error("--needles: a file count")
    nbAxes, pcaSpace = pcaOptions(OPT)
    if nbAxes < 0:
        p.error("--pca: an axis count")
    if pcaSpace and not nbAxes:
        p.error("--pcaSpace works on the projection: give --pca K")
    if nbAxes and OPT.synthetic and nbAxes > int(OPT.synthetic.split("x")[3]):
        p.error(f"--pca {nbAxes}: at most noiseDim = {OPT.synthetic.split('x')[3]} axes")
    for name in ("mapRows", "mapPerplexity", "mapIterations", "mapGrid"):
        if hasattr(OPT, name) and not getattr(OPT, "map", False):
            p.error(f"--{name} belongs to the map: give --map")
    mapped = mapOptions(OPT)
    if mapped:
        mapRows, mapPerplexity, mapIterations, mapGrid = mapped
        if mapRows > MAP_MAX_ROWS:
            p.error(f"--mapRows {mapRows}: at most {MAP_MAX_ROWS} rows (the joint matrix is mapRows x mapRows)")
        if not 4 <= mapRows <= OPT.nbImages:
            p.error(f"--mapRows {mapRows}: 4 to nbImages = {OPT.nbImages} rows")
        if not 1 <= mapPerplexity <= (mapRows - 1) / 3:
            p.error(f"--mapPerplexity {mapPerplexity:g}: 1 to (mapRows - 1) / 3 = {(mapRows - 1) / 3:g}")
        if mapIterations < 0:
            p.error("--mapIterations: an iteration count")
        if not 1 <= mapGrid <= 1024:
            p.error("--mapGrid: 1 to 1024 cells a side")
    nbClusters, nbIterations, nbMaxPerCluster, _ = clusterOptions(OPT)
    if not 1 <= nbClusters <= MAX_CLUSTERS:
        p.error(f"--nbClusters: 1 to {MAX_CLUSTERS}")
    if nbIterations < 0:
        p.error("--nbIterations: an iteration count")
    if not 1 <= nbMaxPerCluster <= MAX_PER_CLUSTER:
        p.error(f"--nbMaxPerCluster: 1 to {MAX_PER_CLUSTER}")
    mixIter = mixtureOptions(OPT)
    if mixIter is not None:
        if OPT.host:
            p.error("--mixture runs on the device-resident tables: not with --host")
        if mixIter < 0:
            p.error("--mixture: an iteration count")
        if nbClusters > MAX_COMPONENTS:
            p.error(f"--mixture: --nbClusters {nbClusters}: at most {MAX_COMPONENTS} components")
    if hasattr(OPT, "silhouetteSweep"):
        for v in OPT.silhouetteSweep.split(","):
            if not v.strip().isdigit():
                p.error(f"--silhouetteSweep {OPT.silhouetteSweep}: cluster counts separated by commas")
            if not 1 <= int(v) <= MAX_CLUSTERS:
                p.error(f"--silhouetteSweep: {int(v)}: 1 to {MAX_CLUSTERS} clusters")
    scored = silhouetteOptions(OPT)
    if hasattr(OPT, "silhouetteRows") and scored is None:
        p.error("--silhouetteRows belongs to the silhouette: give --silhouette or --silhouetteSweep")
    if scored is not None:
        if OPT.host:
            p.error("--silhouette and --silhouetteSweep run on the device-resident tables: not with --host")
        if scored[0] > SILHOUETTE_MAX_ROWS:
            p.error(f"--silhouetteRows {scored[0]}: at most {SILHOUETTE_MAX_ROWS} rows (every pair of rows is visited)")
        if not 2 <= scored[0] <= OPT.nbImages:
            p.error(f"--silhouetteRows {scored[0]}: 2 to nbImages = {OPT.nbImages} rows")
    graphed = outlierOptions(OPT)
    if hasattr(OPT, "outlierRows") and graphed is None:
        p.error("--outlierRows belongs to the outlier factors: give --outliers K")
    if hasattr(OPT, "outlierMetric") and graphed is None and not hasattr(OPT, "mapNeighbours"):
        p.error("--outlierMetric belongs to the neighbour graphs: give --outliers K or --mapNeighbours K")
    if graphed is not None:
        nbNear, nearRows, _ = graphed
        if OPT.host:
            p.error("--outliers runs on the device-resident tables: not with --host")
        if nearRows > OUTLIER_MAX_ROWS:
            p.error(f"--outlierRows {nearRows}: at most {OUTLIER_MAX_ROWS} rows (every pair of rows is visited)")
        if not 2 <= nearRows <= OPT.nbImages:
            p.error(f"--outlierRows {nearRows}: 2 to nbImages = {OPT.nbImages} rows")
        if not 1 <= nbNear <= OUTLIER_MAX_K:
            p.error(f"--outliers {nbNear}: 1 to {OUTLIER_MAX_K} neighbours")
        if nbNear > nearRows - 1:
            p.error(f"--outliers {nbNear}: at most rows - 1 = {nearRows - 1} neighbours (a row is not its own)")
    if hasattr(OPT, "mapNeighbours"):
        if not mapped:
            p.error("--mapNeighbours belongs to the map: give --map")
        if not 1 <= OPT.mapNeighbours <= OUTLIER_MAX_K:
            p.error(f"--mapNeighbours {OPT.mapNeighbours}: 1 to {OUTLIER_MAX_K} neighbours")
        if OPT.mapNeighbours > mapped[0] - 1:
            p.error(f"--mapNeighbours {OPT.mapNeighbours}: at most mapRows - 1 = {mapped[0] - 1} neighbours (a row is not its own)")
    dense = densityOptions(OPT)
    for name in DENSITY_OPTIONS:
        if hasattr(OPT, name) and dense is None:
            p.error(f"--{name} belongs to the density-based clustering: give --density")
    if dense is not None:
        minPts, eps, quantile, denseRows, _ = dense
        if OPT.host:
            p.error("--density runs on the device-resident tables: not with --host")
        if hasattr(OPT, "densityEps") and hasattr(OPT, "densityQuantile"):
            p.error("--densityEps and --densityQuantile: one of the two (a literal radius, or the quantile that chooses it)")
        if denseRows > DENSITY_MAX_ROWS:
            p.error(f"--densityRows {denseRows}: at most {DENSITY_MAX_ROWS} rows (every pair of rows is visited)")
        if not 2 <= denseRows <= OPT.nbImages:
            p.error(f"--densityRows {denseRows}: 2 to nbImages = {OPT.nbImages} rows")
        if not 1 <= minPts <= denseRows:
            p.error(f"--densityMinPts {minPts}: 1 to rows = {denseRows} (a neighbourhood holds no more)")
        if eps is not None and not (math.isfinite(eps) and eps >= 0):
            p.error(f"--densityEps {eps:g}: a finite distance, not below 0")
        if quantile is not None:
            if not 2 <= minPts <= DENSITY_MAX_MINPTS_BY_QUANTILE:
                p.error(f"--densityMinPts {minPts}: 2 to {DENSITY_MAX_MINPTS_BY_QUANTILE} with --densityQuantile (the distance to the (M - 1)-th neighbour): give --densityEps E")
            if not 0 <= quantile <= 1:
                p.error(f"--densityQuantile {quantile:g}: 0 to 1")
    tree = hierarchyOptions(OPT)
    for name in HIERARCHY_OPTIONS:
        if hasattr(OPT, name) and tree is None:
            p.error(f"--{name} belongs to the hierarchical clustering: give --hierarchy")
    if tree is not None:
        minSamples, minClusterSize, treeRows, _, height = tree
        if OPT.host:
            p.error("--hierarchy runs on the device-resident tables: not with --host")
        if treeRows > HIERARCHY_MAX_ROWS:
            p.error(f"--hierarchyRows {treeRows}: at most {HIERARCHY_MAX_ROWS} rows (every pair of rows is visited)")
        if not 2 <= treeRows <= OPT.nbImages:
            p.error(f"--hierarchyRows {treeRows}: 2 to nbImages = {OPT.nbImages} rows")
        if not 1 <= minSamples <= min(treeRows, HIERARCHY_MAX_MINSAMPLES):
            p.error(f"--hierarchyMinSamples {minSamples}: 1 to min(rows, {HIERARCHY_MAX_MINSAMPLES}) = {min(treeRows, HIERARCHY_MAX_MINSAMPLES)} (the row itself and its S - 1 nearest rows)")
        if not 2 <= minClusterSize <= treeRows:
            p.error(f"--hierarchyMinClusterSize {minClusterSize}: 2 to rows = {treeRows}")
        if height is not None and not (math.isfinite(height) and height >= 0):
            p.error(f"--hierarchyCut {height:g}: a finite distance, not below 0")
    if (OPT.needles or OPT.real) and OPT.dataset == "NONE":
        p.error("--needles and --real read their images from --dataset")
    if (OPT.needles or OPT.real) and OPT.host:
        p.error("--needles and --real run on the device-resident tables: not with --host")
    return OPT


def main(argv=None):
    OPT = parse(argv)
    try:
        return run(OPT)
    finally:
        if OPT.needles or OPT.real:                                           # --cacheDataset: the files' bytes go back with the run, however it ends
            from . import dataset
            dataset.uncache()


class Run:
    """What the steps of one run share.  run() calls the steps in the reference's order; a step reads what the steps before it left here and
    leaves its own part.  Device tables are allocated in `tables` and go with it."""

    def __init__(self, OPT, ctx, MODEL_G, MODEL_R, MODEL_R_FIXER, dims, nd, method, colorSpace):
        self.OPT, self.ctx, self.say = OPT, ctx, (lambda *a: None) if OPT.quiet else print
        self.MODEL_G, self.MODEL_R, self.MODEL_R_FIXER = MODEL_G, MODEL_R, MODEL_R_FIXER
        self.dims, self.nd, self.method, self.colorSpace, self.nbSteps = tuple(dims), nd, method, colorSpace, 16
        self.summary = dict(dims=list(dims), noiseDim=nd, noiseMethod=method, nbImages=OPT.nbImages, batchSize=OPT.batchSize,
                            path="host" if OPT.host else "device-resident" if OPT.resident else "device")
        self.tables = DeviceScope(ctx)                                        # owns every device table named below
        self.DATASET = None
        self.dn = self.di = self.da = self.df = None                          # the corpus on the device: noise, images, attributes, attributesFixer
        self.images = self.attributes = self.attributesFixer = None           # ... and on the host (the images: not with --resident)
        # the table the search by attributes, the clusters, the map and the mixture read - the attributes, with --pcaSpace their whitened
        # projection: a DeviceTensor on the device routes, the host array with --host; space_host: its copy for the steps that run on the host
        self.space = self.space_host = None
        self.spaceName = "pca_whitened" if pcaOptions(OPT)[1] else "attributes"
        self.by_attr = self.by_pix = self.map_cells = self.rendered = None
        self.pca = self.needle_rows = None                                    # what the steps before the mixture leave for it
        self.mixture_labels = None                                            # ... and the mixture for the silhouette
        self.density = None                                                   # ... and the density-based clustering (ganrev.density.Clustering)
        self.hierarchy = None                                                 # ... and the hierarchical one (ganrev.hierarchy.Clustering)

    def out(self, name):
        return os.path.join(self.OPT.writeTo, name)


def loadModels(OPT):
    """apply_r.lua:62-103 -> (G, R, R_fixer, dims, noiseDim, noiseMethod, colorSpace)"""
    if OPT.synthetic:
        from . import models, synth
        c, h, w, nd = (int(v) for v in OPT.synthetic.split("x"))
        dims, method, colorSpace = (c, h, w), "normal", "y" if c == 1 else "rgb"
        MODEL_G = models.create_G(dims, nd, seed=OPT.seed); synth.init_params(MODEL_G, OPT.seed)
        MODEL_R = models.create_R(dims, nd, method, False, seed=OPT.seed + 1); synth.init_params(MODEL_R, OPT.seed + 1)
        MODEL_R_FIXER = models.create_R(dims, nd, method, True, seed=OPT.seed + 2); synth.init_params(MODEL_R_FIXER, OPT.seed + 2)
        return MODEL_G, MODEL_R, MODEL_R_FIXER, dims, nd, method, colorSpace
    from . import t7
    ck = t7.load_checkpoint(OPT.G)                                            # apply_r.lua:62-69
    MODEL_G, o = ck["G"], ck.get("opt", {})
    nd, method, colorSpace = int(o.get("noiseDim", 32)), o.get("noiseMethod", "normal"), o.get("colorSpace", "rgb")
    dims = (1 if o.get("colorSpace", "rgb") == "y" else 3, int(o.get("height", 32)), int(o.get("width", 32)))
    return MODEL_G, t7.load_checkpoint(OPT.R)["R"], t7.load_checkpoint(OPT.R_fixer)["R"], dims, nd, method, colorSpace      # :92-94, :101-103


def checkOptions(S):
    """what parse() could not check without the models; before anything is allocated"""
    if pcaOptions(S.OPT)[0] > S.nd:
        raise L.GanrevError(f"--pca {pcaOptions(S.OPT)[0]}: at most noiseDim = {S.nd} axes")
    if anomalyMetric(S.OPT) == "ssim":
        L.ssim_check_args(min(1024, S.OPT.nbImages), S.dims[0], S.dims[1], S.dims[2], 11, 1.0)


def openDataset(S):
    """apply_r.lua:83-87: configured, and never read unless --needles / --real do (--cacheDataset then keeps the files on the GPU); they find
    out here, before anything else is allocated, whether it holds enough files"""
    OPT = S.OPT
    if not (OPT.needles or OPT.real):
        return scripts.open_dataset(OPT, S.colorSpace, S.dims[1], S.dims[2], reads=False)
    DATASET = scripts.open_dataset(OPT, S.colorSpace, S.dims[1], S.dims[2], ctx=S.ctx, reads=True)
    have = len(DATASET.paths if DATASET.paths is not None else DATASET.loadPaths())
    for count, what in ((OPT.nbImages if OPT.real else 0, "--nbImages"), (OPT.needles, "--needles")):
        if have < count:
            raise L.GanrevError(f"--dataset holds {have} matching files, {what} asks for {count}")
    return DATASET


def loadFirst(S, scope, count):
    """apply_r.lua:144 DATASET.loadImages(1, count), on the device; `scope` owns the table"""
    res = S.DATASET.loadImages(1, count, ctx=S.ctx)
    scope.adopt(res.images)
    if tuple(res.images.shape[1:]) != S.dims:
        raise L.GanrevError(f"--dataset images are {res.images.shape[1:]} in colour space {S.colorSpace}, the nets take {S.dims}")
    return res


def variationsStep(S):
    """apply_r.lua:110-138: one noise row, each component walked over its range in turn"""
    OPT, nd, nbSteps = S.OPT, S.nd, S.nbSteps
    S.say("Varying components...")
    steps = np.linspace(-1, 1, nbSteps) if S.method == "uniform" else np.linspace(-3, 3, nbSteps)
    noise1 = createNoiseInputs(1, nd, S.method, seed=OPT.seed)
    var_noise = np.repeat(noise1, nd * nbSteps, axis=0)
    for i in range(nd):
        var_noise[i * nbSteps:(i + 1) * nbSteps, i] = steps
    variations = forwardBatched(S.MODEL_G, var_noise, OPT.batchSize)
    np.save(S.out("variations.npy"), variations.reshape((nd, nbSteps) + S.dims))
    if OPT.render:
        with DeviceTensor(S.ctx, variations.shape) as dv:
            S.ctx.upload(variations, dv.ptr)
            render.variations_grid(dv, nbSteps, path=S.out("variations.png"))                                             # :137-138


def buildCorpus(S):
    """apply_r.lua:141-153: the images and what R and R_fixer recover from them, from one of three sources - G(noise) forwarded chunk by chunk
    through host tensors (--host: images, attributes, attributesFixer), G(noise) by gr_embed_dev, or the first --nbImages files of --dataset
    (--real, :144, commented out there); the last two leave di, da, df on the device"""
    OPT, N, adopt = S.OPT, S.OPT.nbImages, S.tables.adopt
    S.say("Generating images, converting images to attributes...")
    if OPT.real:
        S.say("Loading the first %d images of --dataset..." % N)
        S.di = loadFirst(S, S.tables, N).images
        S.da, S.df = (adopt(t) for t in embedImagesDev([S.MODEL_R, S.MODEL_R_FIXER], S.di, OPT.batchSize))                # :152-153
        S.summary["corpus"] = "dataset"
        return
    noise = createNoiseInputsDev(S.ctx, N, S.nd, S.method, seed=OPT.seed + 1)      # utils/nn_utils.lua:39-51, drawn on the device (both paths: same noise)
    if OPT.host:
        with noise:
            noise = noise.numpy()
        S.images, S.attributes, S.attributesFixer = embed(S.MODEL_G, S.MODEL_R, noise, OPT.batchSize, S.MODEL_R_FIXER)
    else:
        S.dn = adopt(noise)
        S.di, S.da, S.df = (adopt(t) for t in embed_dev(S.MODEL_G, S.MODEL_R, S.dn, OPT.batchSize, S.MODEL_R_FIXER, keep_images=True, dims=S.dims))


def refineRows(S, images_t, z_t):
    """ganrev.refine over one image table and its recovered noise, in place -> the summary's entry"""
    from . import device, refine
    OPT = S.OPT
    with contextlib.closing(device.DeviceModel(S.ctx, S.MODEL_G)) as dmG:
        first, best = refine.refineNoise(S.ctx, dmG, images_t.ptr, z_t.ptr, z_t.shape[0], OPT.refine, OPT.batchSize, lr=OPT.refine_lr,
                                         clamp=1.0 if S.method == "uniform" else 0.0)
    return dict(steps=OPT.refine, lr=OPT.refine_lr, loss_before_mean=float(first.mean(dtype=np.float64)),
                loss_after_mean=float(best.mean(dtype=np.float64)), rows_improved=int((best < first).sum()))


def refineStep(S):
    """--refine STEPS.  `attributes` only: pulling attributesFixer back to the unfixed image would undo the fix, and the anomaly score needs the
    unrefined reconstruction.  The steps after this one read the refined table."""
    OPT = S.OPT
    S.say("Refining the recovered noise through G...")
    S.summary["refine"] = refineRows(S, S.di, S.da)
    if OPT.render:
        k = min(52, OPT.nbImages)
        with forwardBatchedDev(S.MODEL_G, S.da.rows(0, k), OPT.batchSize) as again:
            render.fixed_pairs_grid(S.di, again, k, S.colorSpace, path=S.out("refined_pairs.png"))                        # image next to G(refined z)


def pcaStep(S):
    """--pca K over the attribute table, where it lies -> with --pcaSpace the whitened projection, lying where that table lies (a DeviceTensor,
    on the host with --host); else None"""
    from . import pca as P
    OPT, ctx, out, nbSteps = S.OPT, S.ctx, S.out, S.nbSteps
    nbAxes, pcaSpace = pcaOptions(OPT)
    S.say("Principal axes of the recovered noise...")
    axes, coords, white = principalAxesOfTable(ctx, S.attributes if OPT.host else S.da, nbAxes, pcaSpace)
    if white is not None:
        S.tables.adopt(white)
    with contextlib.closing(axes):
        if mixtureOptions(OPT) is not None:                                   # the mixture reuses the covariance diagonal, and projects the needles
            S.pca = (axes.mean, axes.axes, axes.eigenvalues, np.diag(axes.covariance()).copy())
        np.save(out("pca_mean.npy"), axes.mean); np.save(out("pca_eigenvalues.npy"), axes.eigenvalues)
        np.save(out("pca_axes.npy"), axes.axes[:nbAxes]); np.save(out("pca_projection.npy"), coords)
        S.summary["pca"] = dict(k=nbAxes, explained=[float(v) for v in axes.explained[:nbAxes]], sweeps=axes.sweeps, converged=axes.converged, space=S.spaceName)
        if OPT.render:                                                        # variations.png's conventions, along the axes instead of the coordinates
            with DeviceTensor(ctx, (nbAxes * nbSteps, S.nd)) as dz:
                ctx.upload(P.axisVariations(axes, nbAxes, nbSteps, S.method), dz.ptr)
                with forwardBatchedDev(S.MODEL_G, dz, OPT.batchSize) as walked:
                    render.variations_grid(walked, nbSteps, path=out("variations_pca.png"))
    if white is None or not OPT.host:
        return white
    host = white.numpy()                                                      # on the host like the table it stands for
    S.tables.release(white)
    return host


def mapStep(S):
    """--map over the table the search and the clusters read (the host route uploads the table it has, as --pca does)"""
    S.say("Mapping the recovered noise...")
    y, (kl_iterations, kl), S.map_cells, entry = mapOfTable(S.ctx, S.space, *mapOptions(S.OPT))
    np.save(S.out("map_y.npy"), y); np.save(S.out("map_kl.npy"), np.stack([kl_iterations.astype(np.float64), kl], axis=1)); np.save(S.out("map_cells.npy"), S.map_cells)
    S.summary["map"] = dict(entry, space=S.spaceName)
    if mapNeighbourOptions(S.OPT):
        K, metric = mapNeighbourOptions(S.OPT)
        kept, share = mapNeighboursKept(S.ctx, S.space, y, len(y), K, metric)
        np.save(S.out("map_neighbours_kept.npy"), kept)
        S.summary["map"]["neighbours"] = dict(k=K, metric=metric, mean_share_kept=share)
        S.say("<apply_r> the map keeps %.1f %% of every row's %d nearest rows (%s distance in %s)" % (100 * share, K, metric, S.spaceName))


def needlesInSpace(S, na):
    """the needles' rows in the table the mixture is fitted in"""
    nbAxes, pcaSpace = pcaOptions(S.OPT)
    if not pcaSpace:
        return na.numpy()
    with DeviceScope(S.ctx) as own:
        mean, axes, lam = (own.upload(np.ascontiguousarray(a)) for a in S.pca[:3])
        white = own.tensor((na.shape[0], nbAxes))
        S.ctx.pca_project_dev(na.ptr, na.shape[0], S.nd, mean, axes, lam, nbAxes, True, white.ptr)
        return white.numpy()


def needlesStep(S):
    """--needles N, search by example: the needles are images from outside the corpus - the dataset's first files - embedded like the corpus
    (R, then the same refinement against themselves) and searched in the tables where they lie"""
    OPT, out = S.OPT, S.out
    S.say("Searching the corpus for the first %d images of --dataset..." % OPT.needles)
    with DeviceScope(S.ctx) as own:                                           # the needles' tables go with the step
        nl = loadFirst(S, own, OPT.needles)
        ni = nl.images
        (na,) = (own.adopt(t) for t in embedImagesDev([S.MODEL_R], ni, OPT.batchSize))
        S.summary["needles"] = dict(count=OPT.needles, files=[os.path.basename(f) for f in nl.paths])
        if OPT.refine:
            S.summary["needles"]["refine"] = refineRows(S, ni, na)
        if mixtureOptions(OPT) is not None:
            S.needle_rows = needlesInSpace(S, na)
        nb_attr, nb_pix = searchByExample(100, S.da, na, S.di, ni)
        np.save(out("needle_by_attributes.npy"), nb_attr); np.save(out("needle_by_pixels.npy"), nb_pix); np.save(out("needle_attributes.npy"), na.numpy())
        if OPT.render:
            for i in range(OPT.needles):
                render.similar_example_grid(ni, i, S.di, nb_attr[i], S.colorSpace, path=out("needle_attributes_%02d.png" % (i + 1)))
                render.similar_example_grid(ni, i, S.di, nb_pix[i], S.colorSpace, path=out("needle_pixelwise_%02d.png" % (i + 1)))


def tablesForAnalysis(S):
    """Every table where the rest of the run reads it.  --host: with --render the same pictures come from uploaded tables.  The device routes:
    the small tables come to the host for the files, the noise has done its work, and unless the analysis runs on the device (--resident,
    --render) the images come too and every device table goes here, before the host-side analysis, not at the end of it."""
    OPT, T = S.OPT, S.tables
    if OPT.host:
        S.space_host = S.space
        if OPT.render:
            S.di, S.df = T.tensor(S.images.shape), T.tensor(S.attributesFixer.shape)
            S.ctx.upload(S.images, S.di.ptr); S.ctx.upload(S.attributesFixer, S.df.ptr)
        return
    S.attributes, S.attributesFixer = S.da.numpy(), S.df.numpy()
    S.space_host = S.attributes if S.space is S.da else S.space.numpy()
    T.release(S.dn)
    if not OPT.resident:
        S.images = S.di.numpy()
        if not OPT.render:
            T.close()


def mapPicture(S):
    """map.png, the faces where they land: one grid over the map's cells, from the image table where it lies; each tile's ring takes the colour
    of its row's cluster - the assignment of the clustering step (gr_cosine_assign on its final centroids) repeated for the rows shown"""
    nbClusters, _, _, closest = clusterOptions(S.OPT)
    shown = S.map_cells[S.map_cells >= 0]
    labels = None
    if nbClusters <= NARROW_MAX_CLUSTERS:                                     # (the palette has 12 colours: finer clusterings keep plain rings)
        labels = np.full(S.OPT.nbImages, -1, np.int64)
        labels[shown] = S.ctx.cosine_assign(S.space_host[shown], S.rendered["clusters"][0], take_min=not closest)[0]
    render.map_grid(S.di, S.map_cells, S.colorSpace, labels=labels, path=S.out("map.png"))


def mixtureStep(S, table, centroids, images=None):
    """--mixture ITER, after the clustering, in the table it read"""
    OPT, out, mixIter = S.OPT, S.out, mixtureOptions(S.OPT)
    S.say("Fitting a Gaussian mixture to the recovered noise...")
    reuse = S.pca[3] if S.pca is not None and not pcaOptions(OPT)[1] else None    # (the whitened projection is another table: its variances are its own)
    fitted, (labels, post, rowll), needles = mixtureOfTable(S.ctx, table, centroids, mixIter, reuse, S.needle_rows)
    S.mixture_labels = labels
    for name, a in (("weights", fitted.weights), ("means", fitted.means), ("variances", fitted.variances), ("loglik", fitted.loglik),
                    ("labels", labels), ("posterior", post), ("row_loglik", rowll)):
        np.save(out("mixture_%s.npy" % name), a)
    S.summary["mixture"] = dict(iterations=mixIter, k=fitted.k, var_floor=fitted.var_floor, loglik=[float(v) for v in fitted.loglik],
                                weights=[float(v) for v in fitted.weights], sizes=[int(v) for v in np.bincount(labels, minlength=fitted.k)],
                                row_loglik_min=float(rowll.min()), row_loglik_median=float(np.median(rowll)), space=S.spaceName)
    if needles is not None:
        np.save(out("needle_mixture.npy"), np.stack([needles[0].astype(np.float64), needles[1].astype(np.float64), needles[2].astype(np.float64)], axis=1))
    if OPT.render and images is not None:
        from . import mixture as MX
        for j, cl in enumerate(MX.members(S.ctx, labels, post, fitted.k, clusterOptions(OPT)[2])):
            if cl:                                                            # the average face first, then the rows of highest posterior
                render.cluster_grid(images, [r for r, _ in cl], S.colorSpace, path=out("mixture_%02d.png" % (j + 1)))
        shown = min(512 + 16, OPT.nbImages, 1024)                             # as many rows as anomalies.png shows
        worst = np.argsort(rowll, kind="stable")[:shown]                      # lowest row log-likelihood first
        render.grid(images, worst, int(math.floor(math.sqrt(shown))), S.colorSpace, path=out("mixture_outliers.png"))


def silhouetteStep(S, table, centroids, images=None):
    """--silhouette and --silhouetteSweep, after the clustering (and the mixture), in the table they read.  The clustering's labels are the cosine
    assignment to its final centroids (apply_r.lua:205-217): clusterTableDev from those centroids with no k-means iteration hands them back."""
    OPT, ctx, out = S.OPT, S.ctx, S.out
    rows, sweep = silhouetteOptions(OPT)
    k, nbIterations, m, closest = clusterOptions(OPT)
    with deviceTable(ctx, table) as (ptr, N, d):
        if getattr(OPT, "silhouette", False):
            S.say("Scoring the clusterings (silhouette)...")
            got = []
            clusterTableDev(ctx, ptr, N, d, k, 0, m, centroids, closest, labels_into=got)
            np.save(out("silhouette_clusters_labels.npy"), got[0])
            entry = dict(rows=rows, space=S.spaceName)
            scored = [("clusters", got[0], k), ("mixture", S.mixture_labels, k)]
            if S.density is not None:
                if 1 <= S.density.clusters <= MAX_CLUSTERS:               # (rows past --densityRows are nobody's member, like the noise)
                    padded = np.full(N, -1, np.int32)
                    padded[:S.density.n] = S.density.labels
                    scored.append(("density", padded, S.density.clusters))
                else:
                    entry["density"] = dict(skipped="%d clusters: the silhouette scores 1 to %d" % (S.density.clusters, MAX_CLUSTERS))
            if S.hierarchy is not None:
                if 1 <= S.hierarchy.clusters <= MAX_CLUSTERS:             # (rows past --hierarchyRows are nobody's member, like the noise)
                    padded = np.full(N, -1, np.int32)
                    padded[:S.hierarchy.n] = S.hierarchy.labels
                    scored.append(("hierarchy", padded, S.hierarchy.clusters))
                else:
                    entry["hierarchy"] = dict(skipped="%d clusters: the silhouette scores 1 to %d" % (S.hierarchy.clusters, MAX_CLUSTERS))
            for name, labels, nb in scored:
                if labels is None:
                    continue
                entry[name] = {}
                for metric, sc in silhouetteOfLabels(ctx, (ptr, N, d), rows, labels, nb).items():
                    np.save(out("silhouette_%s_%s.npy" % (name, metric)), sc.values)
                    entry[name][metric] = sc.summary()
                    S.say("<apply_r> silhouette of the %s, %s distance, %d rows in %s: mean %.4f" % (name, metric, rows, S.spaceName, sc.mean))
            S.summary["silhouette"] = entry
        if sweep:
            S.say("Sweeping the number of clusters (silhouette)...")
            found = []
            for K in sweep:
                got = []
                clusterTableDev(ctx, ptr, N, d, K, nbIterations, m, initialCentroids(K, d, OPT.seed), closest, labels_into=got)
                scores = silhouetteOfLabels(ctx, (ptr, N, d), rows, got[0], K)
                found.append(dict(K=K, mean_euclidean=scores["euclidean"].mean, mean_cosine=scores["cosine"].mean,
                                  empty_clusters=int((scores["cosine"].sizes == 0).sum())))
                S.say("<apply_r> silhouette sweep: K %d: mean %.4f (euclidean), %.4f (cosine), %d empty clusters"
                      % (K, found[-1]["mean_euclidean"], found[-1]["mean_cosine"], found[-1]["empty_clusters"]))
            json.dump(dict(rows=rows, space=S.spaceName, nbIterations=nbIterations, closest=closest, seed=OPT.seed, sweep=found),
                      open(out("silhouette_sweep.json"), "w"), indent=1)


def outlierStep(S, table, centroids, images=None):
    """--outliers K, after the clustering, in the table it read: the neighbour graph of the first rows is built once, stays on the device and is
    scored there.  With --pcaSpace the attribute table's graph of the same rows is built beside it: the share of its neighbours that the
    whitened projection kept."""
    from . import knn as KNN
    OPT, ctx, out = S.OPT, S.ctx, S.out
    k, rows, metric = outlierOptions(OPT)
    S.say("Neighbour graph and local outlier factors...")
    with KNN.graph(ctx, table, k, metric, rows=rows, keep=True) as g:
        lof, lrd = KNN.lof(ctx, g)
        host = g.numpy()
        entry = dict(k=k, rows=rows, metric=metric, space=S.spaceName, lof_max=float(lof.max()), lof_median=float(np.median(lof)),
                     lof_p99=float(np.percentile(lof, 99)))
        if pcaOptions(OPT)[1]:
            attributes = S.da if S.da is not None and S.da.ptr is not None else S.attributes
            with KNN.graph(ctx, attributes, k, metric, rows=rows, keep=True) as before:
                entry["kept_by_pca"] = KNN.overlap(ctx, before, g)[1]
    np.save(out("knn_idx.npy"), host.idx); np.save(out("knn_dist.npy"), host.dist)
    np.save(out("outlier_lof.npy"), lof); np.save(out("outlier_lrd.npy"), lrd)
    S.summary["outliers"] = entry
    S.say("<apply_r> local outlier factor, %d neighbours, %s distance, %d rows in %s: median %.4f, 99th percentile %.4f, max %.4f"
          % (k, metric, rows, S.spaceName, entry["lof_median"], entry["lof_p99"], entry["lof_max"]))
    if OPT.render and images is not None:
        shown = min(512 + 16, OPT.nbImages, 1024, rows)                       # as many rows as mixture_outliers.png shows
        worst = np.argsort(-lof, kind="stable")[:shown]                       # highest factor first
        render.grid(images, worst, int(math.floor(math.sqrt(shown))), S.colorSpace, path=out("outliers_lof.png"))


def densityStep(S, table, centroids, images=None):
    """--density, after the clustering, in the table it read: the eps-graph of the first rows is built once, stays on the device and is labelled
    there.  Without --densityEps the radius comes from the neighbour graph of the same rows (the k-distance rule)."""
    from . import density as DN
    OPT, ctx, out = S.OPT, S.ctx, S.out
    minPts, eps, quantile, rows, metric = densityOptions(OPT)
    S.say("Density-based clustering (DBSCAN)...")
    entry = dict(minPts=minPts, metric=metric, rows=rows, space=S.spaceName)
    if eps is None:
        eps, kdist = DN.epsFromNeighbours(ctx, table, minPts, quantile, metric, rows=rows)
        np.save(out("density_kdist.npy"), kdist)
        entry["quantile"] = quantile
    found = S.density = DN.cluster(ctx, table, eps, minPts, metric, rows=rows)
    np.save(out("density_labels.npy"), found.labels); np.save(out("density_core.npy"), found.core.astype(np.int32))
    np.save(out("density_count.npy"), found.count)
    largest = np.argsort(-found.sizes, kind="stable")[:20]                    # largest first, the lower number among equals
    entry.update(eps=float(eps), clusters=found.clusters, core=int(found.core.sum()), border=found.border, noise=found.noise,
                 sizes=[int(found.sizes[c]) for c in largest])
    S.summary["density"] = entry
    S.say("<apply_r> DBSCAN, eps %.6g, minPts %d, %s distance, %d rows in %s: %d clusters, %d core, %d border and %d noise rows"
          % (eps, minPts, metric, rows, S.spaceName, found.clusters, entry["core"], found.border, found.noise))
    if OPT.render and images is not None:
        noise = np.nonzero(found.labels < 0)[0][:min(512 + 16, OPT.nbImages, 1024)]       # the first noise rows, as many as anomalies.png shows
        if len(noise):
            render.grid(images, noise, max(int(math.floor(math.sqrt(len(noise)))), 1), S.colorSpace, path=out("density_noise.png"))
        for j, c in enumerate(largest):
            members = np.nonzero(found.labels == c)[0][:64 + 8]                # lowest rows first
            render.grid(images, members, max(int(math.floor(math.sqrt(len(members)))), 1), S.colorSpace, path=out("density_%02d.png" % (j + 1)))


def hierarchyStep(S, table, centroids, images=None):
    """--hierarchy, after the clustering, in the table it read: the minimum spanning tree of the first rows under the mutual-reachability distance
    is built on the device (the core distances from the neighbour graph of the same rows); the linkage matrix, HDBSCAN's labels and, with
    --hierarchyCut, DBSCAN*'s labels at that height are read off its edges on the host."""
    from . import hierarchy as HR
    OPT, ctx, out = S.OPT, S.ctx, S.out
    minSamples, minClusterSize, rows, metric, height = hierarchyOptions(OPT)
    S.say("Hierarchical density-based clustering (HDBSCAN)...")
    found = S.hierarchy = HR.cluster(ctx, table, minSamples, minClusterSize, metric, rows=rows)
    tree = found.tree
    np.save(out("hierarchy_mst_u.npy"), tree.u); np.save(out("hierarchy_mst_v.npy"), tree.v); np.save(out("hierarchy_mst_w.npy"), tree.w)
    np.save(out("hierarchy_core.npy"), tree.core if tree.core is not None else np.zeros(rows))     # minSamples 1: every row is core at any height
    np.save(out("hierarchy_linkage.npy"), HR.linkage(tree))
    np.save(out("hierarchy_labels.npy"), found.labels); np.save(out("hierarchy_prob.npy"), found.prob)
    largest = np.argsort(-found.sizes, kind="stable")[:20]                    # largest first, the lower number among equals
    entry = dict(minSamples=minSamples, minClusterSize=minClusterSize, metric=metric, rows=rows, space=S.spaceName, rounds=tree.rounds,
                 clusters=found.clusters, noise=found.noise, sizes=[int(found.sizes[c]) for c in largest],
                 weight_quartiles=[float(q) for q in np.quantile(tree.w, [0.0, 0.25, 0.5, 0.75, 1.0])])
    if height is not None:
        at = HR.cut(tree, height)
        np.save(out("hierarchy_cut_labels.npy"), at)
        entry["cut"] = dict(height=height, clusters=int(at.max()) + 1, noise=int((at < 0).sum()))
    S.summary["hierarchy"] = entry
    S.say("<apply_r> HDBSCAN, minSamples %d, minClusterSize %d, %s distance, %d rows in %s: %d Boruvka rounds, %d clusters and %d noise rows"
          % (minSamples, minClusterSize, metric, rows, S.spaceName, tree.rounds, found.clusters, found.noise))
    if OPT.render and images is not None:
        noise = np.nonzero(found.labels < 0)[0][:min(512 + 16, OPT.nbImages, 1024)]       # the first noise rows, as many as anomalies.png shows
        if len(noise):
            render.grid(images, noise, max(int(math.floor(math.sqrt(len(noise)))), 1), S.colorSpace, path=out("hierarchy_noise.png"))
        for j, c in enumerate(largest):
            members = np.nonzero(found.labels == c)[0][:64 + 8]                # lowest rows first
            render.grid(images, members, max(int(math.floor(math.sqrt(len(members)))), 1), S.colorSpace, path=out("hierarchy_%02d.png" % (j + 1)))


def afterClustering(S):
    """the steps that follow the clustering in its table - the mixture, the density-based clustering, the hierarchical one, then the silhouette,
    which scores the labels of all three too, then the outlier factors - as one call (table, centroids, images=None); None when the run asks for
    none of them"""
    steps = ([mixtureStep] * (mixtureOptions(S.OPT) is not None) + [densityStep] * (densityOptions(S.OPT) is not None)
             + [hierarchyStep] * (hierarchyOptions(S.OPT) is not None)
             + [silhouetteStep] * (silhouetteOptions(S.OPT) is not None) + [outlierStep] * (outlierOptions(S.OPT) is not None))
    if not steps:
        return None

    def run_steps(table, centroids, images=None):
        for step in steps:
            step(S, table, centroids, images)
    return run_steps


# apply_r.lua:25-193 main(): the whole analysis as one run.  What the reference computes is written as arrays (.npy) and one
# summary.json under --writeTo; with --render the pictures it saves (apply_r.lua:137-138, 245-258, 283-298, 325-351, 374-389) are written
# beside them as PNG, under the reference's names: variations, cluster_%02d, similar_attributes_%02d, similar_pixelwise_%02d, fixed_pairs,
# fixed_images_528[_unfixed], anomalies (the counts clamp to --nbImages).  G / R / R_fixer come from Torch7 checkpoints (ganrev.t7: train.lua:256, train_r.lua:234) or, with
# --synthetic, from random-initialised nets of the requested shape (a smoke run: no trained checkpoint exists in this repository).
def run(OPT):
    ctx = L.Context(OPT.gpu) if OPT.gpu != int(os.environ.get("LOCAL_RANK", "0")) else L.default_context()
    ctx.set_conv_mode(OPT.conv_mode)
    S = Run(OPT, ctx, *loadModels(OPT))                                       # apply_r.lua:62-103
    checkOptions(S)
    S.DATASET = openDataset(S)                                                # :83-87
    for m in (S.MODEL_G, S.MODEL_R, S.MODEL_R_FIXER):
        m._ctx = ctx
        m.evaluate()
    S.MODEL_R_FIXER.manualSeed(OPT.seed)
    os.makedirs(OPT.writeTo, exist_ok=True)
    out, say, summary, N = S.out, S.say, S.summary, OPT.nbImages
    after = afterClustering(S)
    mixture = {} if after is None else dict(mixture=after)                    # analyseDev calls it while the tables are where they are
    with S.tables:
        variationsStep(S)                                                     # :110-138
        t0 = time.perf_counter()
        buildCorpus(S)                                                        # :141-153
        if OPT.refine:
            refineStep(S)
        white = pcaStep(S) if pcaOptions(OPT)[0] else None                    # after the refinement, on the table it left, like the search and the clusters
        S.space = white if white is not None else S.attributes if OPT.host else S.da     # --pcaSpace: d = K
        if mapOptions(OPT):
            mapStep(S)
        if N >= 500:                                                          # :170-172, on the tables where they were written
            S.by_attr, S.by_pix = createSimilaritySearch(5, 100, S.images, S.space) if OPT.host else createSimilaritySearchDev(5, 100, S.space, S.di)
        if OPT.needles:
            needlesStep(S)
        tablesForAnalysis(S)
        ctx.synchronize()
        summary["embed_and_search_seconds"] = round(time.perf_counter() - t0, 4)
        if OPT.render:
            say("Rendering...")
            S.rendered = renderAnalysis(OPT, out, S.colorSpace, S.MODEL_G, S.di, S.space, S.df, S.by_attr, S.by_pix, **mixture)
        elif OPT.resident:
            say("Analysing on the device...")
            S.rendered = analyseDev(OPT, S.MODEL_G, S.di, S.space, S.df, **mixture)
        if S.map_cells is not None and OPT.render:
            mapPicture(S)
    rendered = S.rendered                                                     # the device tables are gone: the rest is host arrays and files
    np.save(out("attributes.npy"), S.attributes); np.save(out("attributes_fixer.npy"), S.attributesFixer)
    if S.by_attr is not None:
        np.save(out("similar_by_attributes.npy"), S.by_attr); np.save(out("similar_by_pixels.npy"), S.by_pix)

    say("Clustering...")                                                      # :158-162
    centroids, counts, clusters, faces = rendered["clusters"] if rendered else createClusterImages(*clusterOptions(OPT)[:3], S.images, S.space_host, seed=OPT.seed, closest=clusterOptions(OPT)[3])     # (20, 15, 64 + 7 unless asked otherwise)
    np.save(out("cluster_centroids.npy"), centroids); np.save(out("cluster_average_faces.npy"), np.stack(faces))
    summary["cluster_sizes"] = [len(c) for c in clusters]; summary["cluster_total_counts"] = [float(v) for v in counts]
    summary.update(zip(("nbClusters", "nbIterations", "nbMaxPerCluster", "closest"), clusterOptions(OPT)))
    if after is not None and not rendered:                                    # neither --resident nor --render: the host copy of the table is uploaded
        after(S.space_host, centroids)

    say("Fixing faces...")                                                    # :178-181
    nbFixed = min(512 + 16, N)
    np.save(out("fixed_faces.npy"), rendered["fixed"] if rendered else fixFaces(nbFixed, S.MODEL_G, S.attributesFixer, OPT.batchSize))

    say("Detecting anomalies...")                                             # :186-191
    nbCalc = min(1024, N)
    dist, below, is_anom = rendered["anomalies"] if rendered else detectAnomalies(nbCalc, 0.15, S.images, S.MODEL_G, S.attributesFixer, OPT.batchSize)
    if anomalyMetric(OPT) == "ssim":                                          # (parse: only where analyseDev ran) the score is the SSIM, the distances beside it
        np.save(out("anomaly_ssim.npy"), dist)
        dist = rendered["distances"]
    np.save(out("anomaly_distances.npy"), dist)
    summary.update(anomaly_below=float(below), anomalies=int(is_anom.sum()))
    if hasattr(OPT, "anomalyMetric"):
        summary["anomaly_metric"] = OPT.anomalyMetric
    json.dump(summary, open(out("summary.json"), "w"), indent=1)
    say("<apply_r> results in", OPT.writeTo, summary)
    return summary


if __name__ == "__main__":
    main()
