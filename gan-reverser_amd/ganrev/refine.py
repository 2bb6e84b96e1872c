"""Refinement of recovered noise through G (no counterpart in the reference: R's one-shot estimate is all apply_r.lua has).

  refineNoise      z0 = R(x)  ->  argmin_z  mean((G(z) - x)^2)  per image, by optim.adam on z, on the device

G runs in evaluate() mode, where no two images of a batch are coupled (BatchNorm is an affine map of the running statistics), so every row
is an optimisation problem of its own: the criterion is the per-row MSE (gr_mse_rows_dev), the gradient with respect to z comes from the
input-only backward (gr_net_backward_input_dev: nn.Module:updateGradInput in evaluate()), and the step is optim.adam row by row
(gr_adam_rows_step_dev), which also keeps the best z each row has seen - a row never ends worse than it started.
"""
import numpy as np

from . import _lib as L
from . import device


def refineNoise(ctx, G, images_dev, z_dev, N, steps, batchSize, lr=0.01, clamp=0.0):
    """G: a device.DeviceModel.  images_dev [N x C x H x W] and z_dev [N x nd] are device tables; z_dev is overwritten with the best z of
    every row.  Chunks of batchSize rows; per chunk `steps` times (forward, per-row MSE, input-only backward, Adam), then one last look
    (forward, MSE, best-keeping without an update).  clamp > 0 keeps z in [-clamp, clamp] (noiseMethod "uniform": R ends in a Tanh).
    Everything is enqueued on the context's stream; the host waits once, for the two loss vectors.  The parts' mode, input-gradient flag
    and Philox forward counter are what they were when the call returns.  -> (loss_first[N], loss_best[N]) float32: the per-row MSE at
    z0 and the lowest one seen."""
    N, steps, batchSize = int(N), int(steps), int(batchSize)
    if N <= 0 or steps < 0 or batchSize <= 0:
        raise L.GanrevError(f"refineNoise: N {N}, steps {steps}, batchSize {batchSize}")
    nd, n = G.in_features(G.model), G.out_features(G.model)
    hyper = L.AdamHyper(lr=lr)
    mem = device.Buffers(ctx)
    saved = [(net, net.forward_counter(), net.training, net.input_grad) for net in G.nets]
    try:
        for net in G.nets:
            net.set_training(False)
            net.set_input_grad(True)
        bs = min(batchSize, N)
        g, loss = mem.malloc(4 * bs * n), mem.malloc(4 * bs)
        first, best_z = mem.malloc(4 * N), mem.malloc(4 * N * nd)
        best = ctx.upload(np.full(N, np.inf, np.float32), mem.malloc(4 * N))          # (uploads wait on an empty stream: before any work)
        m, v = (ctx.upload(np.zeros(N * nd, np.float32), mem.malloc(4 * N * nd)) for _ in range(2))
        for lo in range(0, N, batchSize):
            b = min(batchSize, N - lo)
            z, x, zo = z_dev + 4 * lo * nd, images_dev + 4 * lo * n, 4 * lo * nd
            for t in range(1, steps + 2):
                last = t == steps + 1                                                   # the last look: no gradient, no update
                out = G.forward(z, b)
                ctx.mse_rows_dev(out, x, b, n, loss, None if last else g)
                if t == 1:
                    ctx.copy2d(first + 4 * lo, b, loss, b, 1, b)
                gz = None if last else G.backward(g, b, True, params=False)
                ctx.adam_rows_step_dev(z, gz, m + zo, v + zo, b, nd, hyper, t, loss, best + 4 * lo, best_z + zo, clamp=clamp, update=not last)
        ctx.copy2d(z_dev, nd, best_z, nd, N, nd)
        return ctx.download(first, (N,)), ctx.download(best, (N,))
    finally:
        for net, counter, training, flag in saved:
            net.set_input_grad(flag)
            net.set_training(training)
            net.set_forward_counter(counter)
        mem.close()
