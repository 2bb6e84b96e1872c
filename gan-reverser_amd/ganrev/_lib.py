"""ctypes binding of libganrev.so (include/ganrev.h) — the only way this package computes anything.

There is NO CPU fallback: if the HIP library is missing, or no gfx950 GPU is visible, every entry point raises
GanrevError.  (The CPU oracle under /oracle is test infrastructure and is never imported from here.)

PyTorch is imported first, when present, only so that this process ends up with ONE HIP runtime / ONE RCCL
(torch ships its own libamdhip64.so.7 / librccl.so.1 with the same sonames as /opt/rocm's): plumbing, not compute.
"""
import ctypes as C
import os

import numpy as np

try:  # noqa: SIM105  (settle which libamdhip64 / librccl the process binds before loading ours)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional plumbing
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GANREV_LIB") or os.path.join(_HERE, "libganrev.so")   # GANREV_LIB: A/B-testing hook


class GanrevError(RuntimeError):
    pass


GR_OK = 0
STATUS = {0: "GR_OK", -1: "GR_ERR_INVALID", -2: "GR_ERR_UNSUPPORTED", -3: "GR_ERR_HIP", -4: "GR_ERR_NO_DEVICE",
          -5: "GR_ERR_COMM", -6: "GR_ERR_STATE"}

# layer kinds (shared numeric values with the oracle's go_layer)
CONV3, BN, ELU, RELU, LEAKYRELU, SIGMOID, TANH, DROPOUT, SPATIAL_DROPOUT, MAXPOOL2, UPSAMPLE2, VIEW, LINEAR, FULLCONV3 = range(1, 15)
CONVK, PRELU = 15, 16       # the D network's extra module types (models.lua:272-337)
AVGPOOL2 = 17               # nn.SpatialAveragePooling(2,2,2,2) (models.lua:71,235,242,249,348-363)
GROUPLINEAR, GROUPCONV3 = 18, 19   # the grouped kinds of create_G4's bundle (models.lua:145-194); PRELU with a = n >= 2 is nn.PReLU(n): one slope per C / n channels
DROPOUT_V2, DROPOUT_ALWAYS_ON = 1, 2
GR_CS_RGB, GR_CS_Y, GR_CS_YUV, GR_CS_HSL = 0, 1, 2, 3      # gr_colorspace_*: the reference's four colour spaces (train.lua:45, dataset.lua:27-33)
COLOR_SPACES = {"rgb": GR_CS_RGB, "y": GR_CS_Y, "yuv": GR_CS_YUV, "hsl": GR_CS_HSL}
COMM_ID_BYTES = 128


class LayerDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("p", C.c_float), ("flags", C.c_int32)]


class Hyper(C.Structure):
    """optim.adam defaults + train_r.lua:22-24 defaults."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("l1", C.c_double), ("l2", C.c_double), ("clamp", C.c_double)]

    def __init__(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, l1=0.0, l2=1e-4, clamp=1.0):
        super().__init__(lr, beta1, beta2, eps, l1, l2, clamp)


class AdamHyper(C.Structure):
    """gr_adam_hyper: optim.adam's own four scalars (gr_adam_rows_step_dev: no penalty, no gradient clamp)"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]

    def __init__(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        super().__init__(lr, beta1, beta2, eps)


GR_OPT_SGD, GR_OPT_ADAGRAD, GR_OPT_ADADELTA, GR_OPT_ADAMAX, GR_OPT_RMSPROP = range(1, 6)      # gr_optim_step: the optim rock's other five methods
OPT_METHODS = {"sgd": GR_OPT_SGD, "adagrad": GR_OPT_ADAGRAD, "adadelta": GR_OPT_ADADELTA, "adamax": GR_OPT_ADAMAX, "rmsprop": GR_OPT_RMSPROP}
# which of a net's two state vectors a method uses, under the key the mirror in ganrev/optim.py keeps it (slot 0, slot 1); sgd's only with a momentum
OPT_STATE_KEYS = {"sgd": ("dfdx", None), "adagrad": ("paramVariance", None), "adadelta": ("paramVariance", "accDelta"), "adamax": ("m", "u"),
                  "rmsprop": ("m", None)}


class OptimConfig(C.Structure):
    """gr_optim_config: the config table of optim.sgd | adagrad | adadelta | adamax | rmsprop (adversarial.lua:147-161,174-188) + the closure's
    penalties.  OptimConfig(method, table, l1=, l2=, clamp=) reads the table's keys as the mirror in ganrev/optim.py reads them: a key that is not
    there takes that METHOD's default (learningRate: sgd, adagrad 1e-3, adamax 2e-3, rmsprop 1e-2; epsilon: adamax 1e-38, rmsprop 1e-8; dampening:
    the momentum).  State keys in the table (dfdx, evalCounter, m, ...) are not config and are ignored."""
    _fields_ = [("method", C.c_int32), ("nesterov", C.c_int32), ("learningRate", C.c_double), ("learningRateDecay", C.c_double),
                ("weightDecay", C.c_double), ("momentum", C.c_double), ("dampening", C.c_double), ("rho", C.c_double), ("eps", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("epsilon", C.c_double), ("alpha", C.c_double),
                ("l1", C.c_double), ("l2", C.c_double), ("clamp", C.c_double)]

    def __init__(self, method="sgd", config=None, l1=0.0, l2=0.0, clamp=0.0):
        cfg = dict(config or {})
        code = OPT_METHODS.get(method, method)       # a name, or a GR_OPT_* number (an unknown one is gr_optim_step's to refuse)
        if not isinstance(code, int):
            raise GanrevError(f"Unknown optimizer method '{method}'")
        mom = cfg.get("momentum", 0.0)
        super().__init__(code, int(bool(cfg.get("nesterov", False))),
                         cfg.get("learningRate", {GR_OPT_ADAMAX: 2e-3, GR_OPT_RMSPROP: 1e-2}.get(code, 1e-3)), cfg.get("learningRateDecay", 0.0),
                         cfg.get("weightDecay", 0.0), mom, cfg.get("dampening", mom), cfg.get("rho", 0.9), cfg.get("eps", 1e-6),
                         cfg.get("beta1", 0.9), cfg.get("beta2", 0.999), cfg.get("epsilon", 1e-38 if code == GR_OPT_ADAMAX else 1e-8),
                         cfg.get("alpha", 0.99), l1, l2, clamp)

    def slots(self):
        """(slot 0 used, slot 1 used) by this configuration"""
        return (self.method != GR_OPT_SGD or self.momentum != 0, self.method in (GR_OPT_ADADELTA, GR_OPT_ADAMAX))


class TsneConfig(C.Structure):
    """gr_tsne_config: the schedule of gr_tsne_run_dev (the defaults of van der Maaten's reference code; eta is the caller's)"""
    _fields_ = [("exaggeration", C.c_float), ("stop_lying_iter", C.c_int32), ("momentum0", C.c_float), ("momentum1", C.c_float),
                ("mom_switch_iter", C.c_int32), ("eta", C.c_float), ("min_gain", C.c_float)]

    def __init__(self, eta, exaggeration=12.0, stop_lying_iter=250, momentum0=0.5, momentum1=0.8, mom_switch_iter=250, min_gain=0.01):
        super().__init__(exaggeration, int(stop_lying_iter), momentum0, momentum1, int(mom_switch_iter), eta, min_gain)


_P = C.c_void_p
_F = C.POINTER(C.c_float)
_SIGS = {
    "gr_init": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "gr_shutdown": (C.c_int, [_P]),
    "gr_last_error": (C.c_char_p, [_P]),
    "gr_version": (C.c_char_p, []),
    "gr_stream": (_P, [_P]),
    "gr_synchronize": (C.c_int, [_P]),
    "gr_device_info": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "gr_net_create": (C.c_int, [_P, C.POINTER(LayerDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "gr_net_destroy": (C.c_int, [_P]),
    "gr_net_out_dim": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gr_net_param_count": (C.c_int64, [_P]),
    "gr_net_get_params": (C.c_int, [_P, _P]),
    "gr_net_set_params": (C.c_int, [_P, _P]),
    "gr_net_get_grads": (C.c_int, [_P, _P]),
    "gr_net_set_grads": (C.c_int, [_P, _P]),
    "gr_net_zero_grads": (C.c_int, [_P]),
    "gr_net_params_dev": (_P, [_P]),
    "gr_net_grads_dev": (_P, [_P]),
    "gr_net_n_bn": (C.c_int, [_P]),
    "gr_net_bn_features": (C.c_int, [_P, C.c_int]),
    "gr_net_get_bn_running": (C.c_int, [_P, C.c_int, _P, _P]),
    "gr_net_set_bn_running": (C.c_int, [_P, C.c_int, _P, _P]),
    "gr_net_set_training": (C.c_int, [_P, C.c_int]),
    "gr_net_set_seed": (C.c_int, [_P, C.c_uint64]),
    "gr_net_get_forward_counter": (C.c_int64, [_P]),
    "gr_net_set_forward_counter": (C.c_int, [_P, C.c_int64]),
    "gr_net_mask_size": (C.c_int64, [_P, C.c_int, C.c_int]),
    "gr_net_set_mask": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "gr_net_get_mask": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "gr_net_forward_host": (C.c_int, [_P, _P, C.c_int, _P]),
    "gr_net_forward_dev": (C.c_int, [_P, _P, C.c_int, _P]),
    "gr_net_output_dev": (_P, [_P]),
    "gr_net_forward_batched_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    "gr_embed_dev": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P, C.c_int64, C.c_int, _P, C.POINTER(_P)]),
    "gr_net_backward_host": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "gr_net_backward_dev": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "gr_net_set_input_grad": (C.c_int, [_P, C.c_int]),
    "gr_net_backward_input_dev": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "gr_mse_rows_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    "gr_adam_rows_step_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.POINTER(AdamHyper), C.c_int, C.c_float, _P, _P, _P, C.c_int]),
    "gr_net_layer_output": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "gr_net_get_pool_index": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "gr_mse_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(C.c_double), _P]),
    "gr_mse_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    "gr_bce_host": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_double), _P]),
    "gr_bce_dev": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P]),
    "gr_adam_step": (C.c_int, [_P, C.POINTER(Hyper), C.c_int]),
    "gr_adam_reset": (C.c_int, [_P]),
    "gr_adam_get_state": (C.c_int, [_P, _P, _P]),
    "gr_adam_set_state": (C.c_int, [_P, _P, _P]),
    "gr_optim_step": (C.c_int, [_P, C.POINTER(OptimConfig), C.c_int]),
    "gr_optim_reset": (C.c_int, [_P]),
    "gr_optim_get_state": (C.c_int, [_P, _P, _P]),
    "gr_optim_set_state": (C.c_int, [_P, _P, _P]),
    "gr_comm_unique_id": (C.c_int, [_P, _P]),
    "gr_comm_init": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "gr_comm_destroy": (C.c_int, [_P]),
    "gr_comm_ranks": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gr_comm_set_host_exchange": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "gr_allreduce_grads": (C.c_int, [_P]),
    "gr_allreduce_dev": (C.c_int, [_P, _P, C.c_int64]),
    "gr_allgather_dev": (C.c_int, [_P, _P, _P, C.c_int64]),
    "gr_broadcast_params": (C.c_int, [_P, C.c_int]),
    "gr_train_r_step": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.POINTER(Hyper), C.c_int, C.POINTER(C.c_double)]),
    "gr_set_conv_mode": (C.c_int, [_P, C.c_int]),
    "gr_get_conv_mode": (C.c_int, [_P]),
    "gr_set_tuning": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "gr_range_guard_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gr_range_guard_scan_params": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "gr_search_stats": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "gr_set_timing": (C.c_int, [_P, C.c_int]),
    "gr_last_step_times": (C.c_int, [_P, _P]),
    "gr_event_record": (C.c_int, [_P, C.c_int]),
    "gr_event_elapsed_ms": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "gr_kernel_times": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "gr_cosine_topk_host": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int]),
    "gr_cosine_topk_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int]),
    "gr_cosine_topk_queries_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int]),
    "gr_cosine_topk_queries_host": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int]),
    "gr_cosine_similarity_host": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_float)]),
    "gr_l2_distance_rows_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, _P]),
    "gr_l2_distance_rows_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, _P]),
    "gr_image_grid_dev": (C.c_int, [_P, C.POINTER(_P), _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                    _P, _P, _P, C.c_float, C.c_int, C.c_float, C.c_float, _P, _P]),
    "gr_rows_mean_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int, _P]),
    "gr_progress_grid_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "gr_l2_nearest_host": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int, C.c_int, _P, _P]),
    "gr_l2_nearest_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int, C.c_int, _P, _P]),
    "gr_kmeans_host": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "gr_cosine_assign_host": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "gr_kmeans_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "gr_cosine_assign_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "gr_cluster_members_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P]),
    "gr_cluster_faces_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, C.c_int, _P]),
    "gr_cluster_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "gr_cluster_members_wide_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P]),
    "gr_pca_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P, _P, _P, _P]),
    "gr_mixture_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "gr_silhouette_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "gr_knn_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P]),
    "gr_lof_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P]),
    "gr_knn_overlap_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P]),
    "gr_eps_graph_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_double, C.c_int, _P, _P]),
    "gr_dbscan_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P]),
    "gr_mst_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_int64, _P, _P, _P, C.POINTER(C.c_int32)]),
    "gr_hdbscan_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, C.POINTER(C.c_int32)]),
    "gr_pca_project_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P]),
    "gr_vae_sample_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P]),
    "gr_vae_sample_backward_dev": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_double, _P]),
    "gr_vae_sample_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P]),
    "gr_vae_sample_backward_host": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_double, _P]),
    "gr_ssim_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _P, _P, _P]),
    "gr_ssim_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _P, _P, _P]),
    "gr_tsne_affinities_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_double, _P, _P, _P]),
    "gr_tsne_gradient_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_float, _P, _P]),
    "gr_tsne_update_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float]),
    "gr_tsne_kl_dev": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "gr_tsne_run_dev": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int]),
    "gr_map_cells_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, _P]),
    "gr_malloc": (C.c_int, [_P, C.c_int64, C.POINTER(_P)]),
    "gr_free": (C.c_int, [_P, _P]),
    "gr_memcpy_h2d": (C.c_int, [_P, _P, _P, C.c_int64]),
    "gr_memcpy_d2h": (C.c_int, [_P, _P, _P, C.c_int64]),
    "gr_fill_normal_dev": (C.c_int, [_P, _P, C.c_int64, C.c_uint64]),
    "gr_fill_uniform_dev": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_float, C.c_uint64]),
    "gr_copy2d_dev": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int64]),
    "gr_add_dev": (C.c_int, [_P, _P, _P, C.c_int64]),
    "gr_colorspace_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _P]),
    "gr_colorspace_host": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _P]),
    "gr_image_scale_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "gr_image_scale_host": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "gr_dataset_images_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "gr_dataset_cache_create": (C.c_int, [_P, C.c_int64, C.POINTER(_P)]),
    "gr_dataset_cache_destroy": (C.c_int, [_P]),
    "gr_dataset_cache_append": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int]),
    "gr_dataset_cache_size": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gr_dataset_cache_image": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gr_dataset_cache_load_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "gr_conv3_forward_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "gr_conv3_backward_data_dev": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "gr_conv3_backward_weight_dev": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "gr_bench_mfma_loop": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "gr_bench_conv3": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)

_lib = None


def load_library():
    """dlopen libganrev.so and declare every prototype of include/ganrev.h.  No compute, no GPU needed."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GanrevError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C gan-reverser_amd/csrc`).  This package has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError here == header and library disagree
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    if isinstance(a, int):
        return C.c_void_p(a)
    return a


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def grid_shape(n_tiles, slots, channels, h, w, from_space, nrow, padding=0, margin=0):
    """(Cout, GH, GW) of gr_image_grid_dev's grid: image.toDisplayTensor's layout, xmaps = min(nrow, n_tiles) tiles per row"""
    xmaps = max(1, min(int(nrow), int(n_tiles)))
    ymaps = -(-int(n_tiles) // xmaps)
    return (3 if from_space >= 0 else int(channels), ymaps * (h + 2 * margin + padding), xmaps * (slots * w + 2 * margin + padding))


def progress_grid_shape(channels, h, w, from_space, grid_h, grid_w):
    """(Cout, GH, GW) of gr_progress_grid_dev's grid: grid_h x grid_w cells and the seven rows that carry the epoch digits"""
    return (3 if from_space >= 0 else int(channels), int(grid_h) * int(h) + 7, int(grid_w) * int(w))


def hdbscan_host(eu, ev, ew, n, min_cluster_size):
    """gr_hdbscan_host: HDBSCAN's labels (scikit-learn's rules at its defaults, include/ganrev.h) of a spanning tree over n rows as gr_mst_dev
    leaves it - eu < ev [n - 1] int32, ew [n - 1] float64 ascending - for one min_cluster_size in [2, n] -> (labels [n] int32, -1 noise;
    prob [n] float64; the number of clusters).  Host work: needs the library, no context and no GPU."""
    eu, ev = np.ascontiguousarray(eu, np.int32), np.ascontiguousarray(ev, np.int32)
    ew = np.ascontiguousarray(ew, np.float64)
    n = int(n)
    if not (eu.shape == ev.shape == ew.shape == (max(n - 1, 0),)):
        raise GanrevError(f"gr_hdbscan_host: a spanning tree over n = {n} rows has n - 1 edges, not {eu.shape}, {ev.shape}, {ew.shape}")
    labels, prob, clusters = np.empty(max(n, 0), np.int32), np.empty(max(n, 0), np.float64), C.c_int32(0)
    r = load_library().gr_hdbscan_host(_ptr(eu), _ptr(ev), _ptr(ew), n, int(min_cluster_size), _ptr(labels), _ptr(prob), C.byref(clusters))
    if r:
        raise GanrevError(f"gr_hdbscan_host: status {r}: n {n} and min_cluster_size {min_cluster_size} with 2 <= min_cluster_size <= n, and n - 1 "
                          "edges 0 <= eu < ev < n that form a tree, their weights finite, not negative and ascending")
    return labels, prob, int(clusters.value)


SSIM_MAX_WIN, SSIM_MAX_HW = 11, 128      # gr_ssim_*: window and image side at most (include/ganrev.h GR_SSIM_MAX_WIN, GR_SSIM_MAX_HW)


def ssim_check_args(n, channels, h, w, win, data_range):
    """the limits of gr_ssim_dev, checked before the library is asked (needs no GPU): raises GanrevError naming the value"""
    n, channels, h, w, win = int(n), int(channels), int(h), int(w), int(win)
    if not (1 <= n < 2 ** 31) or channels < 1:
        raise GanrevError(f"ssim: n {n} (1 .. 2^31 - 1) and channels {channels} must be positive")
    if win < 3 or win > SSIM_MAX_WIN or win % 2 == 0:
        raise GanrevError(f"ssim: win {win}: an odd window of 3 .. {SSIM_MAX_WIN}")
    if min(h, w) < win or max(h, w) > SSIM_MAX_HW:
        raise GanrevError(f"ssim: h {h}, w {w}: images of win = {win} .. {SSIM_MAX_HW} pixels a side")
    if not float(data_range) > 0:
        raise GanrevError(f"ssim: data_range {data_range} must be positive")


class Context:
    """One per process per GPU (gr_ctx)."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = _P()
        rc = self.lib.gr_init(int(device), C.byref(h))
        if rc != GR_OK:
            raise GanrevError(f"gr_init(device={device}) -> {STATUS.get(rc, rc)}: no usable gfx950 GPU "
                              "(libganrev has no CPU path; the oracle under /oracle is for tests only)")
        self.h = h
        self.device = device

    def check(self, rc, what=""):
        if rc != GR_OK:
            msg = self.lib.gr_last_error(self.h)
            raise GanrevError(f"{what}: {STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.gr_shutdown(self.h)
            self.h = None

    def synchronize(self):
        self.check(self.lib.gr_synchronize(self.h), "gr_synchronize")

    def info(self):
        buf = C.create_string_buffer(512)
        self.check(self.lib.gr_device_info(self.h, buf, 512), "gr_device_info")
        return buf.value.decode()

    # ---- raw device memory
    def malloc(self, nbytes):
        p = _P()
        self.check(self.lib.gr_malloc(self.h, int(nbytes), C.byref(p)), "gr_malloc")
        return p.value

    def free(self, p):
        self.check(self.lib.gr_free(self.h, _ptr(p)), "gr_free")

    def upload(self, arr, dptr=None):
        arr = np.ascontiguousarray(arr)
        if dptr is None:
            dptr = self.malloc(arr.nbytes)
        self.check(self.lib.gr_memcpy_h2d(self.h, _ptr(dptr), _ptr(arr), arr.nbytes), "gr_memcpy_h2d")
        return dptr

    def download(self, dptr, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        self.check(self.lib.gr_memcpy_d2h(self.h, _ptr(out), _ptr(dptr), out.nbytes), "gr_memcpy_d2h")
        return out

    def fill_normal(self, dptr, n, seed):
        self.check(self.lib.gr_fill_normal_dev(self.h, _ptr(dptr), int(n), int(seed)), "gr_fill_normal_dev")

    def fill_uniform(self, dptr, n, seed, lo=-1.0, hi=1.0):
        self.check(self.lib.gr_fill_uniform_dev(self.h, _ptr(dptr), int(n), float(lo), float(hi), int(seed)), "gr_fill_uniform_dev")

    def fill_noise(self, dptr, n, method, seed, host=None):
        """createNoiseInputs (utils/nn_utils.lua:39-51) into a device tensor of n floats: normal(0, 1) or uniform(-1, 1) drawn on the
        device, or the host array `host` uploaded in their place (parity tests)"""
        if host is not None:
            self.upload(np.ascontiguousarray(host, np.float32).reshape(int(n)), dptr)      # reshape: n floats, no more
        elif method == "uniform":
            self.fill_uniform(dptr, n, seed, -1.0, 1.0)
        elif method == "normal":
            self.fill_normal(dptr, n, seed)
        else:
            raise ValueError(f"Unknown noise method '{method}'")   # utils/nn_utils.lua:48

    def read_loss(self, dptr):
        """the float64 loss word a criterion kernel left at dptr"""
        return float(self.download(dptr, (1,), np.float64)[0])

    def copy2d(self, dst, dst_pitch, src, src_pitch, rows, cols):
        """rows x cols floats between two row-major device matrices (pitches in floats): nn.Concat's join / slice"""
        self.check(self.lib.gr_copy2d_dev(self.h, _ptr(dst), int(dst_pitch), _ptr(src), int(src_pitch), int(rows), int(cols)), "gr_copy2d_dev")

    def add(self, y, x, n):
        self.check(self.lib.gr_add_dev(self.h, _ptr(y), _ptr(x), int(n)), "gr_add_dev")

    def colorspace_dev(self, in_dev, from_, to, batch, h, w, out_dev):
        """NN_UTILS.switchColorSpace (utils/nn_utils.lua:133-246) on device tensors [batch x (1|3) x h x w]; from_ / to = GR_CS_*.  One
        launch on the context's stream, none for rgb -> rgb (a copy when the pointers differ)."""
        self.check(self.lib.gr_colorspace_dev(self.h, _ptr(in_dev), int(from_), int(to), int(batch), int(h), int(w), _ptr(out_dev)), "gr_colorspace_dev")

    def colorspace(self, images, from_, to):
        """the same on a host array [batch x (1|3) x h x w] -> a new host array [batch x (1|3) x h x w] (gr_colorspace_host)"""
        images = f32(images)
        planes = lambda cs: 1 if int(cs) == GR_CS_Y else 3
        if images.ndim != 4 or (0 <= int(from_) <= 3 and images.shape[1] != planes(from_)):
            raise GanrevError(f"colorspace: images {images.shape} are not [batch x {planes(from_)} x h x w]")
        b, _, h, w = images.shape
        out = np.empty((b, planes(to) if 0 <= int(to) <= 3 else 3, h, w), np.float32)
        self.check(self.lib.gr_colorspace_host(self.h, _ptr(images), int(from_), int(to), b, h, w, _ptr(out)), "gr_colorspace_host")
        return out

    def image_scale_dev(self, in_dev, n, planes, sh, sw, dh, dw, out_dev):
        """image.scale(src, dw, dh), bilinear (dataset.lua:112,150), on a device tensor [n x planes x sh x sw] -> out_dev [n x planes x dh x dw].
        One launch on the context's stream."""
        self.check(self.lib.gr_image_scale_dev(self.h, _ptr(in_dev), int(n), int(planes), int(sh), int(sw), int(dh), int(dw), _ptr(out_dev)),
                   "gr_image_scale_dev")

    def image_scale(self, images, dh, dw):
        """the same on a host array [n x planes x sh x sw] -> a new host array [n x planes x dh x dw] (gr_image_scale_host)"""
        images = f32(images)
        if images.ndim != 4:
            raise GanrevError(f"image_scale: images {images.shape} are not [n x planes x h x w]")
        n, planes, sh, sw = images.shape
        out = np.empty((n, planes, max(int(dh), 0), max(int(dw), 0)), np.float32)
        self.check(self.lib.gr_image_scale_host(self.h, _ptr(images), n, planes, sh, sw, int(dh), int(dw), _ptr(out)), "gr_image_scale_host")
        return out

    def dataset_images_dev(self, bytes_dev, n, sh, sw, sc, dh, dw, to_space, normalize, out_dev):
        """dataset.lua:149-153 for n decoded files of one size: uint8 HWC [n x sh x sw x sc] in device memory -> out_dev fp32
        [n x (1|3) x dh x dw] in colour space to_space (GR_CS_*), normalised to [-1, 1] when `normalize`.  One launch (gr_dataset_images_dev)."""
        self.check(self.lib.gr_dataset_images_dev(self.h, _ptr(bytes_dev), int(n), int(sh), int(sw), int(sc), int(dh), int(dw), int(to_space),
                                                  int(bool(normalize)), _ptr(out_dev)), "gr_dataset_images_dev")

    def bce_dev(self, x, t, n, loss_dev, grad_dev=None):
        self.check(self.lib.gr_bce_dev(self.h, _ptr(x), _ptr(t), int(n), _ptr(loss_dev), _ptr(grad_dev)), "gr_bce_dev")

    # ---- criterion / search
    def mse(self, x, t, n_global=None, want_grad=True):
        x, t = f32(x), f32(t)
        loss = C.c_double()
        g = np.empty_like(x) if want_grad else None
        self.check(self.lib.gr_mse_host(self.h, _ptr(x), _ptr(t), x.size, int(n_global or x.size), C.byref(loss), _ptr(g)), "gr_mse_host")
        return loss.value, g

    def mse_dev(self, x, t, n, loss_dev, grad_dev=None, n_global=None):
        """nn.MSECriterion (sizeAverage) on device tensors of n floats: the loss (one double) into loss_dev, gradInput into
        grad_dev when given; n_global = the element count the mean is taken over (default n)"""
        self.check(self.lib.gr_mse_dev(self.h, _ptr(x), _ptr(t), int(n), int(n_global or n), _ptr(loss_dev), _ptr(grad_dev)), "gr_mse_dev")

    def mse_rows_dev(self, x, t, rows, n, loss_rows_dev, grad_dev=None):
        """per-row nn.MSECriterion on device tables [rows x n]: loss_rows_dev[i] (float) = mean_j (x_ij - t_ij)^2, grad_dev (when given) its
        gradient 2 (x - t) / n.  One launch; the bits repeat."""
        self.check(self.lib.gr_mse_rows_dev(self.h, _ptr(x), _ptr(t), int(rows), int(n), _ptr(loss_rows_dev), _ptr(grad_dev)), "gr_mse_rows_dev")

    def adam_rows_step_dev(self, z, g, m, v, rows, nd, hyper, t, loss_rows, best_loss, best_z, clamp=0.0, update=True):
        """one launch: rows whose loss_rows fell below best_loss store it and copy their z to best_z; then (update) optim.adam step t on
        z / g / m / v [rows x nd] (hyper: AdamHyper), z clamped to +-clamp when clamp > 0"""
        self.check(self.lib.gr_adam_rows_step_dev(self.h, _ptr(z), _ptr(g), _ptr(m), _ptr(v), int(rows), int(nd), C.byref(hyper) if hyper is not None else None,
                                                  int(t), float(clamp), _ptr(loss_rows), _ptr(best_loss), _ptr(best_z), int(bool(update))), "gr_adam_rows_step_dev")

    def bce(self, x, t, want_grad=True):
        """nn.BCECriterion (sizeAverage): (loss, gradInput)"""
        x, t = f32(x), f32(t)
        loss = C.c_double()
        g = np.empty_like(x) if want_grad else None
        self.check(self.lib.gr_bce_host(self.h, _ptr(x), _ptr(t), x.size, C.byref(loss), _ptr(g)), "gr_bce_host")
        return loss.value, g

    def cosine_topk(self, emb, query_rows, k, accumulate_in_float=False, emb_dev=None, n=None, d=None):
        q = np.ascontiguousarray(query_rows, dtype=np.int64)
        if emb_dev is None:
            emb = f32(emb)
            n, d = emb.shape
        k = min(int(k), int(n))
        idx = np.empty((q.size, k), dtype=np.int64)
        sc = np.empty((q.size, k), dtype=np.float32)
        if emb_dev is None:
            rc = self.lib.gr_cosine_topk_host(self.h, _ptr(emb), n, d, _ptr(q), q.size, k, _ptr(idx), _ptr(sc), int(accumulate_in_float))
        else:
            rc = self.lib.gr_cosine_topk_dev(self.h, _ptr(emb_dev), n, d, _ptr(q), q.size, k, _ptr(idx), _ptr(sc), int(accumulate_in_float))
        self.check(rc, "gr_cosine_topk")
        return idx, sc

    def cosine_topk_queries(self, emb, queries, k, accumulate_in_float=False, emb_dev=None, n=None, d=None, queries_dev=None, q=None):
        """search by example: cosine_topk with needle i = row i of `queries` [q x d], vectors that need not be rows of the table; every row of
        the table is scored -> (idx int64 [q, k], scores float32 [q, k]).  emb_dev (with n, d): the table is in device memory; queries_dev (with
        q): so are the needles.  Host needles against a device table are uploaded once; a host table takes host needles."""
        if emb_dev is None:
            emb = f32(emb)
            n, d = emb.shape
        n, d = int(n), int(d)
        if queries_dev is None:
            queries = f32(queries).reshape(-1, d)
            q = queries.shape[0]
        elif emb_dev is None:
            raise GanrevError("cosine_topk_queries: device needles need a device table (emb_dev)")
        q, k = int(q), min(int(k), n)
        idx = np.empty((q, max(k, 0)), dtype=np.int64)
        sc = np.empty((q, max(k, 0)), dtype=np.float32)
        if emb_dev is None:
            rc = self.lib.gr_cosine_topk_queries_host(self.h, _ptr(emb), n, d, _ptr(queries), q, k, _ptr(idx), _ptr(sc), int(accumulate_in_float))
        else:
            qdev = queries_dev if queries_dev is not None else (self.upload(queries) if q > 0 else None)
            try:
                rc = self.lib.gr_cosine_topk_queries_dev(self.h, _ptr(emb_dev), n, d, _ptr(qdev), q, k, _ptr(idx), _ptr(sc), int(accumulate_in_float))
            finally:
                if queries_dev is None and qdev is not None:
                    self.free(qdev)
        self.check(rc, "gr_cosine_topk_queries")
        return idx, sc

    def cosine_similarity(self, a, b):
        a, b = f32(a).ravel(), f32(b).ravel()
        out = C.c_float()
        self.check(self.lib.gr_cosine_similarity_host(self.h, _ptr(a), _ptr(b), a.size, C.byref(out)), "gr_cosine_similarity_host")
        return out.value

    def l2_distance_rows(self, a, b):
        """torch.dist(a[i], b[i]) for every row i (apply_r.lua:369)."""
        a, b = f32(a), f32(b)
        n = a.shape[0]
        a2, b2 = a.reshape(n, -1), b.reshape(n, -1)
        out = np.empty(n, dtype=np.float64)
        self.check(self.lib.gr_l2_distance_rows_host(self.h, _ptr(a2), _ptr(b2), n, a2.shape[1], _ptr(out)), "gr_l2_distance_rows_host")
        return out

    def l2_distance_rows_dev(self, a_dev, b_dev, n, d):
        """the same on two device-resident tables [n x d] (gr_l2_distance_rows_dev): same kernel, same bits; the distances come to the host"""
        out = np.empty(int(n), dtype=np.float64)
        self.check(self.lib.gr_l2_distance_rows_dev(self.h, _ptr(a_dev), _ptr(b_dev), int(n), int(d), _ptr(out)), "gr_l2_distance_rows_dev")
        return out

    def rows_mean_dev(self, table_dev, n_rows, d, rows, out_dev):
        """apply_r.lua:233-243: out_dev [d] = the mean of the listed rows of the device table [n_rows x d], added in list order in fp32 and
        divided once (gr_rows_mean_dev); zeros for an empty list"""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        self.check(self.lib.gr_rows_mean_dev(self.h, _ptr(table_dev), int(n_rows), int(d), _ptr(rows) if rows.size else None, rows.size, _ptr(out_dev)),
                   "gr_rows_mean_dev")

    def image_grid_dev(self, srcs, n_rows, channels, h, w, from_space, rows, nrow, padding=0, margin=0, bg=None, inset=None,
                       inset_rgb=None, fill=1.0, auto_range=False, lo=0.0, hi=1.0, grid_dev=None, u8_dev=None):
        """gr_image_grid_dev (include/ganrev.h states the layout and the arithmetic): srcs = the device tables of the 1 or 2 slots,
        n_rows their row counts, rows [n_tiles x slots] int64 (-1: background), bg [n_tiles x 3], inset [n_tiles] flags.
        -> (Cout, GH, GW) of the grid written to grid_dev (floats, planar) and / or u8_dev (bytes, interleaved)."""
        slots = len(srcs)
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, max(slots, 1))
        n_tiles = rows.shape[0]
        tabs = (_P * max(slots, 1))(*[_ptr(p) for p in srcs])
        nr = np.ascontiguousarray(n_rows, dtype=np.int64).reshape(-1)
        bg = None if bg is None else np.ascontiguousarray(bg, dtype=np.float32).reshape(n_tiles, 3)
        inset = None if inset is None else np.ascontiguousarray(inset, dtype=np.uint8).reshape(n_tiles)
        inset_rgb = None if inset_rgb is None else np.ascontiguousarray(inset_rgb, dtype=np.float32).reshape(3)
        rc = self.lib.gr_image_grid_dev(self.h, tabs, _ptr(nr), slots, int(channels), int(h), int(w), int(from_space), _ptr(rows), n_tiles,
                                        int(nrow), int(padding), int(margin), _ptr(bg), _ptr(inset), _ptr(inset_rgb), float(fill),
                                        int(bool(auto_range)), float(lo), float(hi), _ptr(grid_dev), _ptr(u8_dev))
        self.check(rc, "gr_image_grid_dev")
        return grid_shape(n_tiles, slots, channels, h, w, from_space, nrow, padding, margin)

    def progress_grid_dev(self, table_dev, n_rows, channels, h, w, from_space, rows, grid_h, grid_w, epoch, grid_dev=None, u8_dev=None,
                          n_show=None):
        """gr_progress_grid_dev = NN_UTILS.imagesToGridTensor (include/ganrev.h states the layout): the first grid_h * grid_w of the
        listed rows of the device table [n_rows x channels x h x w] as cells, the epoch's digits below them.  n_show: len(rows).
        -> (Cout, GH, GW) of the grid written to grid_dev (floats, planar) and / or u8_dev (bytes, interleaved)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n_show = rows.size if n_show is None else int(n_show)
        rc = self.lib.gr_progress_grid_dev(self.h, _ptr(table_dev), int(n_rows), int(channels), int(h), int(w), int(from_space),
                                           _ptr(rows) if rows.size else None, n_show, int(grid_h), int(grid_w), int(epoch),
                                           _ptr(grid_dev), _ptr(u8_dev))
        self.check(rc, "gr_progress_grid_dev")
        return progress_grid_shape(channels, h, w, from_space, grid_h, grid_w)

    L2_NEAREST_MAX_Q = 64       # queries per gr_l2_nearest_* call (include/ganrev.h)

    def l2_nearest(self, table, queries, k, table_dev=None, n=None, d=None):
        """sample.lua:130-148 findClosestNeighboursOf: the k nearest rows of `table` [n x d] for each row of `queries` [q x d] by
        torch.dist, ordered by (distance, row) -> (idx int64 [q, k], dist float64 [q, k]).  table_dev (with n, d): the table is already
        in device memory (gr_l2_nearest_dev; the queries are uploaded per call).  More than 64 queries take several calls."""
        if table_dev is None:
            table = f32(table)
            n = table.shape[0]
            d = int(np.prod(table.shape[1:]))
        n, d = int(n), int(d)
        qs = f32(queries).reshape(-1, d)
        nq = qs.shape[0]
        idx = np.empty((nq, int(k)), dtype=np.int64)
        dist = np.empty((nq, int(k)), dtype=np.float64)
        for q0 in range(0, nq, self.L2_NEAREST_MAX_Q):
            part = np.ascontiguousarray(qs[q0:q0 + self.L2_NEAREST_MAX_Q])
            oi, od = idx[q0:q0 + len(part)], dist[q0:q0 + len(part)]
            if table_dev is None:
                rc = self.lib.gr_l2_nearest_host(self.h, _ptr(table), n, d, _ptr(part), len(part), int(k), _ptr(oi), _ptr(od))
            else:
                qd = self.upload(part)
                try:
                    rc = self.lib.gr_l2_nearest_dev(self.h, _ptr(table_dev), n, d, _ptr(qd), len(part), int(k), _ptr(oi), _ptr(od))
                finally:
                    self.free(qd)
            self.check(rc, "gr_l2_nearest")
        return idx, dist

    def kmeans(self, x, k, niter, centroids0):
        """unsup.kmeans(x, k, niter) (apply_r.lua:198) from the given initial centroids -> (centroids, totalcounts, labels)."""
        x = f32(x)
        n, d = x.shape
        cent = np.array(centroids0, dtype=np.float32, order="C", copy=True).reshape(k, d)
        tot = np.zeros(k, np.float32)
        lab = np.zeros(n, np.int32)
        self.check(self.lib.gr_kmeans_host(self.h, _ptr(x), n, d, int(k), int(niter), _ptr(cent), _ptr(tot), _ptr(lab)), "gr_kmeans_host")
        return cent, tot, lab

    def cosine_assign(self, x, centroids, take_min=True):
        """apply_r.lua:205-217: per row the centroid with the minimum (reference behaviour) or maximum cosine similarity."""
        x, cent = f32(x), f32(centroids)
        n, d = x.shape
        lab = np.zeros(n, np.int32)
        sim = np.zeros(n, np.float32)
        self.check(self.lib.gr_cosine_assign_host(self.h, _ptr(x), n, d, _ptr(cent), cent.shape[0], int(take_min), _ptr(lab), _ptr(sim)),
                   "gr_cosine_assign_host")
        return lab, sim

    def kmeans_dev(self, x_dev, n, d, k, niter, cent_dev, totalcounts_dev=None, labels_dev=None):
        """gr_kmeans_dev: unsup.kmeans on a device table [n x d]; cent_dev [k x d] carries the initial centroids in and the final ones out,
        totalcounts_dev [k] floats and labels_dev [n] int32 are optional.  Enqueued on the context's stream."""
        self.check(self.lib.gr_kmeans_dev(self.h, _ptr(x_dev), int(n), int(d), int(k), int(niter), _ptr(cent_dev), _ptr(totalcounts_dev), _ptr(labels_dev)),
                   "gr_kmeans_dev")

    def cosine_assign_dev(self, x_dev, n, d, cent_dev, k, take_min, labels_dev, sims_dev):
        """gr_cosine_assign_dev (apply_r.lua:205-217): labels_dev [n] int32 and sims_dev [n] floats for the device table [n x d]"""
        self.check(self.lib.gr_cosine_assign_dev(self.h, _ptr(x_dev), int(n), int(d), _ptr(cent_dev), int(k), int(bool(take_min)), _ptr(labels_dev),
                                                 _ptr(sims_dev)), "gr_cosine_assign_dev")

    def cluster_members_dev(self, labels_dev, sims_dev, n, k, m, rows_out_dev, sims_out_dev, kept_out_dev, sizes_out_dev):
        """gr_cluster_members_dev (apply_r.lua:218-227): per cluster the m most similar member rows -> rows_out_dev int64 [k x m] (-1 fill),
        sims_out_dev float [k x m] (0 fill), kept_out_dev / sizes_out_dev int32 [k]"""
        self.check(self.lib.gr_cluster_members_dev(self.h, _ptr(labels_dev), _ptr(sims_dev), int(n), int(k), int(m), _ptr(rows_out_dev), _ptr(sims_out_dev),
                                                   _ptr(kept_out_dev), _ptr(sizes_out_dev)), "gr_cluster_members_dev")

    CLUSTER_WIDE_MIN_K = 33          # default of gr_set_tuning "cluster_wide_min_k": gr_cluster_dev's wide kernels from this k on (tests set 1)

    def cluster_dev(self, x_dev, n, d, k, niter, cent_dev, take_min, m, totalcounts_dev, labels_dev, sims_dev, rows_out_dev, sims_out_dev, kept_out_dev,
                    sizes_out_dev):
        """gr_cluster_dev (apply_r.lua:198-227 in one enqueue, k <= 4096, d <= 256, m <= 128): k-means from cent_dev [k x d] (final centroids out;
        totalcounts_dev [k] or None), the cosine assignment into labels_dev int32 / sims_dev [n], and per cluster the m most similar member rows
        into rows_out_dev int64 / sims_out_dev [k x m] (-1 / 0 fill), kept_out_dev / sizes_out_dev int32 [k]"""
        self.check(self.lib.gr_cluster_dev(self.h, _ptr(x_dev), int(n), int(d), int(k), int(niter), _ptr(cent_dev), int(bool(take_min)), int(m),
                                           _ptr(totalcounts_dev), _ptr(labels_dev), _ptr(sims_dev), _ptr(rows_out_dev), _ptr(sims_out_dev),
                                           _ptr(kept_out_dev), _ptr(sizes_out_dev)), "gr_cluster_dev")

    def cluster_faces_dev(self, table_dev, n_rows, d, rows_dev, kept_dev, k, m, out_dev):
        """gr_cluster_faces_dev (apply_r.lua:233-243): out_dev [k x d] = the average faces of all clusters (rows_dev int64 [k x m], kept_dev int32 [k])"""
        self.check(self.lib.gr_cluster_faces_dev(self.h, _ptr(table_dev), int(n_rows), int(d), _ptr(rows_dev), _ptr(kept_dev), int(k), int(m), _ptr(out_dev)),
                   "gr_cluster_faces_dev")

    def cluster_members_wide_dev(self, labels_dev, sims_dev, n, k, m, rows_out_dev, sims_out_dev, kept_out_dev, sizes_out_dev):
        """gr_cluster_members_wide_dev: cluster_members_dev's lists for any k <= 4096, by the kernels of gr_cluster_dev's wide route; sims_dev is
        any per-row score (a mixture's posteriors)"""
        self.check(self.lib.gr_cluster_members_wide_dev(self.h, _ptr(labels_dev), _ptr(sims_dev), int(n), int(k), int(m), _ptr(rows_out_dev),
                                                        _ptr(sims_out_dev), _ptr(kept_out_dev), _ptr(sizes_out_dev)), "gr_cluster_members_wide_dev")

    MIXTURE_MAX_D = MIXTURE_MAX_K = 256     # gr_mixture_dev: columns and components at most (include/ganrev.h)

    def mixture_dev(self, x_dev, n, d, k, niter, var_floor, weights_dev, means_dev, vars_dev, loglik_dev, labels_dev=None, post_dev=None, rowll_dev=None):
        """gr_mixture_dev (1 <= n < 2^31, d <= 256, k <= 256): niter EM iterations of a diagonal Gaussian mixture on the device table [n x d] from
        weights_dev [k], means_dev / vars_dev [k x d] floats (fitted parameters out), then one E-step: loglik_dev [niter + 1] doubles, labels_dev
        int32 / post_dev / rowll_dev [n] floats (each may be None).  niter = 0 scores rows under the given parameters.  Enqueued; no host wait."""
        self.check(self.lib.gr_mixture_dev(self.h, _ptr(x_dev), int(n), int(d), int(k), int(niter), float(var_floor), _ptr(weights_dev), _ptr(means_dev),
                                           _ptr(vars_dev), _ptr(loglik_dev), _ptr(labels_dev), _ptr(post_dev), _ptr(rowll_dev)), "gr_mixture_dev")

    SILHOUETTE_MAX_N, SILHOUETTE_MAX_D, SILHOUETTE_MAX_K = 262144, 256, 4096     # gr_silhouette_dev's limits (include/ganrev.h GR_SILHOUETTE_MAX_N)
    SILHOUETTE_METRICS = {"euclidean": 0, "cosine": 1}

    def silhouette_dev(self, x_dev, n, d, labels_dev, k, metric, s_dev, cluster_mean_dev, sizes_dev, mean_dev, a_dev=None, b_dev=None, nearest_dev=None):
        """gr_silhouette_dev (2 <= n <= 262144, d <= 256, k <= 4096): the silhouette coefficients of the device table [n x d] under labels_dev [n]
        int32 (a label outside [0, k): no cluster); metric "euclidean" / "cosine" (or 0 / 1) -> s_dev [n] doubles, cluster_mean_dev [k] doubles,
        sizes_dev [k] int32, mean_dev 1 double; a_dev / b_dev [n] doubles and nearest_dev [n] int32 may be None.  Enqueued; no host wait."""
        if isinstance(metric, str):
            if metric not in self.SILHOUETTE_METRICS:
                raise GanrevError(f"silhouette: metric {metric!r}: one of {sorted(self.SILHOUETTE_METRICS)}")
            metric = self.SILHOUETTE_METRICS[metric]
        self.check(self.lib.gr_silhouette_dev(self.h, _ptr(x_dev), int(n), int(d), _ptr(labels_dev), int(k), int(metric), _ptr(s_dev), _ptr(a_dev),
                                              _ptr(b_dev), _ptr(nearest_dev), _ptr(cluster_mean_dev), _ptr(sizes_dev), _ptr(mean_dev)), "gr_silhouette_dev")

    KNN_MAX_N, KNN_MAX_D, KNN_MAX_K = 262144, 256, 128      # gr_knn_dev's limits (include/ganrev.h GR_KNN_MAX_N, GR_KNN_MAX_D, GR_KNN_MAX_K)
    KNN_METRICS = {"euclidean": 0, "cosine": 1}

    def knn_dev(self, x_dev, n, d, k, metric, idx_dev, dist_dev):
        """gr_knn_dev (2 <= n <= 262144, d <= 256, k <= min(n - 1, 128)): the k nearest rows j != i of every row i of the device table [n x d], by
        (distance, j) ascending; metric "euclidean" / "cosine" (or 0 / 1) -> idx_dev [n x k] int32, dist_dev [n x k] doubles.  Enqueued; no host
        wait."""
        if isinstance(metric, str):
            if metric not in self.KNN_METRICS:
                raise GanrevError(f"knn: metric {metric!r}: one of {sorted(self.KNN_METRICS)}")
            metric = self.KNN_METRICS[metric]
        self.check(self.lib.gr_knn_dev(self.h, _ptr(x_dev), int(n), int(d), int(k), int(metric), _ptr(idx_dev), _ptr(dist_dev)), "gr_knn_dev")

    def lof_dev(self, idx_dev, dist_dev, n, k, lof_dev, lrd_dev=None):
        """gr_lof_dev: the local outlier factors of a graph as knn_dev leaves it -> lof_dev [n] doubles, and the local reachability densities
        into lrd_dev [n] doubles unless None.  Enqueued; no host wait."""
        self.check(self.lib.gr_lof_dev(self.h, _ptr(idx_dev), _ptr(dist_dev), int(n), int(k), _ptr(lrd_dev), _ptr(lof_dev)), "gr_lof_dev")

    def knn_overlap_dev(self, idx_a_dev, idx_b_dev, n, k, count_dev, mean_dev):
        """gr_knn_overlap_dev: two graphs over the same n rows with the same k -> count_dev [n] int32, how many entries of a's row i are in b's row
        i, and mean_dev 1 double, the mean of count / k.  Enqueued; no host wait."""
        self.check(self.lib.gr_knn_overlap_dev(self.h, _ptr(idx_a_dev), _ptr(idx_b_dev), int(n), int(k), _ptr(count_dev), _ptr(mean_dev)), "gr_knn_overlap_dev")

    DBSCAN_MAX_N, DBSCAN_MAX_D = 262144, 256                # gr_eps_graph_dev's limits (include/ganrev.h GR_DBSCAN_MAX_N, GR_DBSCAN_MAX_D)
    DBSCAN_METRICS = {"euclidean": 0, "cosine": 1}

    @staticmethod
    def eps_words(n):
        """GR_EPS_WORDS(n): the 64-bit words of one row of an eps-graph over n rows"""
        return (int(n) + 63) // 64

    def eps_graph_dev(self, x_dev, n, d, eps, metric, adj_dev, count_dev):
        """gr_eps_graph_dev (2 <= n <= 262144, d <= 256, eps finite and >= 0): the eps-neighbourhood graph of the device table [n x d] as a bitmap;
        metric "euclidean" / "cosine" (or 0 / 1) -> adj_dev [n x eps_words(n)] uint64, bit j of row i set iff dist(i, j) <= eps (the diagonal
        always), and count_dev [n] int32, the rows' popcounts.  Enqueued; no host wait."""
        if isinstance(metric, str):
            if metric not in self.DBSCAN_METRICS:
                raise GanrevError(f"density: metric {metric!r}: one of {sorted(self.DBSCAN_METRICS)}")
            metric = self.DBSCAN_METRICS[metric]
        self.check(self.lib.gr_eps_graph_dev(self.h, _ptr(x_dev), int(n), int(d), float(eps), int(metric), _ptr(adj_dev), _ptr(count_dev)), "gr_eps_graph_dev")

    def dbscan_dev(self, adj_dev, count_dev, n, min_pts, labels_dev, core_dev, n_clusters_dev):
        """gr_dbscan_dev: DBSCAN's labels of an eps-graph as eps_graph_dev leaves it (1 <= min_pts <= n) -> labels_dev [n] int32 (-1: noise),
        core_dev [n] int32 0 / 1 unless None, n_clusters_dev 1 int32.  WAITS on the stream once per round of the component search to read whether
        a label changed; the last kernels are enqueued and not waited for."""
        self.check(self.lib.gr_dbscan_dev(self.h, _ptr(adj_dev), _ptr(count_dev), int(n), int(min_pts), _ptr(labels_dev), _ptr(core_dev),
                                          _ptr(n_clusters_dev)), "gr_dbscan_dev")

    MST_MAX_N, MST_MAX_D = 262144, 256                      # gr_mst_dev's limits (include/ganrev.h GR_MST_MAX_N, GR_MST_MAX_D)
    MST_METRICS = {"euclidean": 0, "cosine": 1}

    def mst_dev(self, x_dev, n, d, metric, core_dev, core_stride, eu_dev, ev_dev, ew_dev):
        """gr_mst_dev (2 <= n <= 262144, d <= 256): the exact minimum spanning tree of the device table [n x d] under w_ij = max(dist_ij, core_i,
        core_j), core_i = core_dev[i * core_stride] doubles (core_dev None: w_ij = dist_ij); metric "euclidean" / "cosine" (or 0 / 1) -> eu_dev,
        ev_dev [n - 1] int32, eu < ev, and ew_dev [n - 1] doubles: the unique tree under the order (w, lo, hi), ascending by it.  Returns the
        number of Boruvka rounds (at most ceil(log2 n)).  WAITS on the stream once per round to read how many edges are out; the last kernel
        (the ranking of the edges) is enqueued and not waited for."""
        if isinstance(metric, str):
            if metric not in self.MST_METRICS:
                raise GanrevError(f"hierarchy: metric {metric!r}: one of {sorted(self.MST_METRICS)}")
            metric = self.MST_METRICS[metric]
        rounds = C.c_int32(0)
        self.check(self.lib.gr_mst_dev(self.h, _ptr(x_dev), int(n), int(d), int(metric), _ptr(core_dev), int(core_stride), _ptr(eu_dev), _ptr(ev_dev),
                                       _ptr(ew_dev), C.byref(rounds)), "gr_mst_dev")
        return int(rounds.value)

    VAE_MAX_ND = 256                 # gr_vae_sample_*: latent dimensions at most (include/ganrev.h GR_VAE_MAX_ND)

    def vae_sample_dev(self, h_dev, eps_dev, B, nd, z_dev, kl_rows_dev=None, kl_dev=None):
        """gr_vae_sample_dev (1 <= B < 2^31, nd <= 256): h_dev [B x 2 nd] = (mu | logvar), eps_dev [B x nd] or None (eps = 0) ->
        z_dev [B x nd] = mu + exp(logvar / 2) eps, kl_rows_dev [B] floats and kl_dev, one double, their mean (each may be None).  Enqueued; no host wait."""
        self.check(self.lib.gr_vae_sample_dev(self.h, _ptr(h_dev), _ptr(eps_dev), int(B), int(nd), _ptr(z_dev), _ptr(kl_rows_dev), _ptr(kl_dev)),
                   "gr_vae_sample_dev")

    def vae_sample_backward_dev(self, h_dev, eps_dev, gz_dev, B, nd, kl_weight, gh_dev):
        """gr_vae_sample_backward_dev: gh_dev [B x 2 nd] = the gradient of recon + kl_weight mean_i KL_i with respect to h, from gz_dev = d recon / d z.
        Enqueued; no host wait."""
        self.check(self.lib.gr_vae_sample_backward_dev(self.h, _ptr(h_dev), _ptr(eps_dev), _ptr(gz_dev), int(B), int(nd), float(kl_weight), _ptr(gh_dev)),
                   "gr_vae_sample_backward_dev")

    def vae_sample_host(self, h, eps=None, want_kl=True):
        """gr_vae_sample_host on host arrays: h [B x 2 nd], eps [B x nd] or None -> (z, kl_rows, kl); the last two None without want_kl.  The bits of
        vae_sample_dev."""
        h = f32(h)
        if h.ndim != 2 or h.shape[1] % 2:
            raise GanrevError(f"vae_sample_host: h {h.shape} is not [B x 2 nd]")
        B, nd = h.shape[0], h.shape[1] // 2
        if eps is not None:
            eps = f32(eps)
            if eps.shape != (B, nd):
                raise GanrevError(f"vae_sample_host: eps {eps.shape} is not [{B} x {nd}]")
        z = np.empty((B, nd), np.float32)
        rows = np.empty(B, np.float32) if want_kl else None
        kl = np.empty(1, np.float64) if want_kl else None
        self.check(self.lib.gr_vae_sample_host(self.h, _ptr(h), _ptr(eps), B, nd, _ptr(z), _ptr(rows), _ptr(kl)),
                   "gr_vae_sample_host")
        return z, rows, (float(kl[0]) if want_kl else None)

    def vae_sample_backward_host(self, h, eps, gz, kl_weight):
        """gr_vae_sample_backward_host on host arrays -> gh [B x 2 nd].  The bits of vae_sample_backward_dev."""
        h, gz = f32(h), f32(gz)
        if h.ndim != 2 or h.shape[1] % 2 or gz.shape != (h.shape[0], h.shape[1] // 2):
            raise GanrevError(f"vae_sample_backward_host: h {h.shape} / gz {gz.shape} are not [B x 2 nd] / [B x nd]")
        B, nd = gz.shape
        if eps is not None:
            eps = f32(eps)
            if eps.shape != (B, nd):
                raise GanrevError(f"vae_sample_backward_host: eps {eps.shape} is not [{B} x {nd}]")
        gh = np.empty((B, 2 * nd), np.float32)
        self.check(self.lib.gr_vae_sample_backward_host(self.h, _ptr(h), _ptr(eps), _ptr(gz), B, nd, float(kl_weight), _ptr(gh)),
                   "gr_vae_sample_backward_host")
        return gh

    def ssim_dev(self, a_dev, b_dev, n, channels, h, w, ssim_rows_dev, mse_rows_dev=None, ssim_mean_dev=None, win=11, sigma=1.5, data_range=1.0):
        """gr_ssim_dev: a_dev, b_dev [n x channels x h x w] floats -> ssim_rows_dev [n] floats, the structural similarity index per image over the valid
        positions of a win x win Gaussian window (sigma <= 0: uniform); mse_rows_dev [n] floats and ssim_mean_dev, one double (each may be None).
        win odd, 3 .. 11, <= min(h, w); h, w <= 128.  Enqueued; no host wait."""
        ssim_check_args(n, channels, h, w, win, data_range)
        self.check(self.lib.gr_ssim_dev(self.h, _ptr(a_dev), _ptr(b_dev), int(n), int(channels), int(h), int(w), int(win), float(sigma), float(data_range),
                                        _ptr(ssim_rows_dev), _ptr(mse_rows_dev), _ptr(ssim_mean_dev)), "gr_ssim_dev")

    def ssim_host(self, a, b, win=11, sigma=1.5, data_range=1.0, want_mse=True, want_mean=True):
        """gr_ssim_host on host arrays [n x channels x h x w] -> (ssim_rows, mse_rows, mean); mse_rows / mean None when not wanted.  The bits of ssim_dev."""
        a, b = f32(a), f32(b)
        if a.ndim != 4 or a.shape != b.shape:
            raise GanrevError(f"ssim_host: a {a.shape} / b {b.shape} are not two tables [n x channels x h x w] of one shape")
        n, ch, h, w = a.shape
        ssim_check_args(n, ch, h, w, win, data_range)
        rows = np.empty(n, np.float32)
        mse = np.empty(n, np.float32) if want_mse else None
        mean = np.empty(1, np.float64) if want_mean else None
        self.check(self.lib.gr_ssim_host(self.h, _ptr(a), _ptr(b), n, ch, h, w, int(win), float(sigma), float(data_range), _ptr(rows), _ptr(mse), _ptr(mean)),
                   "gr_ssim_host")
        return rows, mse, (float(mean[0]) if want_mean else None)

    PCA_MAX_D = 256                  # gr_pca_dev / gr_pca_project_dev: columns at most (include/ganrev.h)

    def pca_dev(self, x_dev, n, d, mean_dev, cov_dev, eigvals_dev, axes_dev, info_dev):
        """gr_pca_dev (2 <= n < 2^31, d <= 256): the principal axes of the device table [n x d] -> mean_dev [d] doubles, cov_dev [d x d] doubles
        or None, eigvals_dev [d] doubles (descending), axes_dev [d x d] floats (row = unit axis), info_dev [2] int32 (sweeps, converged).
        Enqueued on the context's stream."""
        self.check(self.lib.gr_pca_dev(self.h, _ptr(x_dev), int(n), int(d), _ptr(mean_dev), _ptr(cov_dev), _ptr(eigvals_dev), _ptr(axes_dev),
                                       _ptr(info_dev)), "gr_pca_dev")

    def pca_project_dev(self, x_dev, n, d, mean_dev, axes_dev, eigvals_dev, k, whiten, out_dev):
        """gr_pca_project_dev: out_dev [n x k] = (x - mean) . axes[0 .. k)^T, column a times 1 / sqrt(eigval_a) when whiten (0 for eigval_a <= 0;
        eigvals_dev may be None otherwise)"""
        self.check(self.lib.gr_pca_project_dev(self.h, _ptr(x_dev), int(n), int(d), _ptr(mean_dev), _ptr(axes_dev), _ptr(eigvals_dev), int(k),
                                               int(bool(whiten)), _ptr(out_dev)), "gr_pca_project_dev")

    TSNE_MAX_N = 16384               # GR_TSNE_MAX_N: rows of a map at most (include/ganrev.h)

    def tsne_affinities_dev(self, x_dev, n, d, perplexity, p_dev, beta_dev, info_dev):
        """gr_tsne_affinities_dev (4 <= n <= 16384, 1 <= perplexity <= (n - 1) / 3): the joint probabilities of the device table [n x d] ->
        p_dev [n x n] floats (symmetric, zero diagonal), beta_dev [n] doubles or None, info_dev [2] int32 (most updates of beta a row needed,
        rows that hit the cap of 50).  Enqueued on the context's stream."""
        self.check(self.lib.gr_tsne_affinities_dev(self.h, _ptr(x_dev), int(n), int(d), float(perplexity), _ptr(p_dev), _ptr(beta_dev), _ptr(info_dev)),
                   "gr_tsne_affinities_dev")

    def tsne_gradient_dev(self, p_dev, y_dev, n, exaggeration, grad_dev, z_dev=None):
        """gr_tsne_gradient_dev: grad_dev [n x 2] = 4 (e sum_j p w (y_i - y_j) - sum_j w^2 (y_i - y_j) / Z); z_dev [1] double or None"""
        self.check(self.lib.gr_tsne_gradient_dev(self.h, _ptr(p_dev), _ptr(y_dev), int(n), float(exaggeration), _ptr(grad_dev), _ptr(z_dev)),
                   "gr_tsne_gradient_dev")

    def tsne_update_dev(self, y_dev, grad_dev, inc_dev, gains_dev, n, eta, momentum, min_gain=0.01):
        """gr_tsne_update_dev: the delta-bar-delta step on y, inc, gains [n x 2] in place, then y minus its column mean"""
        self.check(self.lib.gr_tsne_update_dev(self.h, _ptr(y_dev), _ptr(grad_dev), _ptr(inc_dev), _ptr(gains_dev), int(n), float(eta), float(momentum),
                                               float(min_gain)), "gr_tsne_update_dev")

    def tsne_kl_dev(self, p_dev, y_dev, n, kl_dev):
        """gr_tsne_kl_dev: kl_dev [1] double = sum_{p > 0} p log(p Z / w)"""
        self.check(self.lib.gr_tsne_kl_dev(self.h, _ptr(p_dev), _ptr(y_dev), int(n), _ptr(kl_dev)), "gr_tsne_kl_dev")

    def tsne_run_dev(self, p_dev, n, config, y_dev, inc_dev, gains_dev, first_iter, iters, kl_dev=None, kl_every=0):
        """gr_tsne_run_dev: iterations first_iter .. first_iter + iters - 1 of the schedule in `config` (a TsneConfig) without a host
        synchronisation; the KL after every iteration t with (t + 1) % kl_every == 0 goes to kl_dev[(t + 1) / kl_every - 1]"""
        self.check(self.lib.gr_tsne_run_dev(self.h, _ptr(p_dev), int(n), C.byref(config) if config is not None else None, _ptr(y_dev), _ptr(inc_dev),
                                            _ptr(gains_dev), int(first_iter), int(iters), _ptr(kl_dev), int(kl_every)), "gr_tsne_run_dev")

    def map_cells_dev(self, y_dev, n, grid_h, grid_w, rows_out_dev, counts_dev=None):
        """gr_map_cells_dev: rows_out_dev [grid_h x grid_w] int64 = the row of y_dev [n x 2] nearest to each cell's centre (-1: empty),
        counts_dev [grid_h x grid_w] int32 or None"""
        self.check(self.lib.gr_map_cells_dev(self.h, _ptr(y_dev), int(n), int(grid_h), int(grid_w), _ptr(rows_out_dev), _ptr(counts_dev)),
                   "gr_map_cells_dev")

    # ---- data parallel
    def comm_unique_id(self):
        buf = (C.c_ubyte * COMM_ID_BYTES)()
        self.check(self.lib.gr_comm_unique_id(self.h, buf), "gr_comm_unique_id")
        return bytes(buf)

    def comm_init(self, uid, nranks, rank):
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(uid)
        self.check(self.lib.gr_comm_init(self.h, buf, int(nranks), int(rank)), "gr_comm_init")

    def comm_destroy(self):
        self.check(self.lib.gr_comm_destroy(self.h), "gr_comm_destroy")

    EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)

    def set_host_exchange(self, nranks, rank, fn):
        """Install fn(dev_ptr, count, kind) -> 0 as this context's collectives (gr_comm_set_host_exchange: kind 0 fp32 SUM, 1 fp64 SUM,
        2 uint32 MAX over the ranks, result left in the device buffer); fn = None removes it.  The "fake comm" of SURVEY.md section 4."""
        if fn is None:
            self._xchg_cb = None
            self.check(self.lib.gr_comm_set_host_exchange(self.h, 1, 0, None, None), "gr_comm_set_host_exchange")
            return

        def tramp(user, buf, count, kind):
            try:
                return int(fn(buf, int(count), int(kind)) or 0)
            except Exception:  # noqa: BLE001 - an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._xchg_cb = self.EXCHANGE_FN(tramp)           # keep the trampoline alive as long as the library may call it
        self.check(self.lib.gr_comm_set_host_exchange(self.h, int(nranks), int(rank), C.cast(self._xchg_cb, C.c_void_p), None),
                   "gr_comm_set_host_exchange")

    def allreduce(self, dptr, n):
        self.check(self.lib.gr_allreduce_dev(self.h, _ptr(dptr), int(n)), "gr_allreduce_dev")

    def allgather(self, send_dev, recv_dev, nbytes):
        self.check(self.lib.gr_allgather_dev(self.h, _ptr(send_dev), _ptr(recv_dev), int(nbytes)), "gr_allgather_dev")

    def set_conv_mode(self, mode):
        """0 / "f32": exact fp32 MFMA; 1 / "bf16x6": fp32-accurate 3-term bf16 split on the bf16 MFMA (6 products);
        2 / "f16x3": fp32-accurate 2-term fp16 split of power-of-two-scaled operands on the f16 MFMA (3 products)."""
        mode = {"f32": 0, "bf16x6": 1, "f16x3": 2}.get(mode, mode)
        self.check(self.lib.gr_set_conv_mode(self.h, int(mode)), "gr_set_conv_mode")

    def set_tuning(self, key, value):
        self.check(self.lib.gr_set_tuning(self.h, key.encode(), int(value)), "gr_set_tuning")

    def search_reruns(self):
        """searches whose sample-bound filter overflowed and ran again on every key, since gr_init"""
        a = C.c_int64(0)
        self.check(self.lib.gr_search_stats(self.h, C.byref(a)), "gr_search_stats")
        return a.value

    def range_guard_stats(self):
        """(scan launches, passes sent to bf16x6) of the f16x3 range guard since gr_init"""
        a, b = C.c_int64(0), C.c_int64(0)
        self.check(self.lib.gr_range_guard_stats(self.h, C.byref(a), C.byref(b)), "gr_range_guard_stats")
        return a.value, b.value

    def conv_mode(self):
        return ("f32", "bf16x6", "f16x3")[self.lib.gr_get_conv_mode(self.h)]

    def set_timing(self, mode):
        self.check(self.lib.gr_set_timing(self.h, int(mode)), "gr_set_timing")

    def kernel_times(self):
        import json
        buf = C.create_string_buffer(1 << 18)
        self.check(self.lib.gr_kernel_times(self.h, buf, 1 << 18), "gr_kernel_times")
        return json.loads(buf.value.decode())

    def event_record(self, slot):
        self.check(self.lib.gr_event_record(self.h, int(slot)), "gr_event_record")

    def event_elapsed_ms(self, a, b):
        ms = C.c_float()
        self.check(self.lib.gr_event_elapsed_ms(self.h, int(a), int(b), C.byref(ms)), "gr_event_elapsed_ms")
        return ms.value

    def comm_ranks(self):
        n, r = C.c_int(), C.c_int()
        self.check(self.lib.gr_comm_ranks(self.h, C.byref(n), C.byref(r)), "gr_comm_ranks")
        return n.value, r.value

    def last_step_times(self):
        t = np.zeros(6, dtype=np.float32)
        self.check(self.lib.gr_last_step_times(self.h, _ptr(t)), "gr_last_step_times")
        return dict(zip(("g_fwd", "r_fwd", "loss", "r_bwd", "allreduce", "adam"), t.tolist()))

    def bench_mfma_loop(self, shape=0, launches=100):
        """fp32-accurate TFLOP/s the bare f16x3 inner loop sustains on this device (0: 32x32x16, 1: 16x16x32 MFMA shape)"""
        t = C.c_float()
        self.check(self.lib.gr_bench_mfma_loop(self.h, int(shape), int(launches), C.byref(t)), "gr_bench_mfma_loop")
        return t.value

    def bench_conv3(self, which, batch, cin, cout, h, w, iters):
        ms = C.c_float()
        self.check(self.lib.gr_bench_conv3(self.h, which, batch, cin, cout, h, w, iters, C.byref(ms)), "gr_bench_conv3")
        return ms.value


_default_ctx = None


def default_context():
    """Lazily created process-wide context on LOCAL_RANK (one process per GPU)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_ctx


class Net:
    """gr_net handle: a compiled nn.Sequential.

    perm (optional): the net keeps its flat vectors in another order than the module tree's getParameters() - a bundle of nn.Concat
    branches (ganrev.nn.bundle_plan) is layer-major on the device, branch-major in the tree.  net_flat = tree_flat[perm].  The
    host <-> device transfers of the flat vectors below are the ONE place that knows: callers see tree order, and everything that
    consumes the vectors on the device (Adam / the optim rules, penalty, clamp, the gradient all-reduce) is element-wise."""

    def __init__(self, ctx, descs, in_dims, perm=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.perm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int64)
        arr = (LayerDesc * len(descs))(*[LayerDesc(*d) for d in descs])
        h = _P()
        c, hh, w = in_dims
        ctx.check(self.lib.gr_net_create(ctx.h, arr, len(descs), int(c), int(hh), int(w), C.byref(h)), "gr_net_create")
        self.h = h
        self.in_dims = tuple(int(v) for v in in_dims)
        oc, oh, ow = C.c_int(), C.c_int(), C.c_int()
        ctx.check(self.lib.gr_net_out_dim(h, C.byref(oc), C.byref(oh), C.byref(ow)), "gr_net_out_dim")
        self.out_dims = (oc.value, oh.value, ow.value)
        self.n_params = int(self.lib.gr_net_param_count(h))
        assert self.perm is None or self.perm.size == self.n_params, (self.perm.size, self.n_params)
        self.training = True               # the mode set_training last gave the net (a new gr_net is in training mode)
        self.input_grad = False            # set_input_grad: evaluate()-mode forwards keep what backward_input_dev reads

    def close(self):
        if getattr(self, "h", None):
            self.lib.gr_net_destroy(self.h)
            self.h = None

    def __del__(self):
        # a net nobody holds any more gives its device buffers back (they are sized by the largest batch it ran); not after its
        # context was shut down - gr_shutdown has released the context the net points to
        try:
            if getattr(self, "h", None) and getattr(getattr(self, "ctx", None), "h", None):
                self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown: nothing to report to)
            pass

    def _c(self, rc, what):
        self.ctx.check(rc, what)

    def _to_net(self, a):
        """a flat vector in tree order -> the net's order"""
        return a if self.perm is None or a is None else np.ascontiguousarray(a.reshape(-1)[self.perm])

    def _to_tree(self, a):
        if self.perm is None:
            return a
        out = np.empty_like(a)
        out[self.perm] = a
        return out

    def get_params(self):
        a = np.empty(self.n_params, dtype=np.float32)
        self._c(self.lib.gr_net_get_params(self.h, _ptr(a)), "gr_net_get_params")
        return self._to_tree(a)

    def set_params(self, a):
        a = self._to_net(f32(a))
        assert a.size == self.n_params
        self._c(self.lib.gr_net_set_params(self.h, _ptr(a)), "gr_net_set_params")

    def get_grads(self):
        a = np.empty(self.n_params, dtype=np.float32)
        self._c(self.lib.gr_net_get_grads(self.h, _ptr(a)), "gr_net_get_grads")
        return self._to_tree(a)

    def set_grads(self, a):
        a = self._to_net(f32(a))
        self._c(self.lib.gr_net_set_grads(self.h, _ptr(a)), "gr_net_set_grads")

    def zero_grads(self):
        self._c(self.lib.gr_net_zero_grads(self.h), "gr_net_zero_grads")

    def n_bn(self):
        return self.lib.gr_net_n_bn(self.h)

    def get_bn_running(self, i):
        n = self.lib.gr_net_bn_features(self.h, i)
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        self._c(self.lib.gr_net_get_bn_running(self.h, i, _ptr(m), _ptr(v)), "gr_net_get_bn_running")
        return m, v

    def set_bn_running(self, i, m, v):
        m, v = f32(m), f32(v)
        self._c(self.lib.gr_net_set_bn_running(self.h, i, _ptr(m), _ptr(v)), "gr_net_set_bn_running")

    def set_training(self, t):
        self._c(self.lib.gr_net_set_training(self.h, int(bool(t))), "gr_net_set_training")
        self.training = bool(t)

    def set_seed(self, s):
        self._c(self.lib.gr_net_set_seed(self.h, int(s)), "gr_net_set_seed")

    def forward_counter(self):
        """the Philox forward-call counter (gr_net_get_forward_counter): forwards since set_seed, in either mode"""
        return int(self.lib.gr_net_get_forward_counter(self.h))

    def set_forward_counter(self, counter):
        self._c(self.lib.gr_net_set_forward_counter(self.h, int(counter)), "gr_net_set_forward_counter")

    def mask_size(self, layer, batch):
        return int(self.lib.gr_net_mask_size(self.h, layer, batch))

    def set_mask(self, layer, keep):
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        self._c(self.lib.gr_net_set_mask(self.h, layer, _ptr(keep), keep.size), "gr_net_set_mask")

    def get_mask(self, layer, n):
        keep = np.empty(n, dtype=np.uint8)
        self._c(self.lib.gr_net_get_mask(self.h, layer, _ptr(keep), n), "gr_net_get_mask")
        return keep

    def forward(self, x, out=None):
        x = f32(x)
        b = x.shape[0]
        if out is None:
            out = np.empty((b,) + self._shape(self.out_dims), dtype=np.float32)
        self._c(self.lib.gr_net_forward_host(self.h, _ptr(x), b, _ptr(out)), "gr_net_forward_host")
        return out

    def forward_dev(self, x_dev, batch, out_dev=None):
        self._c(self.lib.gr_net_forward_dev(self.h, _ptr(x_dev), int(batch), _ptr(out_dev)), "gr_net_forward_dev")
        return self.lib.gr_net_output_dev(self.h)

    def forward_batched_dev(self, x_dev, rows, batch, out_dev):
        """utils/nn_utils.lua:5-33 on device-resident rows: chunks of `batch` rows, each written straight into out_dev"""
        self._c(self.lib.gr_net_forward_batched_dev(self.h, _ptr(x_dev), int(rows), int(batch), _ptr(out_dev)), "gr_net_forward_batched_dev")

    def backward(self, x, gout, want_gin=True):
        x, gout = f32(x), f32(gout)
        b = x.shape[0]
        gin = np.empty_like(x) if want_gin else None
        self._c(self.lib.gr_net_backward_host(self.h, _ptr(x), _ptr(gout), b, _ptr(gin)), "gr_net_backward_host")
        return gin

    def backward_dev(self, x_dev, gout_dev, batch, gin_dev=None):
        self._c(self.lib.gr_net_backward_dev(self.h, _ptr(x_dev), _ptr(gout_dev), int(batch), _ptr(gin_dev)), "gr_net_backward_dev")

    def set_input_grad(self, on):
        """evaluate()-mode forwards keep what backward_input_dev reads (gr_net_set_input_grad); off (the default) they are what they always were"""
        self._c(self.lib.gr_net_set_input_grad(self.h, int(bool(on))), "gr_net_set_input_grad")
        self.input_grad = bool(on)

    def backward_input_dev(self, x_dev, gout_dev, batch, gin_dev):
        """nn.Module:updateGradInput in evaluate(): gradInput alone, nothing accumulated (gr_net_backward_input_dev)"""
        self._c(self.lib.gr_net_backward_input_dev(self.h, _ptr(x_dev), _ptr(gout_dev), int(batch), _ptr(gin_dev)), "gr_net_backward_input_dev")

    def layer_output(self, layer, shape):
        a = np.empty(shape, dtype=np.float32)
        self._c(self.lib.gr_net_layer_output(self.h, layer, _ptr(a), a.size), "gr_net_layer_output")
        return a

    def pool_index(self, layer, n):
        """nn.SpatialMaxPooling.indices of the last forward: n bytes, 0..3 = (dy, dx) scan position in the window"""
        a = np.empty(n, dtype=np.uint8)
        self._c(self.lib.gr_net_get_pool_index(self.h, int(layer), _ptr(a), a.size), "gr_net_get_pool_index")
        return a

    def adam_step(self, hyper, t):
        self._c(self.lib.gr_adam_step(self.h, C.byref(hyper), int(t)), "gr_adam_step")

    def adam_reset(self):
        self._c(self.lib.gr_adam_reset(self.h), "gr_adam_reset")

    def adam_state(self):
        m, v = np.empty(self.n_params, np.float32), np.empty(self.n_params, np.float32)
        self._c(self.lib.gr_adam_get_state(self.h, _ptr(m), _ptr(v)), "gr_adam_get_state")
        return self._to_tree(m), self._to_tree(v)

    def set_adam_state(self, m, v):
        m, v = self._to_net(f32(m)), self._to_net(f32(v))
        self._c(self.lib.gr_adam_set_state(self.h, _ptr(m), _ptr(v)), "gr_adam_set_state")

    def optim_step(self, config, t):
        """penalty + clamp + optim.<config.method> on the device (config: OptimConfig); t = 1-based count of steps since optim_reset"""
        self._c(self.lib.gr_optim_step(self.h, C.byref(config), int(t)), "gr_optim_step")

    def optim_reset(self):
        self._c(self.lib.gr_optim_reset(self.h), "gr_optim_reset")

    def optim_state(self):
        """the net's two state vectors (slot 0, slot 1): what they mean is the method's business (OPT_STATE_KEYS)"""
        a, b = np.empty(self.n_params, np.float32), np.empty(self.n_params, np.float32)
        self._c(self.lib.gr_optim_get_state(self.h, _ptr(a), _ptr(b)), "gr_optim_get_state")
        return self._to_tree(a), self._to_tree(b)

    def set_optim_state(self, slot0=None, slot1=None):
        slot0, slot1 = (None if s is None else self._to_net(f32(s)) for s in (slot0, slot1))
        assert all(s is None or s.size == self.n_params for s in (slot0, slot1))
        self._c(self.lib.gr_optim_set_state(self.h, _ptr(slot0), _ptr(slot1)), "gr_optim_set_state")

    def range_guard_scan(self):
        """f16x3 range guard for loops built from the *_dev calls: synchronous scan of this net's weights / BatchNorm scales; True
        when the context's guard has tripped (it then stays on bf16x6)."""
        t = C.c_int(0)
        self._c(self.lib.gr_range_guard_scan_params(self.h, C.byref(t)), "gr_range_guard_scan_params")
        return bool(t.value)

    def allreduce_grads(self):
        self._c(self.lib.gr_allreduce_grads(self.h), "gr_allreduce_grads")

    def broadcast_params(self, root=0):
        self._c(self.lib.gr_broadcast_params(self.h, int(root)), "gr_broadcast_params")

    @staticmethod
    def _shape(d):
        c, h, w = d
        return (c,) if (h == 1 and w == 1) else (c, h, w)


class DatasetCache:
    """gr_dataset_cache handle: the decoded files of a dataset in device memory (uint8 HWC at source size), and the one launch that turns any
    list of them into the fp32 table gr_dataset_images_dev would write image by image.  One owner, like Net: close() (or the finaliser)
    destroys it while its context is open, never after."""

    def __init__(self, ctx, chunk_bytes=0):
        self.ctx, self.lib = ctx, ctx.lib
        h = _P()
        ctx.check(self.lib.gr_dataset_cache_create(ctx.h, int(chunk_bytes), C.byref(h)), "gr_dataset_cache_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.gr_dataset_cache_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if getattr(self, "h", None) and getattr(getattr(self, "ctx", None), "h", None):
                self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown: nothing to report to)
            pass

    def append(self, image):
        """one decoded file, uint8 [H x W x 1|3|4] (or [H x W]) -> its number in the cache"""
        a = np.ascontiguousarray(image, dtype=np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            raise GanrevError(f"DatasetCache.append: an image is uint8 [H x W x C], not {a.shape}")
        self.ctx.check(self.lib.gr_dataset_cache_append(self.h, _ptr(a), a.shape[0], a.shape[1], a.shape[2]), "gr_dataset_cache_append")
        return len(self) - 1

    def size(self):
        """(images held, their decoded bytes)"""
        n, b = C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.lib.gr_dataset_cache_size(self.h, C.byref(n), C.byref(b)), "gr_dataset_cache_size")
        return n.value, b.value

    def __len__(self):
        return self.size()[0]

    def image(self, i):
        """(sh, sw, sc) of image i: the record kept on the host"""
        sh, sw, sc = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.lib.gr_dataset_cache_image(self.h, int(i), C.byref(sh), C.byref(sw), C.byref(sc)), "gr_dataset_cache_image")
        return sh.value, sw.value, sc.value

    def load_dev(self, indices, dh, dw, to_space, normalize, out_dev):
        """row k of out_dev fp32 [n x (1|3) x dh x dw] = image indices[k], scaled, in colour space to_space (GR_CS_*), normalised to [-1, 1] when
        `normalize`: one launch on the context's stream (gr_dataset_cache_load_dev)"""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        self.ctx.check(self.lib.gr_dataset_cache_load_dev(self.h, _ptr(idx) if idx.size else None, idx.size, int(dh), int(dw), int(to_space),
                                                          int(bool(normalize)), _ptr(out_dev)), "gr_dataset_cache_load_dev")


def embed_dev(gnet, rnets, noise_dev, rows, batch, attr_out_devs, images_out_dev=None):
    """apply_r.lua:145-153 on the device: noise -> G -> images -> every net of `rnets` -> attr_out_devs[k]; nothing visits the host"""
    n = len(rnets)
    nets = (_P * max(n, 1))(*[r.h for r in rnets])
    outs = (_P * max(n, 1))(*[_ptr(p) for p in attr_out_devs])
    rc = gnet.lib.gr_embed_dev(gnet.h, nets, n, _ptr(noise_dev), int(rows), int(batch), _ptr(images_out_dev), outs)
    gnet.ctx.check(rc, "gr_embed_dev")


def train_r_step(gnet, rnet, noise_dev, batch, global_batch, hyper, t, want_loss=True):
    loss = C.c_double()
    rc = rnet.lib.gr_train_r_step(gnet.h, rnet.h, _ptr(noise_dev), int(batch), int(global_batch), C.byref(hyper), int(t),
                                  C.byref(loss) if want_loss else None)
    rnet.ctx.check(rc, "gr_train_r_step")
    return loss.value if want_loss else None
