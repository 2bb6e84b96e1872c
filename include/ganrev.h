/*
 * ganrev.h — C ABI of libganrev.so: the MI355X (gfx950) implementation of gan-reverser's hot path
 * (G forward, R forward/backward, L2+clamp+Adam, data-parallel gradient all-reduce, cosine top-k).
 *
 * The reference has no C header: its boundary is the Torch7 nn.Module / nn.Criterion / optim
 * protocol as *used* by the scripts.  Each entry point below cites the reference call it replaces
 * (paths relative to the reference checkout).  Conventions:
 *   - every call returns GR_OK (0) or a negative gr_status; no C++ exception or abort() crosses the ABI;
 *     gr_last_error(ctx) returns the message of the last failure on that context;
 *   - handles are opaque; one gr_ctx per process per GPU; calls on one ctx are serialised by the caller;
 *   - tensors are fp32, contiguous, NCHW (what the reference's host FloatTensors are, train_r.lua:63);
 *   - `*_host` pointers are host memory and the call is synchronous on return (Lua semantics);
 *     `*_dev` pointers are device memory of the ctx's GPU, work is enqueued on the ctx's stream
 *     (gr_stream) and the call returns without waiting.
 *   - no torch types, no HIP types in signatures (streams/pointers travel as void*).
 */
#ifndef GANREV_H
#define GANREV_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GR_OK = 0,
  GR_ERR_INVALID = -1,      /* bad argument / shape mismatch */
  GR_ERR_UNSUPPORTED = -2,  /* layer sequence or size this build has no kernel for */
  GR_ERR_HIP = -3,          /* HIP runtime error (message has hipGetErrorString) */
  GR_ERR_NO_DEVICE = -4,    /* no gfx950 device: the library has no CPU fallback */
  GR_ERR_COMM = -5,         /* RCCL error */
  GR_ERR_STATE = -6         /* call order (e.g. backward before forward, backward in evaluate mode) */
} gr_status;

/* Module kinds = the nn.* / cudnn.* constructors on the path (models.lua:104-143, 389-464). Numeric values
 * are shared with the test oracle's go_layer so one descriptor list can drive both. */
enum {
  GR_CONV3 = 1,            /* nn/cudnn.SpatialConvolution(a=nInputPlane, b=nOutputPlane, 3,3,1,1,1,1)  models.lua:122,409 */
  GR_BN = 2,               /* nn.SpatialBatchNormalization(a) / nn.BatchNormalization(a)          models.lua:116,410,448 */
  GR_ELU = 3,              /* nn.ELU()                                                           models.lua:411 */
  GR_RELU = 4,             /* cudnn.ReLU(true)                                                   models.lua:117 */
  GR_LEAKYRELU = 5,        /* nn.LeakyReLU(p)            (north_star names it; models.lua:18 dead code) */
  GR_SIGMOID = 6,          /* nn.Sigmoid()                                                       models.lua:133 */
  GR_TANH = 7,             /* nn.Tanh()                                                          models.lua:453 */
  GR_DROPOUT = 8,          /* nn.Dropout(p[,v1])   flags: GR_DROPOUT_V2, GR_DROPOUT_ALWAYS_ON    models.lua:402-405,412,450 */
  GR_SPATIAL_DROPOUT = 9,  /* nn.SpatialDropout(p)                                               models.lua:439 */
  GR_MAXPOOL2 = 10,        /* nn.SpatialMaxPooling(2,2)                                          models.lua:422,440 */
  GR_UPSAMPLE2 = 11,       /* nn.SpatialUpSamplingNearest(2)                                     models.lua:121,127 */
  GR_VIEW = 12,            /* nn.View(a[,b,c])                                                   models.lua:118,446 */
  GR_LINEAR = 13,          /* nn.Linear(a=in, b=out)                                             models.lua:115,447,451 */
  GR_FULLCONV3 = 14,       /* nn.SpatialFullConvolution(a,b,3,3,1,1,1,1) (north_star names it; absent from the reference) */
  /* the module types the D network adds (models.lua:272-337 create_D2, trained by adversarial.lua:37-205) */
  GR_CONVK = 15,           /* nn.SpatialConvolution(a, b, c=K, K, 1, 1, (K-1)/2, (K-1)/2), K = 5 or 1      models.lua:275,297; 8-55 */
  GR_PRELU = 16,           /* nn.PReLU(): one learnable slope (nOutputPlane 0) in the flat vector; the host mirror starts it at 0.25  models.lua:276.
                              a = n >= 2: nn.PReLU(n), n slopes in the flat vector, slope j over channels [j C/n, (j+1) C/n) (C % n == 0; n = C is
                              Torch7's per-plane PReLU); a stage of its own.  a = 0 or 1: the shared slope */
  GR_AVGPOOL2 = 17,        /* nn.SpatialAveragePooling(2,2,2,2)                                  models.lua:71,235,242,249,348-363 */
  /* the grouped kinds an nn.Concat(2) of structurally identical branches compiles to (models.lua:145-194 create_G4); exact fp32 in every
     GR_CONV_MODE, deterministic */
  GR_GROUPLINEAR = 18,     /* c = G block-diagonal nn.Linear(a/G, b/G) side by side (a % G == b % G == 0): group g reads inputs [g a/G, (g+1) a/G),
                              writes outputs [g b/G, (g+1) b/G); weight [b][a/G] (the groups' matrices one after another), bias [b]; output (b,1,1) */
  GR_GROUPCONV3 = 19       /* 3x3 stride-1 pad-1 convolution a -> b planes in c = G groups (a % G == b % G == 0); weight [b][a/G][3][3] (the `groups`
                              layout of cudnn.SpatialConvolution), bias [b]; may stand behind GR_UPSAMPLE2 like GR_CONV3 */
};
#define GR_DROPOUT_V2 1         /* nn.Dropout default: train-time scale 1/(1-p), identity in evaluate() */
#define GR_DROPOUT_ALWAYS_ON 2  /* the fixer's `drop.evaluate = function() end` (models.lua:402-405) */

typedef struct { int32_t kind, a, b, c; float p; int32_t flags; } gr_layer_desc;

typedef struct gr_ctx gr_ctx;
typedef struct gr_net gr_net;

/* ---- context: replaces cutorch.setDevice / cutorch.manualSeed (train_r.lua:58-62) ---- */
int gr_init(int device, gr_ctx** out);
int gr_shutdown(gr_ctx* ctx);
const char* gr_last_error(gr_ctx* ctx);       /* replaces Lua error()/assert messages */
const char* gr_version(void);
void* gr_stream(gr_ctx* ctx);                 /* hipStream_t all work of this ctx is enqueued on */
int gr_synchronize(gr_ctx* ctx);
int gr_device_info(gr_ctx* ctx, char* buf, int buflen);

/* ---- nn.Sequential: models.create_G3 / create_R_default build one of these (models.lua:104,389) ---- */
int gr_net_create(gr_ctx* ctx, const gr_layer_desc* layers, int n_layers, int in_c, int in_h, int in_w, gr_net** out);
int gr_net_destroy(gr_net* net);
int gr_net_out_dim(gr_net* net, int* c, int* h, int* w);
/* m:getParameters() (train_r.lua:122): flat order = modules in sequence order, weight then bias, BN gamma then beta */
int64_t gr_net_param_count(gr_net* net);
int gr_net_get_params(gr_net* net, float* host);
int gr_net_set_params(gr_net* net, const float* host);
int gr_net_get_grads(gr_net* net, float* host);
int gr_net_set_grads(gr_net* net, const float* host);
int gr_net_zero_grads(gr_net* net);                        /* GRAD_PARAMETERS_R:zero()  train_r.lua:143 */
float* gr_net_params_dev(gr_net* net);                     /* device views of the two flat vectors */
float* gr_net_grads_dev(gr_net* net);
/* BN running statistics (module.running_mean / running_var; not part of getParameters) */
int gr_net_n_bn(gr_net* net);
int gr_net_bn_features(gr_net* net, int bn_index);
int gr_net_get_bn_running(gr_net* net, int bn_index, float* mean_host, float* var_host);
int gr_net_set_bn_running(gr_net* net, int bn_index, const float* mean_host, const float* var_host);
/* m:training() / m:evaluate()  (train_r.lua:70,189,222; apply_r.lua:64,94,103) */
int gr_net_set_training(gr_net* net, int training);
/* Dropout noise: production = counter-based Philox keyed (seed, forward-call counter, layer, element)
 * [replaces torch.manualSeed-driven MT19937, train_r.lua:38-39]; tests inject explicit keep flags. */
int gr_net_set_seed(gr_net* net, uint64_t seed);
/* The forward-call counter of that key: every gr_net_forward_* adds one, in either mode; gr_net_set_seed restarts it at 0.  Reading it
 * before a forward that is only an observation (an evaluate() look at the model in the middle of a training run: ganrev/progress.py) and
 * setting it back afterwards leaves the Dropout masks of every later forward as they would have been without it.  get: -1 for a null
 * net; set: GR_ERR_INVALID for a null net or a negative counter. */
int64_t gr_net_get_forward_counter(gr_net* net);
int gr_net_set_forward_counter(gr_net* net, int64_t counter);
int64_t gr_net_mask_size(gr_net* net, int layer_index, int batch);       /* elements of that layer's noise tensor */
int gr_net_set_mask(gr_net* net, int layer_index, const uint8_t* keep_host, int64_t n);  /* used by the NEXT forward only */
int gr_net_get_mask(gr_net* net, int layer_index, uint8_t* keep_host, int64_t n);        /* noise of the LAST forward */
/* m:forward(input) -> m.output   (train_r.lua:139,146; utils/nn_utils.lua:18) */
int gr_net_forward_host(gr_net* net, const float* in_host, int batch, float* out_host);
int gr_net_forward_dev(gr_net* net, const float* in_dev, int batch, float* out_dev /*nullable: result stays in m.output*/);
float* gr_net_output_dev(gr_net* net);                     /* m.output (device), valid until the next forward.  After an evaluate()-mode gr_net_forward_dev with a
                                                            * non-null out_dev the last stage wrote out_dev ITSELF (no copy): m.output then IS the caller's buffer and is
                                                            * valid only while the caller keeps out_dev alive (Torch7: the caller's tensor).  Same for gr_net_layer_output
                                                            * of the last layer. */
/* NN_UTILS.forwardBatched(model, input, batchSize) (utils/nn_utils.lua:5-33; apply_r.lua:146,152,153) on device-resident rows:
 * in_dev [rows x in] -> out_dev [rows x out] in chunks of `batch` rows (the last one ragged).  In evaluate() mode each chunk's last
 * kernel writes its rows of out_dev itself: the reference's per-row copy loop (utils/nn_utils.lua:25-28) has no counterpart.
 * m.output afterwards = the last chunk's rows of out_dev. */
int gr_net_forward_batched_dev(gr_net* net, const float* in_dev, int64_t rows, int batch, float* out_dev);
/* apply_r.lua:145-153 as one device-resident pipeline: per chunk of `batch` rows  images = G:forward(noise) (:146), then for each of
 * the n_rnets reverser nets (MODEL_R :152, MODEL_R_FIXER :153)  attributes_k = R_k:forward(images)  written to attr_out_dev[k]
 * [rows x nd_k] - the tables gr_cosine_topk_dev searches (apply_r.lua:265-282).  images_out_dev [rows x C x H x W] is nullable: the images
 * are kept only when the caller needs them (pixel-wise search, fix-faces); otherwise a chunk's images live in G's output buffer
 * until R has read them.  Every net keeps the mode its m:evaluate() / m:training() call set (apply_r.lua:64,94,103: evaluate). */
int gr_embed_dev(gr_net* gnet, gr_net* const* rnets, int n_rnets, const float* noise_dev, int64_t rows, int batch,
                 float* images_out_dev /*nullable*/, float* const* attr_out_dev);
/* m:backward(input, gradOutput) -> m.gradInput ; accumulates into the flat gradient  (train_r.lua:151) */
int gr_net_backward_host(gr_net* net, const float* in_host, const float* grad_out_host, int batch, float* grad_in_host /*nullable*/);
int gr_net_backward_dev(gr_net* net, const float* in_dev, const float* grad_out_dev, int batch, float* grad_in_dev /*nullable*/);
/* nn.Module:updateGradInput in evaluate() mode: gradInput alone.  A frozen BatchNorm is a per-channel affine map of the running statistics,
 * no parameter gradient is formed, and neither the flat gradient nor a running statistic nor a mask is touched; everything runs on the
 * context's stream.  gr_net_set_input_grad(net, 1) (per net, default 0) makes every evaluate()-mode forward of the net keep what this
 * backward reads - raw stage outputs and fp32 stage outputs instead of fused epilogues and operand-ready-only hand-overs; with the flag
 * off the forward is what it always was.  gr_net_backward_input_dev needs the last forward to have been such a forward at the same
 * batch, and the net still in evaluate() mode: GR_ERR_STATE otherwise, with a message naming what is missing. */
int gr_net_set_input_grad(gr_net* net, int on);
int gr_net_backward_input_dev(gr_net* net, const float* in_dev, const float* grad_out_dev, int batch, float* grad_in_dev);
/* nn.SpatialMaxPooling.indices of the last forward (models.lua:422,440): one byte per output element, 0..3 = position in the
 * 2x2 window in scan order (dy, dx); n must be batch * C * Ho * Wo of that layer */
int gr_net_get_pool_index(gr_net* net, int layer_index, uint8_t* host, int64_t n);
/* debugging / layer-by-layer parity: copy out the output of module `layer_index` of the last forward */
int gr_net_layer_output(gr_net* net, int layer_index, float* host, int64_t n);

/* ---- nn.MSECriterion (train_r.lua:119,147,150). n_global = element count the mean is taken over
 * (= n on one GPU; = global batch * nd under data parallelism so a SUM all-reduce reproduces the reference). ---- */
int gr_mse_host(gr_ctx* ctx, const float* x_host, const float* t_host, int64_t n, int64_t n_global, double* loss_out, float* grad_host /*nullable*/);
int gr_mse_dev(gr_ctx* ctx, const float* x_dev, const float* t_dev, int64_t n, int64_t n_global, double* loss_dev /*1 double*/, float* grad_dev /*nullable*/);
/* nn.BCECriterion, sizeAverage = true (train.lua:173: CRITERION = nn.BCECriterion(), used by adversarial.lua; THNN BCECriterion.c, EPS = 1e-12):
 * loss = -1/n sum(log(x + EPS) t + log(1 - x + EPS) (1 - t)), gradInput = -1/n (t - x) / ((1 - x + EPS)(x + EPS)); terms in double. */
int gr_bce_host(gr_ctx* ctx, const float* x_host, const float* t_host, int64_t n, double* loss_out, float* grad_host /*nullable*/);
int gr_bce_dev(gr_ctx* ctx, const float* x_dev, const float* t_dev, int64_t n, double* loss_dev /*1 double*/, float* grad_dev /*nullable*/);

/* ---- fevalR penalty + clamp (train_r.lua:153-165) fused with optim.adam (train_r.lua:125,170) ---- */
typedef struct {
  double lr, beta1, beta2, eps;   /* optim.adam defaults: 1e-3, 0.9, 0.999, 1e-8 */
  double l1, l2, clamp;           /* OPT.R_L1 0, OPT.R_L2 1e-4, OPT.R_clamp 1   (train_r.lua:22-24) */
} gr_hyper;
int gr_adam_step(gr_net* net, const gr_hyper* h, int t /*1-based step; state.t after increment*/);
/* ---- noise refinement: row-wise criterion and optimiser on device tables (every row is an optimisation problem of its own) ----
 * gr_mse_rows_dev: loss[i] = sum_j (x_ij - t_ij)^2 / n (a float per row; the sum in double in a fixed order, so the bits repeat) and, unless
 * grad_dev is null, grad_ij = 2 (x_ij - t_ij) / n.  One launch.
 * gr_adam_rows_step_dev, one launch: first, every row whose loss_rows[i] < best_loss[i] stores that loss and copies row i of z to best_z;
 * then, when update != 0, optim.adam at step t (1-based) on z / g / m / v [rows x nd] exactly as gr_adam_step computes it without penalty and
 * gradient clamp (step size formed in double, epsilon outside the bias correction), and when clamp > 0, z clamped to [-clamp, clamp]. */
typedef struct { double lr, beta1, beta2, eps; } gr_adam_hyper;
int gr_mse_rows_dev(gr_ctx* ctx, const float* x_dev, const float* t_dev, int64_t rows, int64_t n, float* loss_rows_dev, float* grad_dev /*nullable*/);
int gr_adam_rows_step_dev(gr_ctx* ctx, float* z_dev, float* g_dev, float* m_dev, float* v_dev, int64_t rows, int64_t nd, const gr_adam_hyper* /*hyper*/, int t,
                          float clamp, const float* loss_rows_dev, float* best_loss_dev, float* best_z_dev, int update);
int gr_adam_reset(gr_net* net);                             /* OPTSTATE = {adam={R={}}}  train_r.lua:125 */
int gr_adam_get_state(gr_net* net, float* m_host, float* v_host);
int gr_adam_set_state(gr_net* net, const float* m_host, const float* v_host);

/* ---- the other five choices of --D_optmethod / --G_optmethod (train.lua:37-38), dispatched in adversarial.lua:147-161,174-188: the penalty and
 * clamp lines of fevalD / fevalG_on_D (adversarial.lua:86-88,126-128) fused with optim.sgd | adagrad | adadelta | adamax | rmsprop, one launch over the
 * net's flat params, grads and its two state vectors.  The `optim` rock is un-vendored: the update rules are those of the float32 restatements in
 * ganrev/optim.py, in their operation order, bit for bit (penalties summed as gr_adam_step sums them: g + (sign(x) l1 + x l2)).  The penalised, clamped
 * gradient is written back to grads (sgd's weightDecay term is not: the rock adds it to a clone).
 * State: the two vectors are the ones gr_adam_* uses (slot 0 = m, slot 1 = v there).  A method touches only its own slots:
 *     method     slot 0                      slot 1
 *     sgd        dfdx (momentum buffer;      -
 *                untouched at momentum 0)
 *     adagrad    paramVariance               -
 *     adadelta   paramVariance               accDelta
 *     adamax     m                           u
 *     rmsprop    m                           -
 * Changing a net's method (adam included) without a reset in between is the caller's error: the new rule would read the old one's state.
 * Scalars are computed in double and rounded to fp32 once (clr = learningRate / (1 + (t - 1) learningRateDecay), 1 - dampening, 1 - beta1,
 * learningRate / (1 - beta1^t)); 1 - rho and 1 - alpha are fp32 differences of the rounded values, as the mirrors take them. ---- */
enum { GR_OPT_SGD = 1, GR_OPT_ADAGRAD = 2, GR_OPT_ADADELTA = 3, GR_OPT_ADAMAX = 4, GR_OPT_RMSPROP = 5 };
typedef struct {
  int32_t method;                 /* GR_OPT_* */
  int32_t nesterov;               /* sgd: needs momentum > 0 and dampening == 0, else GR_ERR_INVALID */
  double learningRate;            /* rock defaults: sgd, adagrad 1e-3; adamax 2e-3; rmsprop 1e-2 (train.lua:189-190 gives sgd OPT.X_sgd_lr, 0.02); adadelta has none */
  double learningRateDecay;       /* sgd, adagrad: 0 */
  double weightDecay;             /* sgd: 0 */
  double momentum;                /* sgd: 0 (train.lua:189-190: OPT.X_sgd_momentum, 0) */
  double dampening;               /* sgd: the rock defaults it to the momentum - a plain value here, the caller copies momentum into it */
  double rho, eps;                /* adadelta: 0.9, 1e-6 */
  double beta1, beta2;            /* adamax: 0.9, 0.999 */
  double epsilon;                 /* adamax 1e-38, rmsprop 1e-8 */
  double alpha;                   /* rmsprop: 0.99 */
  double l1, l2, clamp;           /* OPT.D_L1 / D_L2 / D_clamp, OPT.G_L1 / G_L2 / G_clamp (train.lua:27-36); 0 = off */
} gr_optim_config;
/* one optim.<method>(feval, PARAMETERS, OPTSTATE.<method>.<net>) call after the closure has left its gradient in grads (adversarial.lua:147-161,174-188);
 * t = 1-based count of steps since the state was reset (sgd, adagrad: evalCounter + 1; adamax: state.t after its increment; at t == 1 sgd's buffer
 * becomes the gradient).  An unknown method, an invalid nesterov request or t < 1 returns GR_ERR_INVALID and launches nothing.  While the context's
 * sticky fault word is set (see "fused_head") the step changes nothing, as gr_adam_step. */
int gr_optim_step(gr_net*, const gr_optim_config* /*config*/, int t);
int gr_optim_reset(gr_net* net);                            /* OPTSTATE = {sgd = {D = {..}, G = {..}}, adagrad = {D = {}, G = {}}, ...}  train.lua:183-193: both slots zero */
int gr_optim_get_state(gr_net* net, float* slot0_host, float* slot1_host);       /* either may be null; what train.lua's OPTSTATE tables hold between batches */
int gr_optim_set_state(gr_net* net, const float* slot0_host, const float* slot1_host);

/* ---- data parallelism (NEW capability required by north_star; the reference is single-GPU, train_r.lua:34,58-62) ---- */
#define GR_COMM_ID_BYTES 128
int gr_comm_unique_id(gr_ctx* ctx, void* id_out /*GR_COMM_ID_BYTES, generated on rank 0, shipped by the host to all ranks*/);
int gr_comm_init(gr_ctx* ctx, const void* id, int nranks, int rank);    /* RCCL communicator over xGMI */
int gr_comm_destroy(gr_ctx* ctx);
int gr_comm_ranks(gr_ctx* ctx, int* nranks, int* rank);
/* Host-exchange hook (tests / bring-up on boxes whose ranks cannot each own a GPU; SURVEY.md section 4: "a fake comm that sums host
 * buffers in-process"): stands in for EVERY collective this context would issue through RCCL - the gradient and loss all-reduce of
 * gr_train_r_step, gr_allreduce_dev, the BatchNorm-statistics exchange of "sync_bn".  fn is called in stream order from inside the
 * library call with a device buffer of `count` elements and must return 0 with the reduction over all ranks in it:
 * kind 0 = fp32 SUM, 1 = fp64 SUM, 2 = uint32 MAX.  It may synchronise (gr_memcpy_d2h / gr_memcpy_h2d on this context are allowed
 * from inside it).  fn = NULL removes the hook.  Mutually exclusive with gr_comm_init. */
typedef int (*gr_exchange_fn)(void* user, void* buf_dev, int64_t count, int kind);
int gr_comm_set_host_exchange(gr_ctx* ctx, int nranks, int rank, gr_exchange_fn fn, void* user);
int gr_allreduce_grads(gr_net* net);                        /* SUM over ranks of the flat gradient; no-op when nranks == 1 */
int gr_allreduce_dev(gr_ctx* ctx, float* buf_dev, int64_t n);
/* all-gather of bytes_per_rank bytes from every rank into recv_dev [nranks x bytes_per_rank], rank order (the sharded search's
 * candidate exchange: apply_r.lua:266-282 over a corpus split across GPUs; one ncclAllGather).  One rank: a copy. */
int gr_allgather_dev(gr_ctx* ctx, const void* send_dev, void* recv_dev, int64_t bytes_per_rank);
int gr_broadcast_params(gr_net* net, int root);             /* make replicas identical before the first step */

/* ---- one whole iteration of train_r.lua:138-170:  images = G:forward(noise) ; R fwd ; MSE ; R bwd ;
 *      [all-reduce] ; L1/L2 + clamp ; Adam.   noise_dev is this rank's shard [batch x nd]; global_batch is the
 *      MSE normaliser's batch (== batch on one GPU).  loss_out receives the (global) un-penalised MSE. ---- */
int gr_train_r_step(gr_net* gnet, gr_net* rnet, const float* noise_dev, int batch, int global_batch,
                    const gr_hyper* h, int t, double* loss_out /*nullable: skipping it avoids a host sync*/);
/* per-phase device times (ms) of the last gr_train_r_step when timing is enabled: [G fwd, R fwd, loss, R bwd, allreduce, adam] */
/* convolution arithmetic (default 2): 1 = "bf16x6": every fp32 operand split into three bf16 terms, six products on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation — fp32-level error (same parity bars), 2.7x the matrix rate;
 * 2 = "f16x3": every operand tensor scaled by a power of two (its device-tracked max|.| -> [2^14, 2^15)) and split into two
 * fp16 terms (22 significand bits), three products on v_mfma_f32_32x32x16_f16, result scaled back exactly — fp32-level
 * error (same parity bars) with half the MFMAs of bf16x6;
 * 0 = exact fp32 on v_mfma_f32_32x32x2_f32.  Also settable with the environment variable GR_CONV_MODE=f32|bf16x6|f16x3 before gr_init. */
int gr_set_conv_mode(gr_ctx* ctx, int mode);
int gr_get_conv_mode(gr_ctx* ctx);
/* Runtime knobs.  These are ALL the keys the shipping library answers (anything else: GR_ERR_INVALID); environment variables read once in gr_init:
 * GR_CONV_MODE (f32 | bf16x6 | f16x3, default f16x3), GR_RANGE_GUARD (0 | 1), GR_SIDE_WGRAD (-1 | 0 | 1), GR_FUSED_HEAD (0 | 1).  Nothing else selects
 * kernels at run time: variants that lost their A/B measurement are not in the sources (docs/HISTORY.md names them).
 *   "p16_min_tiles"  (default 128, process-wide) smallest tile count at which a 3x3 convolution takes the operand-ready (P16) kernels; tests set 1 to
 *                    exercise that path on small shapes
 *   "stack8_min_wgs" (default 128, process-wide) smallest grid at which 8x8 planes are stacked four to a convolution tile; tests force the path
 *   "group_mfma_min_tiles" (default 512, process-wide) smallest number of (image, group) tiles, B x G, at which a GR_GROUPCONV3 stage of 16 planes per group
 *                    and planes up to 32 x 32 takes the f16x3 / bf16x6 MFMA launches (csrc/groupmfma.hip) instead of the fp32 ones; never in f32 mode; tests set 1
 *   "cluster_wide_min_k" (default 33, process-wide) smallest k at which gr_cluster_dev takes its wide kernels (csrc/kmeans.hip) instead of the launches of
 *                    gr_kmeans_dev / gr_cosine_assign_dev / gr_cluster_members_dev; the two routes give the same bits; tests set 1 to compare them - no user knob
 *   "eval_p16"       (default 1) evaluate()-mode stages hand their output to the next convolution operand-ready - see below
 *   "side_wgrad"     (default -1 = by stage size: on from 2^26 activations) R's convolution weight gradients on a second stream beside the rest of backward;
 *                    bit-identical either way (measured: cfg3 -1.1 %, cfg2 +1.1 %: profiles/r05_ab_side_wgrad_*.txt)
 *   "fused_head"     (default 1) gr_train_r_step runs R's last two stages (Linear -> BatchNormalization -> ELU -> Dropout -> Linear [-> Tanh], models.lua:446-454),
 *                    the criterion (train_r.lua:147-151) and their backward in ONE launch where that wins (at most 4 rows per workgroup of 8 features:
 *                    batch <= 256 at 512 features, and nd <= 32); same operations per value as the stage-by-stage path, sums in another order (1e-6 on the
 *                    loss, 1e-4 of a module's largest entry on the gradients: tests/test_gpu_parity.py::test_head_kernel_equals_the_stage_by_stage_step).
 *                    0 = stage by stage: what gr_net_forward_* / gr_net_backward_* compute, bit for bit.  The launch synchronises its C1 / 8 workgroups with
 *                    two grid barriers, so it is only taken on a device with at least that many CUs; a barrier that still times out (~5 s: the CUs were held
 *                    by other work) sets a sticky device word - the optimiser update of that step and of every later one is skipped (parameters and Adam
 *                    state stay those of the last good step) and the next call that synchronises (gr_train_r_step with loss_out, gr_synchronize,
 *                    gr_net_get_params / gr_net_get_grads) returns GR_ERR_STATE once and re-arms the barrier
 *   "head_fault_inject" (default 0; test hook) 1 = the NEXT head launch waits at its barriers for an arrival count that never comes and gives up after 2^10
 *                    polls: the failure path above, on demand (tests/test_gpu_abi_behaviour.py)
 *   "sync_bn"        (default 0) synchronised BatchNorm under data parallelism - see below
 *   "range_guard"    (default 1) the f16x3 range guard - see below */
int gr_set_tuning(gr_ctx* ctx, const char* key, int value);
/* "eval_p16" (default 1; f16x3 arithmetic): in evaluate() mode (apply_r.lua:120-153: MODEL_R:forward on generated images) a stage hands its output to the
 * next 3x3 convolution as that convolution's operand-ready image (fp16 hi / lo vectors written by the convolution epilogue or the pooling stage's pipeline
 * kernel, scaled by an a-priori bound from the weights' per-channel L1 norms and the measured maximum of the stage's input) instead of as an fp32 tensor.
 * Same 1e-4 parity bar; a pure function of the stage's input and parameters (chunks, batch sizes and the host-memory calls agree bit for bit).  0 keeps
 * the fp32 tensors between the stages (gr_net_layer_output can then read them; a gr_net_backward_* after an evaluate()-mode forward needs them). */
/* "sync_bn" (default 0): synchronised BatchNorm under data parallelism (optional).  With a communicator (or the host-exchange
 * hook) on the context, every training-mode BatchNorm adds its per-channel batch sums over the ranks - (sum y, sum y^2) in the forward,
 * (sum dz, sum dz (y - mean)) in the backward, 2 x C doubles each - before it uses them, so that P ranks of B images compute what ONE
 * device computes on P x B images (models.lua:410-448 on the global batch; running statistics identical on every rank).  Default = per-rank
 * statistics (the oracle's "BatchNorm in P groups").  Needs equal shards: gr_train_r_step checks batch x ranks == global_batch. */
/* f16x3 range guard ("range_guard" 1/0 in gr_set_tuning, default on; GR_RANGE_GUARD=0 before gr_init turns it off).  f16x3 scales a
 * tensor by one power of two: an entry 2^k below the tensor maximum keeps about 40 - k bits, and an output channel's relative
 * error grows with the product of the per-channel spreads of the activation and the weight tensor multiplied.  The host-memory calls
 * (gr_net_forward_host / gr_net_backward_host) measure, before computing, the per-channel spread (log2 largest / smallest
 * non-zero channel maximum) of the input / gradOutput, of every weight tensor an f16x3 kernel reads (per input and per output
 * channel) and of the BatchNorm (gamma, beta) pairs, and run the pass on bf16x6 (fp32 exponent range) when the largest
 * activation-side spread (input, gradOutput, BatchNorm pairs) plus the largest weight-side spread exceed 20 bits.  gr_train_r_step scans the parameters every 64th step without synchronising and
 * switches the context to bf16x6 when a scan trips.  Counters: scan launches and passes sent to bf16x6 since gr_init (the
 * latter also in gr_kernel_times as "range_guard_fallback"). */
int gr_range_guard_stats(gr_ctx* ctx, int64_t* scans, int64_t* fallbacks);
/* The device-pointer calls (gr_net_forward_dev / gr_net_backward_dev) are NOT guarded: host loops built from them (the GAN game,
 * adversarial.lua:139-201 mirrored by ganrev.adversarial.DeviceGame) call this every few dozen batches per net: synchronous scan of
 * the net's weights and BatchNorm scales; a hostile spread keeps the context on bf16x6 (as gr_train_r_step's sampled scan does).
 * tripped_out (nullable): 1 when the context's guard has tripped. */
int gr_range_guard_scan_params(gr_net* net, int* tripped_out);
int gr_set_timing(gr_ctx* ctx, int mode /*0 off, 1 per-phase events in gr_train_r_step, 2 per-kernel events*/);
/* mode 2: JSON array of {kernel, phase, launches, total_ms, flops, bytes} (algorithmic flops/bytes) accumulated since it was
 * enabled; phase = the part of gr_train_r_step that launched it ("G forward", "R forward", "loss", "R backward", "adam") or "" */
int gr_kernel_times(gr_ctx* ctx, char* buf, int buflen);
int gr_last_step_times(gr_ctx* ctx, float* ms6);
/* HIP events on the ctx's own stream (a host timer or a torch.cuda.Event on another stream does not see this work):
 * gr_event_record marks slot (0..65535) at the current point of the stream; gr_event_elapsed_ms waits for slot b. */
int gr_event_record(gr_ctx* ctx, int slot);
int gr_event_elapsed_ms(gr_ctx* ctx, int slot_a, int slot_b, float* ms);

/* ---- apply_r.lua:265-282 search loop + apply_r.lua:396-400 cosineSimilarity (nn.CosineDistance) ----
 * For each query row q: score every row j of emb[N x d] (self included) with
 *   w1*sqrt(1/(sum a^2+1e-12) * 1/(sum b^2+1e-12)), order by (score desc, index asc), return the first k.
 * accumulate_in_float selects fp32 instead of the default fp64 row-sum accumulation (TH accreal). */
int gr_cosine_topk_host(gr_ctx* ctx, const float* emb_host, int64_t n, int d, const int64_t* query_rows_host, int q, int k,
                        int64_t* idx_out_host, float* score_out_host, int accumulate_in_float);
int gr_cosine_topk_dev(gr_ctx* ctx, const float* emb_dev, int64_t n, int d, const int64_t* query_rows_host, int q, int k,
                       int64_t* idx_out_host, float* score_out_host, int accumulate_in_float);
/* Search by example: the same search with needle q = row q of queries [q x d], vectors that need not be rows of emb.  Every row of emb is
 * scored (there is no self hit to drop), same order, same k rules (clamped to n; k > 1024: GR_ERR_UNSUPPORTED), same dispatch on (n, d, q, k)
 * and the same overflow rerun.  A needle that equals a table row bit for bit returns what the row-index search of that row returns, indices
 * and score bits.  A zero needle scores 0 against every row: rows 0 .. k-1.  A finite needle whose norm the approximate passes cannot carry (zero,
 * or elements beyond fp16 with 32 or more needles) costs one rerun, not the result.  Non-finite needles are not supported. */
int gr_cosine_topk_queries_dev(gr_ctx* ctx, const float* emb_dev, int64_t n, int d, const float* queries_dev, int q, int k,
                               int64_t* idx_out_host, float* score_out_host, int accumulate_in_float);
int gr_cosine_topk_queries_host(gr_ctx* ctx, const float* emb_host, int64_t n, int d, const float* queries_host, int q, int k,
                                int64_t* idx_out_host, float* score_out_host, int accumulate_in_float);
int gr_cosine_similarity_host(gr_ctx* ctx, const float* a_host, const float* b_host, int d, float* out);
/* Tables of 2^17 rows or more are searched through a bound taken from a strided 16384-row sample (only keys at or above the
 * sample's k-th largest key are kept: same result, bit for bit, without writing n x q keys).  With 32 or more needles (d <= 128)
 * the candidates come from ONE bf16 MFMA GEMM of the table against all needles (approximate cosines, error bound 2^-7 + 2^-10, two
 * cuts with twice that margin) and only they are scored in the exact op order: the result is still bit-identical.  When a table's
 * order defeats the sample (a candidate list overflows) the search runs again on every key.  reruns = how often that
 * happened since gr_init. */
int gr_search_stats(gr_ctx* ctx, int64_t* reruns);

/* ---- apply_r.lua:355-372 (detectAnomalies): out[i] = torch.dist(a[i], b[i]) = sqrt(sum_j (a_ij - b_ij)^2), rows of length d ---- */
int gr_l2_distance_rows_host(gr_ctx* ctx, const float* a_host, const float* b_host, int64_t n, int64_t d, double* out_host);
/* the same kernel on two device-resident tables [n x d] (the images and their fixed versions where embed / G left them); the n distances
 * come back to the host, the call is synchronous.  Bit-identical to gr_l2_distance_rows_host on the same values. */
int gr_l2_distance_rows_dev(gr_ctx* ctx, const float* a_dev, const float* b_dev, int64_t n, int64_t d, double* out_host);

/* ---- The pictures apply_r.lua and sample.lua end in, rendered from device-resident image tables (csrc/render.hip) ----
 *
 * gr_image_grid_dev = image.toDisplayTensor over tiles gathered from up to two tables, with the reference's decorations (apply_r.lua:137,
 * 256,286-297,325-341,346-350,375-388; sample.lua:166-185).  Tables are [n_rows[s] x channels x h x w] fp32, channels 1 or 3.
 *   layout     n_tiles tiles, xmaps = min(nrow, n_tiles) per row, ymaps = ceil(n_tiles / xmaps) rows.  A tile is TH x TW with TH = h + 2 margin,
 *              TW = slots w + 2 margin; a cell is the tile + padding, the tile sits at offset padding / 2 (integer) in its cell; the grid is
 *              GH x GW = ymaps (TH + padding) x xmaps (TW + padding).
 *   tile t     slot s (0 .. slots-1, side by side) shows row rows_host[t slots + s] of src_dev[s]; a row of -1 leaves the tile's background
 *              bg_host[3t ..] (null: 0), which also paints the margin ring (margin 0 or 1): the blue field of fixed_pairs, the black or red
 *              frame of anomalies.  inset_host[t] != 0 (null: none) overwrites the outermost pixel ring of every slot image of the tile with
 *              inset_rgb: the blue frame drawn over the needle of similar_*.
 *   colour     from_space = GR_CS_*: the slot image goes through the toRgb arithmetic of gr_colorspace_* (same device functions), the grid
 *              has 3 channels.  from_space = -1: channels copied as they are, the grid has `channels` channels (fixed_images_*, which skip
 *              toRgb in the reference); backgrounds and inset_rgb then use their first `channels` entries.
 *   range      every pixel inside a tile - image, margin or empty slot - after conversion and decoration is a value v.  auto_range = 0:
 *              lo, hi as given (lo <= hi).  auto_range = 1 (toDisplayTensor without min / max, sample.lua:166-168): lo = min v + 0, hi = max v + 0
 *              over all of them (compare-selects, a NaN never wins; the + 0 makes a zero bound +0), found by a reduction launch.
 *              out = hi == lo ? 0 : (clamp(v, lo, hi) - lo) / (hi - lo)   - compare-select clamp, two subtractions, one division, fp32.
 *              Pixels no tile covers (padding, the unfilled end of the last row) get `fill` as it is.
 *   outputs    grid_dev [Cout x GH x GW] floats and / or u8_dev [GH x GW x Cout] bytes, u8 = (uint8) min(255, max(0, trunc(out * 255 + 0.5)))
 *              (one multiplication, one addition).  This quantisation is this library's choice: the reference writes lossy JPEG, so no byte
 *              parity with its files exists or is claimed.
 * One launch on the ctx stream, two with auto_range; the host arrays are uploaded by the call and are the caller's again when it returns.
 * GR_ERR_INVALID with a gr_last_error message, and no launch, for: slots outside {1, 2}, a null table, both outputs null, channels / from_space
 * that do not fit, h, w, n_tiles, nrow < 1, padding outside [0, 64], margin outside {0, 1}, a row outside [-1, n_rows[s]), lo > hi, a grid
 * beyond 2^28 pixels.
 *
 * gr_rows_mean_dev: out_dev[p] = (((0 + x[rows[0]][p]) + x[rows[1]][p]) + ...) / n for p < d - the average face of a cluster as
 * apply_r.lua:233-243 computes it (face:add per image in list order, one face:div), fp32 throughout; n == 0 writes zeros.  table_dev is
 * [n_rows x d]; a row outside [0, n_rows) returns GR_ERR_INVALID without a launch. ---- */
int gr_image_grid_dev(gr_ctx* ctx, const float* const* src_dev, const int64_t* n_rows, int slots, int channels, int h, int w, int from_space,
                      const int64_t* rows_host, int n_tiles, int nrow, int padding, int margin, const float* bg_host, const uint8_t* inset_host,
                      const float* inset_rgb, float fill, int auto_range, float lo, float hi, float* grid_dev, uint8_t* u8_dev);
int gr_rows_mean_dev(gr_ctx* ctx, const float* table_dev, int64_t n_rows, int64_t d, const int64_t* rows_host, int n, float* out_dev);

/* ---- The trainers' progress pictures: NN_UTILS.imagesToGridTensor + saveImagesAsGrid (utils/nn_utils.lua:490-548) from a device-resident
 * table [n_rows x channels x h x w] fp32 (train.lua:312-314; ganrev/progress.py).  Not image.toDisplayTensor: a fixed grid_h x grid_w
 * grid of cells without padding, seven more pixel rows below them, and the epoch number drawn there.
 *   layout     the grid is GH x GW = (grid_h h + 7) x (grid_w w) and starts as zeros.  Cell t < min(n_show, grid_h grid_w) shows table row
 *              rows_host[t]; cells fill row-major, the top-left corner of cell t is ((t / grid_w) h, (t % grid_w) w).  Later cells and the
 *              seven bottom rows stay 0; entries of rows_host beyond the grid are ignored (and not checked).
 *   colour     as gr_image_grid_dev: from_space = GR_CS_* sends the tile through the toRgb arithmetic of gr_colorspace_* and the grid has 3
 *              channels; from_space = -1 copies the channels as they are.
 *   digits     the decimal digits of epoch, least significant first: digit number p = 1, 2, ... covers rows GH-7 .. GH-3 and columns
 *              GW-2-6p .. GW-6p (0-based), a 3 x 5 block of 0 / 1 written into every channel after the tiles, its zeros included.  The
 *              glyphs are the seven-segment shapes of utils/nn_utils.lua:430-479 ("1" is the right-hand column only).
 *   outputs    grid_dev [Cout x GH x GW] floats, the values as they are (no clamp), and / or u8_dev [GH x GW x Cout] bytes by the
 *              quantisation rule of gr_image_grid_dev with lo = 0, hi = 1: u8 = (uint8) min(255, max(0, trunc(clamp(v, 0, 1) * 255 + 0.5))),
 *              a NaN gives 0.
 * One launch on the ctx stream.  Four pixels of a grid row per thread when w is a multiple of 4 and table_dev / grid_dev are 16-byte,
 * u8_dev 4-byte aligned (16-byte loads and grid stores, the 4 Cout bytes of u8 as Cout words); one pixel per thread otherwise.
 * GR_ERR_INVALID with a gr_last_error message, and no launch, for: a null table, both outputs null, channels / from_space that do not
 * fit, n_rows, h, w, grid_h, grid_w < 1, n_show < 0 (or rows_host null with cells to show), a row outside [0, n_rows) among the rows shown,
 * epoch < 0, digits that do not fit (GW - 2 - 6 ndigits < 0: the reference raises an index error there), a grid beyond 2^28 pixels. ---- */
int gr_progress_grid_dev(gr_ctx* ctx, const float* table_dev, int64_t n_rows, int channels, int h, int w, int from_space,
                         const int64_t* rows_host, int n_show, int grid_h, int grid_w, int epoch, float* grid_dev /*nullable*/, uint8_t* u8_dev /*nullable*/);

/* ---- sample.lua:130-148 findClosestNeighboursOf: the k nearest table rows of each query by torch.dist ----
 * Contract: for each query q [d] and table row x_j [d] (table [n x d], fp32, contiguous)
 *   S(q, j) = sum_{i = 0 .. d-1} (double)(t_i * t_i), t_i = |q_i - x_ji| in fp32, t_i * t_i rounded to fp32 (no fused multiply-add),
 *             summed left to right in fp64;  dist(q, j) = sqrt(S) in fp64
 * (the torch.dist convention of gr_l2_distance_rows_host).  Results are ordered by (dist ascending, row index ascending) and the first k
 * are returned: idx_out_host / dist_out_host [q x k], row-major per query, on the host; the call is synchronous.  k = 1 is sample.lua's
 * loop (its strict < keeps the first minimum).  +inf (fp32 overflow of t * t) is an ordinary value; a NaN distance orders after every
 * number, +inf included.  One divergence: the reference loop starts from row 1's distance, so a NaN there is returned by it, never here.
 * Distances are bit-identical to the sequential fp64 sum, indices those of a full sort.
 * How: one streaming pass sums the same fp32 terms per lane in fp32 and combines the lanes in fp64 (S~, |S~ - S| <= eps S with
 * eps = (T + 2) 2^-24 + (d + 64) 2^-51, T = terms per lane <= 4 ceil(d / 256)); the rows with S~ within that window of a bound on the
 * k-th smallest are re-scored exactly.  Tables of at most 4096 rows, and calls where a candidate list overflows (hundreds of exact
 * copies of the nearest row, a constant table, sums near the fp32 range), score every row exactly instead (kernel "l2_exact_kernel"
 * in gr_kernel_times).  Queries are taken 16 per pass over the table.
 * Limits: 1 <= d <= 65536, 1 <= q <= 64, 1 <= k <= n; null pointers or n <= 0 return GR_ERR_INVALID, k > 128 GR_ERR_UNSUPPORTED.
 * _host uploads the table and the queries; _dev takes both in device memory (16-byte alignment and d % 4 == 0 select 16-byte loads). */
int gr_l2_nearest_host(gr_ctx* ctx, const float* table_host, int64_t n, int64_t d, const float* queries_host, int q, int k,
                       int64_t* idx_out_host, double* dist_out_host);
int gr_l2_nearest_dev(gr_ctx* ctx, const float* table_dev, int64_t n, int64_t d, const float* queries_dev, int q, int k,
                      int64_t* idx_out_host, double* dist_out_host);

/* ---- apply_r.lua:197-217 (createClusterImages): clustering of the recovered noise vectors ----
 * gr_kmeans_host replaces `unsup.kmeans(attributes, nbClusters, nbIterations)` (apply_r.lua:198; un-vendored luarock, restated
 * from memory - see csrc/kmeans.hip): centroids_inout [k x d] carries the INITIAL centroids in (upstream draws them from
 * Torch's RNG and normalises each row) and the final ones out; total_counts_out [k] = members summed over the iterations
 * (upstream's second return value); labels_out [n] (nullable) = assignment of the last iteration.  k <= 32, d <= 256.
 * gr_cosine_assign_host replaces the loop apply_r.lua:205-217: for every row the cosine similarity (nn.CosineDistance op order)
 * to each centroid, keeping the MINIMUM when take_min != 0 - what the reference does (`dist < minDist`), although it names the
 * variable a distance - or the maximum otherwise; ties keep the first centroid. */
int gr_kmeans_host(gr_ctx* ctx, const float* x_host, int64_t n, int d, int k, int niter, float* centroids_inout_host,
                   float* total_counts_out_host, int32_t* labels_out_host);
int gr_cosine_assign_host(gr_ctx* ctx, const float* x_host, int64_t n, int d, const float* centroids_host, int k, int take_min,
                          int32_t* labels_out_host, float* sims_out_host);
/* The clustering on the tables gr_embed_dev wrote (apply_r.lua:197-243).  Every pointer marked _dev is device memory; the work is enqueued
 * on the ctx stream and the calls return without waiting for it; scratch comes from the context.
 * gr_kmeans_dev (apply_r.lua:198) and gr_cosine_assign_dev (apply_r.lua:205-217) are gr_kmeans_host and gr_cosine_assign_host without the
 * copies: the same kernels in the same order, the same bits.  cent_dev [k x d]: initial centroids in, final ones out; totalcounts_dev [k]
 * and labels_dev [n] are nullable (labels_dev is written by the iterations: untouched when niter == 0).  k <= 32, d <= 256, else
 * GR_ERR_UNSUPPORTED.
 * gr_cluster_members_dev (apply_r.lua:218-227: table.sort by similarity, the first nbMaxPerCluster entries): for cluster j < k the
 * min(m, members) rows i with labels_dev[i] == j that have the largest sims_dev[i], ordered by similarity descending (-0 and +0 are equal),
 * ties by ascending row; a NaN similarity ranks after every number, NaNs among themselves by row - the order of a stable argsort of
 * -similarity.  rows_out_dev (int64) and sims_out_dev are [k x m]; slots past the rows written hold -1 and 0.  kept_out_dev [k] = rows
 * written, sizes_out_dev [k] = members of the cluster.  The result is a function of the inputs alone (a sort of distinct keys).
 * 1 <= n < 2^31, k <= 32, m <= 128, else GR_ERR_UNSUPPORTED with a gr_last_error message; labels outside [0, k) belong to no cluster.
 * gr_cluster_faces_dev (apply_r.lua:233-243): out_dev [k x d], row j = gr_rows_mean_dev of rows_dev[j][0 .. kept_dev[j]) over table_dev
 * [n_rows x d] - the fp32 adds in list order, one division by kept_dev[j], bit for bit - all clusters in one launch; zeros for kept_dev[j] == 0.
 * rows_dev is [k x m] int64; the lists are device data, so an entry outside [0, n_rows) is skipped by the kernel (the divisor stays
 * kept_dev[j]) where gr_rows_mean_dev refuses it; kept_dev[j] is clamped to [0, m]. */
int gr_kmeans_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, int k, int niter, float* cent_dev, float* totalcounts_dev /*nullable*/,
                  int32_t* labels_dev /*nullable*/);
int gr_cosine_assign_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, const float* cent_dev, int k, int take_min, int32_t* labels_dev,
                         float* sims_dev);
int gr_cluster_members_dev(gr_ctx* ctx, const int32_t* labels_dev, const float* sims_dev, int64_t n, int k, int m, int64_t* rows_out_dev,
                           float* sims_out_dev, int32_t* kept_out_dev, int32_t* sizes_out_dev);
int gr_cluster_faces_dev(gr_ctx* ctx, const float* table_dev, int64_t n_rows, int64_t d, const int64_t* rows_dev, const int32_t* kept_dev, int k, int m,
                         float* out_dev);
/* gr_cluster_dev: apply_r.lua:198-227 in one enqueue on the ctx stream, for any k up to 4096 - gr_kmeans_dev (cent_dev [k x d]: initial centroids in,
 * final ones out; totalcounts_dev [k] nullable), then gr_cosine_assign_dev on the final centroids (labels_dev / sims_dev [n]: the COSINE assignment,
 * the k-means labels stay in scratch), then gr_cluster_members_dev of those labels (rows_out_dev / sims_out_dev [k x m], kept_out_dev / sizes_out_dev
 * [k]).  Semantics, fill values (-1 / 0), tie and NaN rules are the ones stated above for the three calls; the result is a function of the inputs alone.
 * Limits: 1 <= k <= 4096, d <= 256, 1 <= m <= 128, 1 <= n < 2^31; outside them GR_ERR_UNSUPPORTED with a gr_last_error text that names the value; null
 * pointers (totalcounts_dev excepted), non-positive n, d, k, m or a negative niter GR_ERR_INVALID.  The context stays usable after either.
 * Routes.  k < "cluster_wide_min_k" (default 33), while the k x d fp64 member sums fit the 60 KB of LDS gr_kmeans_dev needs: exactly the launches of the
 * three calls, in their order.  Otherwise the wide kernels, which reproduce those bits wherever both routes apply: per (row, centroid) one sequential
 * fp32 chain in column order, s = s + c[j][t] * x[i][t], multiply and add rounded separately, v = s - c2[j], label = first maximum over ascending j (a row
 * whose scores are NaN: label 0); member sums in fp64 - per block of 512 consecutive rows a cluster's rows in row order from +0.0, the blocks' partials in
 * block order from +0.0, one rounding to fp32, one fp32 division by (float)count; a cluster without a row keeps its centroid and c2.  The rows are grouped
 * by label with a stable counting sort per 512-row block; the m best members are taken from the index grouped by the cosine labels.  No floating-point
 * atomics: two runs agree bit for bit.
 * Scratch comes from the context.  Narrow route: that of the three calls (ceil(n / 512) x k x d doubles).  Wide route: with B = ceil(n / 512) blocks and
 * S = B x min(k, 512) segment slots, S x d doubles + 2 S + 2 B + 512 B + n ints: O(n) index entries, and at most n x d doubles once k >= 512. */
int gr_cluster_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, int k, int niter, float* cent_dev, int take_min, int m,
                   float* totalcounts_dev /*nullable*/, int32_t* labels_dev, float* sims_dev, int64_t* rows_out_dev, float* sims_out_dev,
                   int32_t* kept_out_dev, int32_t* sizes_out_dev);

/* gr_cluster_members_wide_dev: gr_cluster_members_dev's lists - the same rule, fill values, tie and NaN order - for any k up to 4096, by the grouping and
 * member-selection kernels of gr_cluster_dev's wide route (one helper serves both).  sims_dev is any per-row score: a mixture's posteriors rank a
 * component's rows the way similarities rank a cluster's.  Limits: 1 <= k <= 4096, 1 <= m <= 128, 1 <= n < 2^31; outside them GR_ERR_UNSUPPORTED with
 * a gr_last_error text that names the value; null pointers or non-positive n, k, m GR_ERR_INVALID.  Scratch: the index of gr_cluster_dev's wide route,
 * 2 S + 2 B + 512 B ints. */
int gr_cluster_members_wide_dev(gr_ctx* ctx, const int32_t* labels_dev, const float* sims_dev, int64_t n, int k, int m, int64_t* rows_out_dev,
                                float* sims_out_dev, int32_t* kept_out_dev, int32_t* sizes_out_dev);

/* ---- principal axes of a device table (csrc/pca.hip; new: the reference has no counterpart) ----
 * gr_pca_dev: x_dev [n x d] floats -> mean_dev [d] doubles, cov_dev [d x d] doubles (nullable), eigvals_dev [d] doubles (descending),
 * axes_dev [d x d] floats (row a = unit axis a), info_dev [2] int32 (sweeps used, converged flag).  Every pointer is device memory; the work is
 * enqueued on the ctx stream and the call returns without waiting for it; scratch comes from the context.  No floating-point atomics: the result
 * is a function of the inputs alone and does not depend on the device's CU count.
 * Mean (fp64).  Per block of 512 consecutive rows the rows are added in row order from +0.0; the block partials are added in block order from
 * +0.0; one division by n.
 * Covariance, two-pass and centred: C = 1 / (n - 1) sum_r c_r c_r^T with c_rt = (float)((double)x_rt - mean_t), one rounding to fp32.  Per block of
 * 512 rows and element (i, j) one sequential fp32 chain in row order from +0.0, acc = acc + c_ri * c_rj, multiply and add rounded separately
 * (chain length L = 512).  P = 128 partial matrices, a constant of the library: with B = ceil(n / 512) blocks, partial p adds the chains of the
 * blocks floor(p B / P) .. floor((p + 1) B / P) - 1 in block order in fp64 from +0.0 (an empty range leaves +0.0); C_ij = (the partials in order
 * p = 0 .. P - 1 from +0.0, fp64) / (double)(n - 1).  Elements with i <= j are computed and written to [i][j] and [j][i]: both triangles carry the
 * same bits.
 * Eigen-decomposition: cyclic Jacobi in fp64 in ONE workgroup on C, round-robin (circle method) ordering: with m = d + (d & 1) players, round
 * r = 0 .. m - 2 of a sweep rotates the pairs (m - 1, r) and ((r + k) mod (m - 1), (r - k) mod (m - 1)), k = 1 .. m / 2 - 1, all at once (a pair
 * with player d, for odd d, has a bye).  Rotation of the pair (p, q) as listed: tau = (a_qq - a_pp) / (2 a_pq), t = sgn(tau) / (|tau| + sqrt(1 + tau^2)) (sgn(0) = 1),
 * c = 1 / sqrt(1 + t^2), s = t c; a pair whose a_pq is exactly 0 is skipped (a constant column or a diagonal matrix never divides 0 by 0).
 * Stop: off(A)_F^2 <= tau_stop^2 ||C||_F^2 with tau_stop = 2^-46, tested before every sweep (a diagonal C: 0 sweeps), and after at most 30
 * sweeps - then info[1] = 0 and the call still returns GR_OK: the caller decides.  Eigenvalues are the diagonal as computed (a rank-deficient
 * table may give -tiny), ordered descending, ties by ascending column of the final diagonal; axis a is the matching column of V rounded to fp32
 * and signed so that its largest-magnitude fp32 component, the first one among equals, is positive.
 * gr_pca_project_dev: out_dev [n x k] floats, out_ra = sum_t c_rt axes[a][t] for a < k: c_rt as above, per (row, axis) one sequential fp32 chain in
 * column order from +0.0, acc = acc + c_rt * axes[a][t], multiply and add rounded separately.  whiten != 0: column a becomes
 * (float)((double)acc * (1 / sqrt(eigvals[a]))), and 0 where eigvals[a] <= 0 (or NaN).  eigvals_dev may be null when whiten == 0.  16-byte loads
 * when x_dev is 16-byte aligned.
 * Limits: gr_pca_dev 2 <= n < 2^31, 1 <= d <= 256; gr_pca_project_dev 1 <= n < 2^31, 1 <= k <= d <= 256; outside them GR_ERR_UNSUPPORTED with a
 * gr_last_error text that names the value; null pointers (cov_dev excepted) or non-positive n, d, k GR_ERR_INVALID.  The context stays usable
 * after either.  A table whose squared covariances overflow fp64 is outside the contract.
 * Scratch: ceil(n / 512) x d doubles (the mean's block partials) + (P + 2) x d^2 doubles (the partial matrices, A and V): at most 68 MB + n d / 64
 * bytes, whatever the device. */
int gr_pca_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, double* mean_dev, double* cov_dev /*nullable*/, double* eigvals_dev, float* axes_dev,
               int32_t* info_dev);
int gr_pca_project_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, const double* mean_dev, const float* axes_dev, const double* eigvals_dev /*nullable unless whiten*/,
                       int k, int whiten, float* out_dev);

/* ---- diagonal-covariance Gaussian mixture of a device table, fitted by EM (csrc/mixture.hip; new: the reference has no counterpart) ----
 * gr_mixture_dev: x_dev [n x d] floats; weights_dev [k], means_dev [k x d], vars_dev [k x d] floats, the initial parameters in, the fitted ones out;
 * loglik_dev [niter + 1] doubles; labels_dev (int32), post_dev, rowll_dev [n] nullable.  Every pointer is device memory; the work is enqueued on the
 * ctx stream and the call returns without waiting for it; scratch comes from the context.  For t = 0 .. niter - 1 an E-step under the current
 * parameters, which writes loglik[t], then an M-step; one last E-step under the final parameters writes loglik[niter] and the per-row outputs.
 * niter = 0 scores rows under given parameters, which come back bit for bit.
 * Everything past the loads is fp64, every operation rounded on its own (no fused multiply-add); exp and log are the device library's.
 * Log-density.  Once per E-step and component: h_jt = 0.5 / var_jt; c_j = log(w_j) - 0.5 (d log(2 pi) + S_j), S_j the log(var_jt) added in column order
 * from +0.0.  Per (row, component) one chain in column order from +0.0: dl = x_it - mu_jt, e = dl dl, q = q + e h_jt; l_ij = c_j - q.  A component
 * with w_j = 0 has l = -inf: it is dead and adds nothing.
 * Row log-likelihood.  The components form 4 contiguous ranges of ceil(k / 4).  Within a range, in ascending j, the running pair (m, s) from (-inf, 0):
 * l > m: s = s exp(m - l) + 1, m = l, label = j; otherwise, for l > -inf, s = s + exp(l - m).  M = the largest m, the lowest range among equals:
 * labels = its label, the first maximum of l_ij over ascending j; S = the s_g exp(m_g - M) added in range order from +0.0; L_i = M + log(S);
 * post = (float)exp(M - L_i), the responsibility at the label; rowll = (float)L_i.  loglik[t]: per block of 512 consecutive rows the L_i in row order
 * from +0.0, the block partials in block order from +0.0, one division by n.
 * M-step.  r_ij = exp(l_ij - L_i), l_ij by the chain above, 0 where l_ij = -inf.  Per block of 512 rows and (j, t) three chains in row order from +0.0:
 * a1 = a1 + r x; dl = x - mu_jt, e = dl dl, a2 = a2 + r e; an = an + r.  P = 128 partial sets, a constant of the library: with B = ceil(n / 512) blocks,
 * set p adds the chains of the blocks floor(p B / P) .. floor((p + 1) B / P) - 1 in block order from +0.0; S1, S2, N = the sets in order from +0.0.
 * N_j >= 1: mu' = S1 / N; dm = mu' - mu; var' = S2 / N - dm dm - the second moment about the old mean, never sum r x^2 - mu^2 - and var_floor where
 * that is not above it; both rounded to float once.  N_j < 1, less than one row's worth of responsibility: the mean and the variances stay, bit for
 * bit.  w' = (float)(N / n) either way.
 * No floating-point atomics, nothing depends on the CU count or on the order in which workgroups finish: two runs give the same bits, and niter = 3
 * gives the bits of three calls with niter = 1.
 * Limits: 1 <= n < 2^31, 1 <= d <= 256, 1 <= k <= 256; outside them GR_ERR_UNSUPPORTED with a gr_last_error text that names the value; null required
 * pointers, non-positive n, d, k, a negative niter or a var_floor that is not > 0: GR_ERR_INVALID.  The context stays usable after either.  A table or
 * parameters with non-finite elements, or weights that are all 0, are outside the contract (the call still returns).
 * Scratch: n + ceil(n / 512) + k + k d + P k (2 d + 1) doubles: 8 n bytes plus at most 135 MB, whatever the device. */
int gr_mixture_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, int k, int niter, float var_floor, float* weights_dev /*[k] in/out*/,
                   float* means_dev /*[k x d] in/out*/, float* vars_dev /*[k x d] in/out*/, double* loglik_dev /*[niter + 1]*/,
                   int32_t* labels_dev /*[n] nullable*/, float* post_dev /*[n] nullable*/, float* rowll_dev /*[n] nullable*/);

/* ---- silhouette coefficients of a labelled device table (csrc/silhouette.hip; new: the reference has no counterpart) ----
 * gr_silhouette_dev: x_dev [n x d] floats, labels_dev [n] int32; s_dev [n], a_dev, b_dev [n] doubles and nearest_dev [n] int32 (the last three nullable),
 * cluster_mean_dev [k] doubles, sizes_dev [k] int32, mean_dev 1 double.  metric 0: euclidean distance, 1: cosine distance.  Every pointer is device
 * memory; the work is enqueued on the ctx stream and the call returns without waiting for it; scratch comes from the context.
 * Everything past the loads is fp64, every operation rounded on its own (no fused multiply-add); sqrt is the device library's (correctly rounded).
 * Pair distance, euclidean.  t = x_it - x_jt, D = D + t t in column order from +0.0, dist = sqrt(D) - never |x_i|^2 + |x_j|^2 - 2 x_i . x_j, which
 * loses near-duplicate rows and can go negative under the root.
 * Pair distance, cosine.  p = p + x_it x_jt in column order from +0.0; q_i = sqrt(Q_i), Q_i = Q_i + x_it x_it by the same chain, once per row;
 * c = p / (q_i q_j), and 0 where either norm is 0; dist = 1 - c, and 0 where that is not above 0.
 * Per (row i, cluster c): the dist of the members j of c, without i itself, added in ascending row order in one chain from +0.0.  A label outside
 * [0, k) belongs to no cluster, as in gr_cluster_members_dev: such a row is nobody's member and its own outputs are s = a = b = 0, nearest = -1.
 * Per row: a = sum_own / (size_own - 1), and 0 for size_own = 1.  b = the smallest sum_c / size_c over the non-empty clusters c != own, nearest = that
 * c, the first minimum over ascending c; without another member b = 0 and nearest = -1.  s = (b - a) / max(a, b); s = 0 where size_own = 1, where
 * max(a, b) = 0, or where no other cluster has a member.
 * Summaries: sizes[c] = the members of c.  cluster_mean[c] = the members' s added in ascending row order from +0.0, divided by sizes[c]; 0 for an
 * empty cluster.  mean: per block of 512 consecutive rows the s_i in row order from +0.0, the block partials in block order from +0.0, one division
 * by n (rows without a cluster count as 0).
 * No floating-point atomics, nothing depends on the CU count or on the order in which workgroups finish: two runs give the same bits.
 * Limits: 2 <= n <= GR_SILHOUETTE_MAX_N (the pair work is n^2 d), 1 <= d <= 256, 1 <= k <= 4096; outside them GR_ERR_UNSUPPORTED with a gr_last_error
 * text that names the value; null required pointers, non-positive n, d, k or an unknown metric: GR_ERR_INVALID.  The context stays usable after
 * either.  Non-finite elements are outside the contract.
 * Scratch, with B = ceil(n / 512) blocks and S = B x min(k, 512) segment slots: 2 S + 2 B + 512 B + k B + k + 1 + n ints (the grouped index) and
 * n + B doubles (the norms and the mean's partials): at most 13 MB + 12 n bytes, whatever the device. */
#define GR_SILHOUETTE_MAX_N 262144
int gr_silhouette_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, const int32_t* labels_dev, int k, int metric /*0 euclidean, 1 cosine*/,
                      double* s_dev /*[n]*/, double* a_dev /*[n] nullable*/, double* b_dev /*[n] nullable*/, int32_t* nearest_dev /*[n] nullable*/,
                      double* cluster_mean_dev /*[k]*/, int32_t* sizes_dev /*[k]*/, double* mean_dev /*[1]*/);

/* ---- the k-nearest-neighbour graph of a device table, and what is read off it (csrc/knn.hip; new: the reference has no counterpart) ----
 * gr_knn_dev: x_dev [n x d] floats; idx_dev [n x k] int32 and dist_dev [n x k] doubles receive, for every row i, the k rows j != i of smallest
 * distance and those distances, ordered by (distance ascending, j ascending).  metric 0: euclidean distance, 1: cosine distance.  Every pointer is
 * device memory; the work is enqueued on the ctx stream and the call returns without waiting for it; scratch comes from the context.  The graph stays
 * on the device: gr_lof_dev and gr_knn_overlap_dev read it where it lies.
 * Everything past the loads is fp64, every operation rounded on its own (no fused multiply-add); sqrt is the device library's (correctly rounded).
 * The pair distances are gr_silhouette_dev's, operation for operation and bit for bit:
 * Pair distance, euclidean.  t = x_it - x_jt, D = D + t t in column order from +0.0, dist = sqrt(D) - never |x_i|^2 + |x_j|^2 - 2 x_i . x_j.
 * Pair distance, cosine.  p = p + x_it x_jt in column order from +0.0; q_i = sqrt(Q_i), Q_i = Q_i + x_it x_it by the same chain, once per row;
 * c = p / (q_i q_j), and 0 where either norm is 0; dist = 1 - c, and 0 where that is not above 0.
 * Selection.  Row i itself never appears in its list; a duplicate of row i does, at distance 0.  Among equal distances the lower row index comes
 * first, inside the list and at its end: of two rows that tie for the k-th place the lower one is kept.
 * Cost.  All n^2 pairs are visited (the symmetry dist_ij = dist_ji is not used).  The lists cost about k ln(n / k) insertions per row for rows in
 * random order; a table sorted so that every later row is nearer to some row costs that row n k list moves.
 * gr_lof_dev: the local outlier factor of every row of a graph as gr_knn_dev leaves it (idx_dev, dist_dev [n x k]); lrd_dev (nullable) and lof_dev
 * [n] doubles.  kdist_j = dist[j][k - 1]; reach(i, j) = max(kdist_j, dist[i][p]) for the p-th neighbour j of i; m_i = (the k reach values added in
 * list order from +0.0) / k; lrd_i = 1 / (m_i + 1e-10) - the constant keeps a row among k or more exact duplicates finite; lof_i = ((the
 * neighbours' lrd added in list order from +0.0) / k) / lrd_i.  Indices outside [0, n) are outside the contract.
 * gr_knn_overlap_dev: idx_a_dev, idx_b_dev [n x k]: two graphs over the same n rows with the same k.  count_dev [n] int32: how many entries of row i
 * of a occur in row i of b.  mean_dev 1 double: the values count_i / k (one division each), per block of 512 consecutive rows in row order from
 * +0.0, the block partials in block order from +0.0, one division by n.
 * No floating-point atomics, no grid barrier, nothing depends on the CU count or on the order in which workgroups finish: two runs give the same bits.
 * Limits: 2 <= n <= GR_KNN_MAX_N (the pair work is n^2 d in fp64), 1 <= d <= GR_KNN_MAX_D, 1 <= k <= min(n - 1, GR_KNN_MAX_K); outside them
 * GR_ERR_UNSUPPORTED with a gr_last_error text that names the value; null required pointers, non-positive n, d, k or an unknown metric:
 * GR_ERR_INVALID.  Nothing is launched in either case and the context stays usable.  Non-finite elements are outside the contract.
 * Scratch: gr_knn_dev n doubles (the norms; 8 n bytes, at most 2 MB); gr_lof_dev n doubles (lrd); gr_knn_overlap_dev n + ceil(n / 512) doubles. */
#define GR_KNN_MAX_N 262144
#define GR_KNN_MAX_D 256
#define GR_KNN_MAX_K 128
int gr_knn_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, int k, int metric /*0 euclidean, 1 cosine*/, int32_t* idx_dev /*[n x k]*/,
               double* dist_dev /*[n x k]*/);
int gr_lof_dev(gr_ctx* ctx, const int32_t* idx_dev, const double* dist_dev, int64_t n, int k, double* lrd_dev /*[n] nullable*/, double* lof_dev /*[n]*/);
int gr_knn_overlap_dev(gr_ctx* ctx, const int32_t* idx_a_dev, const int32_t* idx_b_dev, int64_t n, int k, int32_t* count_dev /*[n]*/,
                       double* mean_dev /*[1]*/);

/* ---- density-based clustering of a device table: DBSCAN (csrc/density.hip; new: the reference has no counterpart) ----
 * Two calls in the manner of gr_knn_dev and gr_lof_dev: one builds an object that stays on the device, the other reads it there.
 * gr_eps_graph_dev: x_dev [n x d] floats; adj_dev [n x GR_EPS_WORDS(n)] 64-bit words receives the eps-neighbourhood graph as a bitmap: bit j of row i
 * - word j / 64, bit j % 64 - is set iff dist(i, j) <= eps (equality counts); count_dev [n] int32 receives the popcount of every row.  metric 0:
 * euclidean distance, 1: cosine distance.  Every pointer is device memory; the work is enqueued on the ctx stream and the call returns without waiting
 * for it; scratch (n doubles, the cosine norms) comes from the context.
 * dist is gr_silhouette_dev's and gr_knn_dev's pair distance, operation for operation and bit for bit; everything past the loads is fp64, every
 * operation rounded on its own (no fused multiply-add); sqrt is the device library's (correctly rounded):
 * Pair distance, euclidean.  t = x_it - x_jt, D = D + t t in column order from +0.0, dist = sqrt(D).
 * Pair distance, cosine.  p = p + x_it x_jt in column order from +0.0; q_i = sqrt(Q_i), Q_i = Q_i + x_it x_it by the same chain, once per row;
 * c = p / (q_i q_j), and 0 where either norm is 0; dist = 1 - c, and 0 where that is not above 0.
 * The diagonal bit is always set: a row is in its own neighbourhood (as in scikit-learn), so count_i >= 1 counts the row itself.  Bits at and past n
 * in a row's last word are 0.  The chain is symmetric in i and j - x_it - x_jt and x_jt - x_it square to the same bits, the product commutes - so
 * the bitmap is symmetric bit for bit: bit j of row i equals bit i of row j.  All n^2 pairs are visited (the symmetry is not used to halve the work).
 * Because the distances are gr_knn_dev's bits, count_i >= m exactly where column m - 2 of gr_knn_dev's dist (k >= m - 1) is <= eps.
 * gr_dbscan_dev: the labels of DBSCAN read off such a bitmap (adj_dev, count_dev as gr_eps_graph_dev leaves them; one bitmap serves any min_pts).
 * The rule, which is scikit-learn's DBSCAN(metric="precomputed") result exactly:
 *   row i is core iff count_i >= min_pts (the row itself counts);
 *   the clusters are the connected components of the core rows under adj; they are numbered 0, 1, ... in ascending order of their smallest core row;
 *   a row that is not core but has a core row in its neighbourhood is a border row: it takes the lowest cluster number among its core neighbours;
 *   every other row is noise: -1.
 * labels_dev [n] int32; core_dev [n] int32 (nullable) 0 / 1; n_clusters_dev 1 int32.  gr_silhouette_dev scores such a labelling unchanged: a label
 * outside [0, k) is nobody's member.
 * The components come from bounded kernels only: every core row starts with its own index as label; a round gives a wave to every core row, which
 * takes the smallest label m among its core neighbours and, where m is below its own label l, lowers label[l] and label[i] to m by integer
 * atomicMin; a second kernel then replaces every label by the fixed point of label[label[...]] (label[x] <= x always, so the walk descends and ends).
 * Rounds repeat until one changes nothing.  The number of rounds depends on the order the atomics land in, the result does not: the fixed point -
 * every core row carries the smallest core row of its component - is unique.  n - 1 rounds always suffice; a call that has not settled after n
 * rounds returns GR_ERR_STATE with the outputs untouched.
 * UNLIKE ITS NEIGHBOURS, gr_dbscan_dev WAITS ON THE STREAM: once per round, to read whether a label changed (typically a handful of rounds).  The
 * last kernels (border rows, numbering, outputs) are enqueued and not waited for.  Scratch: 2 n int32 and ceil(n / 64) words from the context.
 * No floating-point atomics, no grid barrier, no unbounded spin: two runs give the same bits.
 * Limits: 2 <= n <= GR_DBSCAN_MAX_N (the pair work is n^2 d in fp64; the bitmap is n^2 / 8 bytes: 8 GB at the limit), 1 <= d <= GR_DBSCAN_MAX_D,
 * eps finite and >= 0, 1 <= min_pts <= n; outside the size limits GR_ERR_UNSUPPORTED with a gr_last_error text that names the value; null required
 * pointers, non-positive n, d or min_pts, a negative or non-finite eps or an unknown metric: GR_ERR_INVALID.  Nothing is launched in either case,
 * the outputs are untouched and the context stays usable.  Non-finite elements are outside the contract. */
#define GR_DBSCAN_MAX_N 262144
#define GR_DBSCAN_MAX_D 256
#define GR_EPS_WORDS(n) (((n) + 63) / 64)
int gr_eps_graph_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, double eps, int metric /*0 euclidean, 1 cosine*/,
                     uint64_t* adj_dev /*[n x GR_EPS_WORDS(n)]*/, int32_t* count_dev /*[n]*/);
int gr_dbscan_dev(gr_ctx* ctx, const uint64_t* adj_dev, const int32_t* count_dev, int64_t n, int min_pts, int32_t* labels_dev /*[n]*/,
                  int32_t* core_dev /*[n] nullable, 0/1*/, int32_t* n_clusters_dev /*[1]*/);

/* ---- clustering without an eps: the exact minimum spanning tree on the device, HDBSCAN read off it on the host (csrc/mst.hip, csrc/hdbscan.cpp;
 * new: the reference has no counterpart) ----
 * gr_mst_dev: x_dev [n x d] floats; core_dev nullable, row i's core distance at core_dev[i * core_stride] (core_stride in doubles, >= 1: column
 * k - 1 of a gr_knn_dev dist table is read in place with pointer dist + k - 1 and stride k; column minSamples - 2 is the core distance for
 * DBSCAN's minPts = minSamples, the row itself included); eu_dev, ev_dev [n - 1] int32 and ew_dev [n - 1] doubles receive the tree.  Every pointer
 * but rounds_host is device memory; scratch comes from the context.
 * Weights.  dist_ij is gr_silhouette_dev's, gr_knn_dev's and gr_eps_graph_dev's pair distance, operation for operation and bit for bit; everything
 * past the loads is fp64, every operation rounded on its own (no fused multiply-add); sqrt is the device library's (correctly rounded):
 * Pair distance, euclidean.  t = x_it - x_jt, D = D + t t in column order from +0.0, dist = sqrt(D).
 * Pair distance, cosine.  p = p + x_it x_jt in column order from +0.0; q_i = sqrt(Q_i), Q_i = Q_i + x_it x_it by the same chain, once per row;
 * c = p / (q_i q_j), and 0 where either norm is 0; dist = 1 - c, and 0 where that is not above 0.
 * w_ij = max(dist_ij, core_i, core_j) - the mutual-reachability distance; with core_dev == NULL, w_ij = dist_ij.  Core distances are >= +0.0
 * and finite (negative, -0.0 or non-finite ones are outside the contract), so w is never negative and never -0.0.
 * The tree.  Edges are ordered by the strict total order (w ascending, then min(i, j), then max(i, j)).  Under a strict total order the minimum
 * spanning tree is unique: that tree is the result.  The outputs hold its n - 1 edges with eu < ev, sorted ascending by that same order - a function
 * of the inputs alone, whatever the launch geometry or the order in which workgroups and atomics land.
 * Method: Boruvka rounds from bounded kernels only.  A pair pass finds, for every row i, the smallest edge to a row of another component (all n^2
 * pairs are visited every round; the symmetry is not used); integer atomicMin on the 64-bit pattern of w, then on (lo << 32 | hi) among the rows
 * that hold that w, gives every component its smallest outgoing edge; a component hooks under the component that edge reaches, and where two chose
 * the same edge the lower root emits it and stays; parent pointers are compressed by a walk cut at n steps.  Every round at least halves the
 * component count, so ceil(log2 n) rounds always suffice; a call that has not finished by then returns GR_ERR_STATE with the outputs untouched.  The
 * emitted edges are then ranked by counting (rank = the number of smaller keys; the keys are distinct) and scattered.
 * LIKE gr_dbscan_dev, gr_mst_dev WAITS ON THE STREAM: once per round, to read how many edges are out.  The last kernel (the ranking) is enqueued and
 * not waited for.  rounds_host (nullable, HOST memory) receives the number of rounds.
 * Scratch: 6 n 8-byte words and 3 n + 1 int32 from the context (60 n bytes: 15.7 MB at the limit), each array on a 256-byte boundary.
 * No floating-point atomics, no grid barrier, no unbounded spin: two runs give the same bits.
 * Limits: 2 <= n <= GR_MST_MAX_N (the pair work is n^2 d in fp64, per round), 1 <= d <= GR_MST_MAX_D; outside them GR_ERR_UNSUPPORTED with a
 * gr_last_error text that names the value; null required pointers, non-positive n or d, an unknown metric or core_stride < 1: GR_ERR_INVALID.
 * Nothing is launched in either case, the outputs are untouched and the context stays usable.  Non-finite elements are outside the contract.
 *
 * gr_hdbscan_host: HDBSCAN's labels of a spanning tree as gr_mst_dev leaves it, on the host: no context, no GPU.  eu, ev, ew [n - 1]: a spanning
 * tree over n rows, eu < ev, ew ascending; labels [n] int32 (-1: noise), prob [n] doubles, n_clusters 1 int32: all host memory.
 * The rules are scikit-learn 1.7's HDBSCAN at its defaults (cluster_selection_method="eom", allow_single_cluster=False,
 * cluster_selection_epsilon=0, no max_cluster_size); where the paper and scikit-learn differ, scikit-learn's behaviour is the definition.  All fp64:
 *   hierarchy: the edges are merged in the order given; edge k joins the components of eu[k] (left) and ev[k] (right) into node n + k.
 *   lambda = 1 / w, and +inf at w = 0.
 *   condensed tree: the nodes n + k in descending k, skipping nodes inside a side that has fallen out.  The root is cluster 0, born at lambda 0.
 *     For a node of cluster c whose sides hold L and R rows, m = min_cluster_size: L >= m and R >= m: the left side becomes a new cluster, then the
 *     right one, both born at lambda; one side below m: its rows fall out of c at lambda, the other side goes on as c; both below m: the rows of both
 *     fall out of c at lambda.
 *   stability_c = stability_c + term from +0.0, one term per side that leaves c (a new cluster, or the rows that fall out; s its row count), in
 *     the order above, left before right: term = (lambda - birth_c) * (double)s, and 0 where lambda == birth_c.  lambda_max_c = the largest lambda
 *     among c's terms.
 *   selection (excess of mass): the clusters in descending number (children before parents), the root left out: S = stability_left +
 *     stability_right for a cluster with children; where S > stability_c the cluster is not selected and stability_c = S, else it is selected and
 *     no cluster below it is.  The root is never selected.
 *   label of a row: the selected cluster that the cluster it fell out of is, or lies under; -1 without one.
 *   prob of a row: q = min(lambda_row, lambda_max_C) / lambda_max_C for its selected cluster C, and 1 where q is not finite; 0 for a row of -1.
 *   Clusters are numbered 0, 1, ... in ascending order of their smallest member row.
 * Among equal weights the merge order is the order given (gr_mst_dev's: by (lo, hi)); another implementation may merge ties in another order.
 * GR_ERR_INVALID with the outputs untouched for: a null pointer, n < 2 (or above 2^30), min_cluster_size outside [2, n], an index outside [0, n),
 * eu >= ev, a weight that is negative or not finite, weights not ascending, edges that close a cycle.
 * Not built: `leaf` selection, allow_single_cluster, GLOSH outlier scores, prediction for new rows. */
#define GR_MST_MAX_N 262144
#define GR_MST_MAX_D 256
int gr_mst_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, int metric /*0 euclidean, 1 cosine*/, const double* core_dev /*nullable*/,
               int64_t core_stride /*in doubles, >= 1*/, int32_t* eu_dev, int32_t* ev_dev, double* ew_dev /*[n - 1] each*/,
               int32_t* rounds_host /*nullable*/);
int gr_hdbscan_host(const int32_t* eu, const int32_t* ev, const double* ew, int64_t n, int min_cluster_size, int32_t* labels /*[n], -1 noise*/,
                    double* prob /*[n]*/, int32_t* n_clusters);

/* ---- the sampling layer of a variational autoencoder (csrc/vae.hip; new: the reference has no counterpart) ----
 * The layer between an encoder whose head emits a mean and a log-variance and a decoder: the reparameterisation z = mu + exp(logvar / 2) eps, its KL
 * term against the unit Gaussian, and the backward of both.  h [B x 2 nd] floats: columns 0 .. nd - 1 of a row hold mu, columns nd .. 2 nd - 1 hold
 * logvar; eps, z and gz are [B x nd], gh is [B x 2 nd].  A null eps is eps = 0 (z = mu: the encoder's mean, with the KL of the row as a score).
 * The _dev calls take device pointers, enqueue on the ctx stream and return without waiting; the _host calls take host pointers, stage them, run
 * the same kernels and wait: the same bits.
 * Everything past the loads is fp64, every operation rounded on its own (no fused multiply-add); exp is the device library's.
 * Forward.  s = exp(0.5 lv); se = s eps; z = (float)(mu + se).  Element KL: mm = mu mu, ss = s s, a = mm + ss, b = a - 1, d = b - lv, k = 0.5 d.
 * kl_rows[i] = (float)K_i, K_i the k of row i added in column order from +0.0.  kl[0], the mean over rows: per block of 512 consecutive rows the K_i
 * (fp64, not the rounded kl_rows) in row order from +0.0, the block partials in block order from +0.0, one division by B.
 * Backward, for the loss recon + kl_weight mean_i K_i, gz = d recon / d z.  c = kl_weight / B, one fp64 division; s as in forward;
 * gmu = (float)(gz + c mu); glv = (float)((gz eps) (0.5 s) + c (0.5 (s s - 1))); gh = (gmu | glv) in h's layout.
 * No floating-point atomics, nothing depends on the CU count: two runs give the same bits.  16-byte loads and stores are used when nd % 4 == 0 and
 * every pointer is 16-byte aligned, scalar ones otherwise: the same bits either way.
 * Limits: 1 <= nd <= 256 (GR_VAE_MAX_ND), 1 <= B < 2^31; outside them GR_ERR_UNSUPPORTED with a gr_last_error text that names the value; null required
 * pointers or non-positive B, nd: GR_ERR_INVALID.  Nothing is launched in either case and the context stays usable.  Finite inputs with
 * |logvar| <= 80 are the contract; beyond that the call still returns.
 * Scratch (only when kl is asked for): B + ceil(B / 512) doubles from the context. */
#define GR_VAE_MAX_ND 256
int gr_vae_sample_dev(gr_ctx* ctx, const float* h_dev, const float* eps_dev /*nullable: eps = 0*/, int64_t B, int nd, float* z_dev,
                      float* kl_rows_dev /*[B] nullable*/, double* kl_dev /*1 double, nullable*/);
int gr_vae_sample_backward_dev(gr_ctx* ctx, const float* h_dev, const float* eps_dev /*nullable: eps = 0*/, const float* gz_dev, int64_t B, int nd,
                               double kl_weight, float* gh_dev /*[B x 2 nd]*/);
int gr_vae_sample_host(gr_ctx* ctx, const float* h, const float* eps /*nullable*/, int64_t B, int nd, float* z, float* kl_rows /*nullable*/,
                       double* kl /*nullable*/);
int gr_vae_sample_backward_host(gr_ctx* ctx, const float* h, const float* eps /*nullable*/, const float* gz, int64_t B, int nd, double kl_weight,
                                float* gh);

/* ---- image-to-image scores: the structural similarity index and the mean squared error (csrc/quality.hip; new: the reference has no counterpart) ----
 * gr_ssim_dev: a_dev, b_dev [n x channels x h x w] floats -> ssim_rows_dev [n] floats, the SSIM of Wang et al. 2004 per image over the valid window
 * positions (no padding); mse_rows_dev [n] floats (nullable), the mean squared error per image from the same pass; ssim_mean_dev (1 double, nullable), the
 * mean of the per-image SSIM.  Every pointer is device memory; the work is enqueued on the ctx stream and the call returns without waiting for it;
 * scratch comes from the context.  gr_ssim_host takes host pointers, stages them once, runs the same kernels and waits: the same bits.
 * Everything past the loads is fp64, every operation rounded on its own (no fused multiply-add): var = sum w x^2 - mu^2 cancels, and fp32 window sums
 * lose 4.5e-5 of the index on a flat bright image.  With x = a, y = b (a float enters by an exact conversion, a product of two floats is exact):
 * Window.  sigma > 0: e[i] = exp(-(d d) / (2 (sigma sigma))), d = i - (win - 1) / 2, i = 0 .. win - 1, the host's exp; E = the e[i] added in index order
 * from +0.0; g[i] = e[i] / E.  sigma <= 0: the uniform window g[i] = 1 / win.  The 2-D window is g (x) g, applied as two 1-D passes.
 * Constants.  C1 = k1 k1, k1 = 0.01 data_range; C2 = k2 k2, k2 = 0.03 data_range.
 * Horizontal.  Per channel, input row i and valid column c (ow = w - win + 1 of them), five chains over t = 0 .. win - 1 from +0.0:
 * H = H + g[t] q[i][c + t], for q = x, y, x x, y y, x y.
 * Vertical.  Per valid position (r, c) (oh = h - win + 1 rows), five chains over t from +0.0: V = V + g[t] H[r + t][c], giving mx, my, sxx, syy, sxy.
 * Position.  mxx = mx mx, myy = my my, mxy = mx my; vx = sxx - mxx, vy = syy - myy, cxy = sxy - mxy; n1 = 2 mxy + C1, n2 = 2 cxy + C2,
 * d1 = (mxx + myy) + C1, d2 = (vx + vy) + C2; S = (n1 n2) / (d1 d2).  The x and y chains are the same instruction sequence and every operation that
 * mixes them is commutative: swapping a and b gives the same bits, and a == b gives n1 == d1 and n2 == d2 bit for bit, so S == 1.0 exactly.
 * Image.  R_r = the S of row r added in column order from +0.0; P_ch = the R_r of channel ch in row order from +0.0; Q = the P_ch in channel order
 * from +0.0; q = Q / (channels oh ow), one division; ssim_rows[i] = (float)q.  mse_rows[i] is formed the same way over every pixel: e = d d, d = x - y;
 * rows of e in column order, the rows in row order, the channels in channel order, one division by channels h w, one rounding to float.
 * Mean.  ssim_mean[0]: per block of 512 consecutive images the q (fp64, not the rounded ssim_rows) in image order from +0.0, the block partials in
 * block order from +0.0, one division by n.
 * No floating-point atomics, nothing depends on the CU count or on how many rows of an image the kernel holds at a time: two runs give the same bits.
 * 16-byte loads are used when w % 4 == 0 and both tables are 16-byte aligned, scalar ones otherwise: the same bits either way.
 * Limits: win odd, 3 <= win <= GR_SSIM_MAX_WIN (11), win <= min(h, w), h, w <= GR_SSIM_MAX_HW (128), channels >= 1, 1 <= n < 2^31, data_range > 0 (a NaN is
 * refused too); anything else, and a null a, b or ssim_rows, is GR_ERR_INVALID with a gr_last_error text that names the value, before any launch; the
 * context stays usable.  Non-finite pixels are outside the contract (the call still returns).  a and b may be the same table.
 * Scratch (only when ssim_mean is asked for): n + ceil(n / 512) doubles from the context. */
#define GR_SSIM_MAX_WIN 11
#define GR_SSIM_MAX_HW 128
int gr_ssim_dev(gr_ctx* ctx, const float* a_dev, const float* b_dev, int64_t n, int channels, int h, int w, int win, double sigma, double data_range,
                float* ssim_rows_dev /*[n]*/, float* mse_rows_dev /*[n] nullable*/, double* ssim_mean_dev /*1 double, nullable*/);
int gr_ssim_host(gr_ctx* ctx, const float* a, const float* b, int64_t n, int channels, int h, int w, int win, double sigma, double data_range,
                 float* ssim_rows /*[n]*/, float* mse_rows /*[n] nullable*/, double* ssim_mean /*nullable*/);

/* ---- exact (dense) t-SNE of a device table (csrc/tsne.hip; new: the reference has no counterpart) ----
 * A two-dimensional, neighbour-preserving map of up to GR_TSNE_MAX_N rows: the joint matrix is n x n floats (1 GiB at the cap).  Barnes-Hut,
 * FFT interpolation and sparse affinities are out of scope.  Every pointer is device memory; the work is enqueued on the ctx stream and the calls
 * return without waiting for it; scratch comes from the context.  No floating-point atomics, nothing depends on the CU count: two runs give the
 * same bits.
 * gr_tsne_affinities_dev: x_dev [n x d] floats -> p_dev [n x n] floats, beta_dev [n] doubles (nullable), info_dev [2] int32 (the largest number
 * of updates of beta any row needed; the rows that still missed the tolerance after 50).
 *   D_ij = sum_k t_k^2 with t_k = (double)x_ik - (double)x_jk (exact), fp64, in column order from +0.0, multiply and add rounded separately; never
 *   the |x|^2 + |y|^2 - 2xy form.  m_i = min_{j != i} D_ij, r_j = D_ij - m_i.
 *   Per row the bisection of van der Maaten's reference code on beta, fp64: beta = 1; S = sum_{j != i} e_j and T = sum_{j != i} r_j e_j with
 *   e_j = exp(-beta r_j); H = log(S) + beta T / S; stop when |H - log(perplexity)| <= 1e-5 or after 50 updates; H too large: the lower side is
 *   beta, beta <- beta * 2 while the upper side is unbounded, else the midpoint; H too small: the mirror image with beta / 2.  Order of S and T:
 *   thread t of 1024 adds its columns j = t, t + 1024, ... in that order from +0.0, then the tree t += t + o, o = 512 .. 1.
 *   c_ij = (float)(e_j / S), c_ii = 0; p_ij = p_ji = (float)(((double)c_ij + (double)c_ji) / (double)(2 n)): symmetric bit for bit, zero diagonal.
 *   Scratch: n d floats (the table transposed).
 * gr_tsne_gradient_dev: p_dev, y_dev [n x 2] floats -> grad_dev [n x 2] floats, z_dev [1] double (nullable).  fp32, each operation rounded:
 *   dx = y_i0 - y_j0, dy = y_i1 - y_j1, w_ij = 1 / (1 + (dx dx + dy dy)).  fp64 from there: A_i = sum_j ((double)p_ij w) (dx, dy),
 *   B_i = sum_j (w w) (dx, dy), Z_i = sum_{j != i} w; Z = sum_i Z_i; g_i = (float)(4 (e A_i - B_i / Z)).  One pass reads P once.  Order of a row's
 *   sums: a workgroup of 256 threads owns 8 consecutive rows; thread t adds its columns j = t, t + 256, ... in that order from +0.0; within a wave
 *   v += v[lane + o] for o = 32, 16, 8, 4, 2, 1; then ((wave 0 + wave 1) + wave 2) + wave 3.  Order of Z: thread t of 256 adds Z_t, Z_(t + 256), ...
 *   from +0.0, then the tree t += t + o, o = 128 .. 1.  Scratch: 5 n doubles.
 * gr_tsne_update_dev: the delta-bar-delta rule of the reference implementation, elementwise fp32, each operation rounded, over y, inc, gains
 *   [n x 2]: sign(v) = 1, -1 or 0 (for +-0); gains = sign(g) == sign(inc) ? gains * 0.8f : gains + 0.2f; gains = min_gain where it is below;
 *   inc = momentum * inc - (eta * gains) * g; y = y + inc.  Then the column mean, fp64: per block of 512 consecutive rows the rows in row order
 *   from +0.0, the block partials in block order from +0.0, one division by n; y = (float)((double)y - mean).
 * gr_tsne_kl_dev: kl_dev [1] double = sum_{p_ij > 0} p_ij log(p_ij Z / w_ij), computed as sum_i K_i + log(Z) sum_i P_i with
 *   K_i = sum_{p_ij > 0} (double)p_ij (log((double)p_ij) - log((double)w_ij)), P_i = sum_j p_ij, Z as above; w in fp32 as above, the rest fp64, the
 *   orders of the gradient.  p_dev is the joint matrix as gr_tsne_affinities_dev wrote it (no exaggeration).
 * gr_tsne_run_dev: iterations t = first_iter .. first_iter + iters - 1 on the stream without a host synchronisation, each the launches of
 *   gr_tsne_gradient_dev with e = (t < stop_lying_iter ? exaggeration : 1) and gr_tsne_update_dev with (t < mom_switch_iter ? momentum0 :
 *   momentum1), eta and min_gain: the same bits as those calls.  kl_every > 0 and kl_dev given: after every iteration t with (t + 1) % kl_every
 *   == 0 the KL of gr_tsne_kl_dev goes to kl_dev[(t + 1) / kl_every - 1], so kl_dev holds (first_iter + iters) / kl_every doubles.
 * gr_map_cells_dev: y_dev [n x 2] floats -> rows_out_dev [grid_h x grid_w] int64, the row nearest to each cell's centre (ties: the lower row;
 *   an empty cell: -1), counts_dev [grid_h x grid_w] int32 (nullable) the rows per cell.  Bounding box lo, hi per axis by compare-selects; axis 0
 *   runs along grid_w, axis 1 along grid_h, cell index = cell_1 * grid_w + cell_0.  fp32, each operation rounded: cell = min(G - 1,
 *   (int)(((v - lo) / (hi - lo)) * (float)G)), 0 when hi == lo; centre = lo + ((float)cell + 0.5f) * ((hi - lo) / (float)G); distance =
 *   da da + db db.  One 64-bit unsigned integer atomicMin per row on the key (distance bits << 32 | row): order-independent.  Scratch: 8 bytes per
 *   cell.
 * Limits: null pointers (the nullable ones excepted), n < 4 (affinities; n < 1 elsewhere), d < 1, a perplexity outside [1, (n - 1) / 3], a grid
 * side < 1 or negative iteration counts: GR_ERR_INVALID.  n > GR_TSNE_MAX_N (gr_map_cells_dev: n >= 2^31, a grid side > 1024):
 * GR_ERR_UNSUPPORTED with a gr_last_error text that names the value.  Nothing is launched and no output is touched in either case; the context
 * stays usable. */
#define GR_TSNE_MAX_N 16384
typedef struct {
  float exaggeration;        /* the factor on P during the early iterations (12) */
  int32_t stop_lying_iter;   /* iterations t < stop_lying_iter run exaggerated (250) */
  float momentum0, momentum1; /* before and from mom_switch_iter (0.5, 0.8) */
  int32_t mom_switch_iter;   /* (250) */
  float eta, min_gain;       /* learning rate; floor of the gains (0.01) */
} gr_tsne_config;
int gr_tsne_affinities_dev(gr_ctx* ctx, const float* x_dev, int64_t n, int d, double perplexity, float* p_dev, double* beta_dev /*nullable*/,
                           int32_t* info_dev);
int gr_tsne_gradient_dev(gr_ctx* ctx, const float* p_dev, const float* y_dev, int64_t n, float exaggeration, float* grad_dev, double* z_dev /*nullable*/);
int gr_tsne_update_dev(gr_ctx* ctx, float* y_dev, const float* grad_dev, float* inc_dev, float* gains_dev, int64_t n, float eta, float momentum,
                       float min_gain);
int gr_tsne_kl_dev(gr_ctx* ctx, const float* p_dev, const float* y_dev, int64_t n, double* kl_dev);
int gr_tsne_run_dev(gr_ctx* ctx, const float* p_dev, int64_t n, const gr_tsne_config* /*config*/, float* y_dev, float* inc_dev, float* gains_dev,
                    int first_iter, int iters, double* kl_dev /*nullable*/, int kl_every);
int gr_map_cells_dev(gr_ctx* ctx, const float* y_dev, int64_t n, int grid_h, int grid_w, int64_t* rows_out_dev, int32_t* counts_dev /*nullable*/);

/* ---- device memory helpers for hosts without a tensor library (LuaJIT FFI, ctypes) ---- */
int gr_malloc(gr_ctx* ctx, int64_t bytes, void** out_dev);
int gr_free(gr_ctx* ctx, void* dev);
int gr_memcpy_h2d(gr_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes);
int gr_memcpy_d2h(gr_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes);
/* fill a device buffer with N(0,1) (Philox + Box-Muller): synthetic createNoiseInputs (utils/nn_utils.lua:39-51) for benches */
int gr_fill_normal_dev(gr_ctx* ctx, float* dst_dev, int64_t n, uint64_t seed);
/* the other noise method of createNoiseInputs (utils/nn_utils.lua:44-45): uniform(lo, hi), lo = -1, hi = 1 in the reference */
int gr_fill_uniform_dev(gr_ctx* ctx, float* dst_dev, int64_t n, float lo, float hi, uint64_t seed);

/* ---- nn.Concat (models.lua:293-321, the D network) on device-resident tensors.  The container itself stays host code: it calls
 * its branches' gr_net_forward_dev / gr_net_backward_dev; these move its data without leaving the GPU (ctx stream, asynchronous).
 * gr_copy2d_dev: `rows` rows of `cols` floats between two row-major matrices (pitches in floats): a branch output [B x k] into
 * columns of the joined [B x sum k] output, or a column range of gradOutput into a contiguous [B x k] slice.
 * gr_add_dev: y += x, the sum of the branches' gradInputs (nn.Concat:updateGradInput). */
int gr_copy2d_dev(gr_ctx* ctx, float* dst_dev, int64_t dst_pitch, const float* src_dev, int64_t src_pitch, int64_t rows, int64_t cols);
int gr_add_dev(gr_ctx* ctx, float* y_dev, const float* x_dev, int64_t n);

/* ---- NN_UTILS.switchColorSpace(images, from, to) = rgbToColorSpace(toRgb(images, from), to)  (utils/nn_utils.lua:133-246;
 * pretrain_with_previous_net.lua:167,182; dataset.lua:153).  NCHW fp32, [batch x planes x h x w]: GR_CS_Y has 1 plane, the others 3.
 * One launch: the rgb intermediate is never written, and the result is bit-identical to from -> rgb followed by rgb -> to (each step
 * rounds to fp32 as its own call would).  rgb -> rgb is the only pass-through (no launch; out = a copy of in when the pointers differ);
 * y -> y, yuv -> yuv and hsl -> hsl DO go through rgb, as the reference does (y -> y yields 0.21y + 0.72y + 0.07y).
 * rgb -> y is nn_utils.rgb2y's mixture (:221-246), not image.rgb2y.  The yuv and hsl arithmetic restates Torch's `image` rock (DESIGN.md
 * section 1).  in == out is allowed when both spaces have the same plane count.  A bad from / to, batch, h or w <= 0, a null pointer, or
 * in == out with different plane counts return GR_ERR_INVALID and leave out untouched. ---- */
enum { GR_CS_RGB = 0, GR_CS_Y = 1, GR_CS_YUV = 2, GR_CS_HSL = 3 };
int gr_colorspace_dev(gr_ctx* ctx, const float* in_dev, int from, int to, int64_t batch, int h, int w, float* out_dev);
int gr_colorspace_host(gr_ctx* ctx, const float* in_host, int from, int to, int64_t batch, int h, int w, float* out_host);

/* ---- dataset.lua:99-173: what loadImages / loadRandomImages do to every file after decoding it (csrc/dataset.hip) ----
 *
 * gr_image_scale_* = image.scale(src, width, height) in its default bilinear mode on fp32 NCHW [n x planes x sh x sw] -> [n x planes x dh x dw]
 * (dataset.lua:112,150).  The arithmetic restates the un-vendored `image` rock's scaleBilinear FROM MEMORY and is unpinned, like the yuv / hsl
 * arithmetic above.  Per plane the row pass runs first - every source row from sw to dw values, each rounded to fp32 -
 * then the column pass maps every column of that intermediate from sh to dh.  Each pass is scaleLinear_rowcol(src_len, dst_len); all variables
 * fp32, one IEEE operation per step (no fused multiply-add, `/` correctly rounded), in this order:
 *   dst_len == src_len   copy
 *   dst_len >  src_len   src_len == 1 replicates the value; else scale = (float)(src_len - 1) / (float)(dst_len - 1);
 *                        for di < dst_len - 1:  f = di * scale; i = (long)f; f -= i; dst[di] = (1 - f) * src[i] + f * src[i + 1];
 *                        dst[dst_len - 1] = src[src_len - 1]
 *   dst_len <  src_len   (fractional box average) scale = (float)src_len / (float)dst_len; (i0, f0) = (0, 0); for each di:
 *                        f1 = (di + 1) * scale; i1 = (long)f1; f1 -= i1;  acc = (1 - f0) * src[i0]; n = 1 - f0;
 *                        for s = i0 + 1 .. i1 - 1: acc += src[s]; n += 1;   if i1 < src_len: acc += f1 * src[i1]; n += f1;
 *                        dst[di] = acc / n; (i0, f0) = (i1, f1)
 *                        ((i0, f0) before output di is the split of (float)di * scale: a thread computes its own span in closed form)
 * One launch; the intermediate is never written.  in == out is not supported.
 *
 * gr_dataset_images_dev = the loader's fused path, one launch per batch of decoded files: uint8 interleaved HWC [n x sh x sw x sc] in device
 * memory -> fp32 NCHW [n x planes(to_space) x dh x dw].  sc = 1 (grey, replicated to three channels), 3, or 4 (alpha dropped): what
 * image.load(fp, 3, "float") yields (dataset.lua:149).  Per pixel: v = (float)byte / 255.0f (correctly rounded); the two scale passes above;
 * rgbToColorSpace(to_space) by the device functions of gr_colorspace_*; if normalize != 0, NN_UTILS.normalize as the live code has it
 * (utils/nn_utils.lua:371-375): v * 2, + (-1), clamp to [-1, 1] by compare-selects.  Bit-identical to the unfused chain bytes -> / 255 planar,
 * gr_image_scale_dev, gr_colorspace_dev(rgb -> to_space), normalise.
 *
 * GR_ERR_INVALID with a gr_last_error message, no launch and `out` untouched for: a null pointer; n, planes, sh, sw, dh or dw < 1; sc outside
 * {1, 3, 4}; a bad to_space; in == out (gr_image_scale_*).  Limits of the index arithmetic: every side at most 32768 (the fp32 products
 * di * scale then stay exact enough that no index leaves its row), and at most 2^40 elements in the input and in the output tensor. ---- */
int gr_image_scale_dev(gr_ctx* ctx, const float* in_dev, int64_t n, int planes, int sh, int sw, int dh, int dw, float* out_dev);
int gr_image_scale_host(gr_ctx* ctx, const float* in_host, int64_t n, int planes, int sh, int sw, int dh, int dw, float* out_host);
int gr_dataset_images_dev(gr_ctx* ctx, const uint8_t* in_dev, int64_t n, int sh, int sw, int sc, int dh, int dw, int to_space, int normalize,
                          float* out_dev);

/* ---- a dataset's decoded files, kept on the device (csrc/ops.hip, csrc/dataset.hip; ganrev.dataset.cache) ----
 *
 * A run draws from the same files epoch after epoch.  The cache holds each file's bytes as the file stores them - uint8, interleaved HWC,
 * at source size, sc = 1, 3 or 4 channels - and gr_dataset_cache_load_dev turns any list of them into the fp32 table in ONE launch: row k of
 * out_dev [n x planes(to_space) x dh x dw] is, bit for bit, what gr_dataset_images_dev writes for image indices_host[k] alone (the
 * arithmetic stated above: / 255, the two scale passes, rows first, rgbToColorSpace, the optional normalise step).  Source size and channel
 * count vary from image to image inside the launch, an image may be listed several times, and the order is free.
 *
 * The handle (`cache`, an opaque pointer) belongs to one context and follows the rule of a gr_net: gr_dataset_cache_destroy waits for the
 * context's stream and frees what the cache holds; it is called before gr_shutdown of that context, never after.
 * gr_dataset_cache_create: chunk_bytes <= 0 takes the default (64 MB).  The arena grows by chunks of that size, one device allocation each;
 * bytes that were uploaded are never copied again, and an image larger than a chunk gets a chunk of its own.
 * gr_dataset_cache_append uploads one image (the caller's array is its own again on return); its number is the append order, from 0.  A failed
 * device allocation returns GR_ERR_HIP and the cache stays usable with the images it holds.
 * gr_dataset_cache_size: the number of images and their decoded bytes.  gr_dataset_cache_image: the record of image i (any out pointer may be null).
 * gr_dataset_cache_load_dev is enqueued on the context's stream like every operator: it uploads the index list and launches; it waits for the
 * stream only in the first load after an append, which brings the device copy of the records up to date.
 *
 * GR_ERR_INVALID with a gr_last_error message, no launch and `out` untouched for: a null pointer; n < 1; an index outside [0, n_images);
 * dh or dw < 1; a side above 32768 (source or target); sc outside {1, 3, 4}; a bad to_space; more than 2^40 elements in the table. ---- */
int gr_dataset_cache_create(gr_ctx* ctx, int64_t chunk_bytes, void** cache_out);
int gr_dataset_cache_destroy(void* cache);
int gr_dataset_cache_append(void* cache, const uint8_t* bytes_host, int sh, int sw, int sc);
int gr_dataset_cache_size(void* cache, int64_t* n_images, int64_t* bytes);
int gr_dataset_cache_image(void* cache, int64_t i, int* sh, int* sw, int* sc);
int gr_dataset_cache_load_dev(void* cache, const int64_t* indices_host, int64_t n, int dh, int dw, int to_space, int normalize, float* out_dev);

/* ---- single-kernel entry points used by bench.py's roofline leg and by kernel-level parity tests ---- */
int gr_conv3_forward_dev(gr_ctx* ctx, const float* in_dev, const float* w_dev, const float* bias_dev, float* out_dev,
                         int batch, int cin, int cout, int h, int w, int upsample2);
int gr_conv3_backward_data_dev(gr_ctx* ctx, const float* gout_dev, const float* w_dev, float* gin_dev,
                               int batch, int cin, int cout, int h, int w);
int gr_conv3_backward_weight_dev(gr_ctx* ctx, const float* in_dev, const float* gout_dev, float* gw_dev /*+=*/,
                                 int batch, int cin, int cout, int h, int w);
/* times `iters` launches of the dominant conv kernel (R.conv2 shape by default) with HIP events on the ctx stream */
int gr_bench_conv3(gr_ctx* ctx, int which /*0 fwd,1 bwd-data,2 bwd-weight*/, int batch, int cin, int cout, int h, int w,
                   int iters, float* avg_ms_out);

/* sustained fp32-accurate TFLOP/s of the bare f16x3 inner loop (operands re-read from LDS, three fp16 MFMA products per accumulate, two
 * waves per SIMD, random data) on this device, after a warm-up under load: what the chip's clock under MFMA load leaves of the 833
 * TFLOP/s spec ceiling.  shape 0 = v_mfma_f32_32x32x16_f16 (the convolution kernels' instruction), 1 = v_mfma_f32_16x16x32_f16. */
int gr_bench_mfma_loop(gr_ctx* ctx, int shape, int launches, float* tflops_out);

#ifdef __cplusplus
}
#endif
#endif
