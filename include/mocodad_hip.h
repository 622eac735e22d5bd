/*
 * mocodad_hip.h — C ABI of the MI355X-native MoCoDAD anomaly-scoring path (libmocodad_hip.so).
 *
 * The reference (aleflabo/MoCoDAD) is pure Python/PyTorch and has no FFI; the seam it offers is the
 * Python module surface of models/mocodad.py.  These entry points are what a maintainer binds with
 * ctypes from that surface; each cites the reference code it replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MCD_E* code; mcd_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI.
 *   - the CALLER owns every buffer (device pointers unless stated "host"); the library owns only
 *     mcd_weights_t.  All tensors are dense row-major float32 in the reference's own layouts.
 *   - compute entry points are asynchronous on the caller's hipStream_t (passed as void*), perform no
 *     allocation and no host synchronisation, and are re-entrant across streams and devices.  (One exception, a diagnostic
 *     entry: mcd_debug_set_prof sets one process-wide pointer.)
 *   - there is NO CPU fallback: without a gfx950 device these calls fail with MCD_EDEVICE.
 */
#ifndef MOCODAD_HIP_H
#define MOCODAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCD_ABI_VERSION 15

enum {
    MCD_OK = 0,
    MCD_EINVAL = -1,      /* bad argument / unsupported shape */
    MCD_EMISSING = -2,    /* a state_dict tensor is missing or has the wrong size */
    MCD_EDEVICE = -3,     /* HIP error (no device, launch failure, ...) */
    MCD_EUNSUPPORTED = -4 /* configuration the kernels do not cover (message says which) */
};

/* conditioning strategy of models/mocodad.py:24-29,100-126 (canonical names) */
enum { MCD_STRATEGY_INJECT = 0, MCD_STRATEGY_CONCAT = 1, MCD_STRATEGY_NO_CONDITION = 2,
       MCD_STRATEGY_INBETWEEN_IMP = 3, /* condition frames stay at their own positions among the U-Net frames */
       MCD_STRATEGY_RANDOM_IMP = 4     /* same, with a different random set of n_cond condition frames per window
                                          (mcd_window_view_t.cond_mask) */ };
/* loss_fn of models/mocodad.py:24,66 (reduction='none', mean over C*Tx*V at :484) */
enum { MCD_LOSS_SMOOTH_L1 = 0, MCD_LOSS_L1 = 1, MCD_LOSS_MSE = 2 };
/* aggregation strategy of models/mocodad.py:454-520 */
enum {
    MCD_AGGR_ALL = 0, MCD_AGGR_BEST = 1, MCD_AGGR_WORST = 2, MCD_AGGR_MEAN = 3, MCD_AGGR_MEDIAN = 4,
    MCD_AGGR_MEAN_POSE = 5, MCD_AGGR_MEDIAN_POSE = 6, MCD_AGGR_QUANTILE = 7
};

#define MCD_MAX_FRAMES 32
#define MCD_MAX_COND_LAYERS 8
/* cond_layers value selecting the 'E_unet' condition encoder (STSE_Unet: the U-Net's down path + to_time_dim,
 * models/mocodad.py:110-114, stsae_unet.py:8-251); cond_channels is ignored */
#define MCD_COND_UNET (-1)

/* One named fp32 tensor of the Lightning checkpoint's state_dict (HOST memory).  Names are the
 * reference's own keys: "model.st_gcnnsd1.0.tcn.0.weight", "condition_encoder.btlnk.bias", ... */
typedef struct {
    const char* name;
    const float* data;
    int64_t numel;
} mcd_tensor_t;

/* Architecture, as MoCoDAD.build_model derives it (models/mocodad.py:90-126, stsae_unet.py:254-357). */
typedef struct {
    int32_t num_coords;   /* C: 2 */
    int32_t n_joints;     /* V: 17 (the U-Net hard-wires 17/12/10, stsae_unet.py:11) */
    int32_t t_unet;       /* frames the U-Net runs on: n_frames_corrupt (inject) or seg_len (the other strategies) */
    int32_t t_cond;       /* condition frames seen by the condition encoder (0 when there is none) */
    int32_t emb_dim;      /* embedding_dim == latent_dim: 16 */
    int32_t strategy;     /* MCD_STRATEGY_* */
    int32_t cond_layers;  /* ST-GCN layers of the condition encoder: len(channels)+1, or MCD_COND_UNET */
    int32_t cond_channels[MCD_MAX_COND_LAYERS]; /* their output channels: channels + [h_dim] */
} mcd_model_cfg_t;

/* One scoring call = MoCoDAD.forward on one batch (models/mocodad.py:129-184). */
typedef struct {
    int32_t n_windows;    /* B */
    int32_t n_samples;    /* n_generated_samples S */
    int32_t noise_steps;  /* ns: ns-1 denoiser passes per sample (mocodad.py:163) */
    int32_t seg_len;      /* T of the data tensor (B,C,T,V) */
    int32_t n_cond;       /* len(cond_idx)   (0 for no_condition) */
    int32_t n_corrupt;    /* len(corrupt_idx) */
    int32_t cond_idx[MCD_MAX_FRAMES];     /* frame indices selected at mocodad.py:743-748 */
    int32_t corrupt_idx[MCD_MAX_FRAMES];
    int32_t loss_fn;      /* MCD_LOSS_* */
} mcd_score_cfg_t;

typedef struct mcd_weights mcd_weights_t;

/* Replaces: LightningModule.load_state_dict + model.eval() (eval_MoCoDAD.py:36-38).
 * Folds every eval-mode BatchNorm2d into the preceding 1x1 conv (stsgcn.py:57-80,181-182), repacks the
 * channel-mixing matrices into MFMA fragment order and uploads them to `device`.
 * The handle is read-only for the scoring calls (any number of streams / host threads may share it) with ONE exception: two
 * device words in which workgroup 0 of a trajectory launch leaves (launch signature, its own lifetime in 100 MHz ticks) for
 * the next launch of the same grid to size its wave-priority time slice from.  Launches that overlap on different streams
 * race on these words (plain stores, no ordering); a torn or stale pair only selects the host's estimate of the slice (the
 * signature does not match) or a slice measured by the other launch -- scheduling, never results: scores are bit-identical
 * whatever the words hold (tests/test_hip_parity.py::test_overlapping_launches_on_two_streams). */
int mcd_pack_weights(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg,
                     int32_t device, mcd_weights_t** out);
void mcd_free_weights(mcd_weights_t* w);

/* Replaces: MoCoDAD._encode_condition -> STSAE/STSE.encode (mocodad.py:546-560, stsae.py:59-92).
 * cond_data (B,C,t_cond,V) -> emb_out (B,emb_dim).  The AE decoder (dead work at eval) is not run.
 * Windows are independent (ABI version 11, see mcd_score): a window with non-finite poses, or whose encoding overflows, gets
 * the non-finite embedding it gets as the only window of a call and changes no bit of any other window's.
 * (A test / diagnostic entry without a workspace argument: encoders that need scratch memory -- 'E_unet' above 12 condition
 * frames, the shipped encoder at 25 .. 31 (three 32-channel activation buffers no longer fit LDS) -- return MCD_EUNSUPPORTED here and run inside mcd_score / mcd_score_fused.) */
int mcd_cond_encode(const mcd_weights_t* w, const float* cond_data, int32_t n_windows, float* emb_out,
                    void* stream);

/* Scratch of the two single-pass entries below for n_windows windows: 0 for 1 .. 12 U-Net frames (everything lives in LDS), the
 * activation slabs of the slab-tiled kernel for 13 .. 32 frames (or of the runtime-shape kernel under MCD_OPT_GENERIC_UNET). */
int64_t mcd_pass_workspace_bytes(const mcd_weights_t* w, int32_t n_windows);

/* Replaces: STSAE_Unet.forward (stsae_unet.py:406-438) for one timestep shared by the batch.
 * x (B,C,t_unet,V), step_table row `t` (see mcd_score; t >= 0, the table must hold at least t + 1 rows -- a negative t is
 * MCD_EINVAL), cond (B,emb_dim) or NULL -> eps_out (B,C,t_unet,V).
 * Runs the production kernel of the frame count in single-pass mode: score_kernel<T_u,...> (1 .. 12 frames) or
 * score_tiled_kernel (13 .. 32; workspace = mcd_pass_workspace_bytes, else may be NULL). */
int mcd_unet_forward(const mcd_weights_t* w, const float* x, const float* cond, const float* step_table,
                     int32_t t, int32_t n_windows, float* eps_out, void* workspace, void* stream);

/* TEST ENTRY.  One stage of the U-Net alone, run by the production stage functions inside the trajectory kernel:
 * stage 0..10 = ST_GCNN_layer.forward of the 11 layers in execution order (stsgcn.py:94-116; st_gcnnsp1a.0, sd1.0, sd1.1,
 * sd2.0, sd2.1, sd3.0, sd3.1, su4.0, su4.1, su3.0, su3.1), 11..14 = CNN_layer over the joint axis as called at
 * stsae_unet.py:205,213,381,391 (down1, down2, up3, up2; without the skip add).
 * x (B,Cin,t_unet,Vin), emb (B,emb_dim) = the layer's `t` argument (the layer adds Linear(SiLU(emb)); required),
 * out (B,Cout,t_unet,Vout).  Instantiated for 3, 5, 6, 7, 9, 10, 11, 12 U-Net frames (score_kernel's LDS plan; each with the
 * template arguments and compile flags of the production kernel of that frame count -- twelve waves at 9 .. 12) and for 13 .. 32
 * (score_tiled_kernel: the stage's input is put where the previous layer's epilogue leaves it -- slab and LDS hand-over
 * regions -- and its output read from where its own epilogue puts it; workspace = mcd_pass_workspace_bytes).  In the slab-tiled
 * kernel the joint resamplers are not stages of their own: stages 3, 5, 7, 9 are (down1 | down2 | up3 | up2) + the layer, x is
 * the RESAMPLER's input (B,Cin,t_unet,17|12|10|12) and `skip` (stages 7, 9; or NULL) the U-Net skip tensor d2 (B,64,t_unet,12) /
 * d1 (B,32,t_unet,17) added behind the resampler (stsae_unet.py:381-383,391-393); stages 11..14 return MCD_EUNSUPPORTED there.
 * `skip` must be NULL otherwise. */
int mcd_layer_forward(const mcd_weights_t* w, int32_t stage, const float* x, const float* skip, const float* emb,
                      int32_t n_windows, float* out, void* workspace, void* stream);

/* The noise tensor the perf mode (noise == NULL) of mcd_score draws in-kernel, in mcd_score's `noise` layout
 * (S, max(ns-1,1), B, C=2, Tx, V=17): mcd_score(noise = this tensor) reproduces mcd_score(noise = NULL, seed,
 * first_window_id) bit for bit.  Replaces nothing in the reference (which draws torch.randn_like, mocodad.py:162,176);
 * it exists so that the in-kernel generator's distribution can be tested and the perf mode can be replayed by an oracle.
 * KEY LAYOUT (tests/draws_ref.py restates it in NumPy; tests/test_draws_gpu.py holds this tensor and every kernel's own draw to
 * it).  One Philox4x32-10 call has the key (low, high 32 bits of seed) and the counter (c0, c1, c2, c3):
 *   c1 = noise slot k (0 = x_T, k >= 1 = the z of step ns - k), c2 = sample s, c3 = (first_window_id + b) mod 2^32;
 *   x_T (k = 0):       c0 = (c * Tx + tx) * 17 + v, one call per element: z = r(w0) cos(a(w1)) of its output words w0 .. w3;
 *   step noise (k>=1): c0 = tx * 9 + v0 / 2, one call per joint pair (v0 even) of corrupt frame tx: (w0, w1) give the
 *                      coordinates c = 0, 1 of joint v0 as (r cos a, r sin a), (w2, w3) the same of joint v0 + 1 (unused at
 *                      v0 = 16);
 *   u(w) = ((float)(w >> 8) + 0.5f) * 2^-24 in float (the largest word rounds to u = 1 and gives r = 0),
 *   r(w) = sqrt(-1.38629436111989f * log2(u(w))), a(w) = 6.28318530717958647692f * u(w), on the hardware's log2, sqrt, sin, cos. */
int mcd_philox_noise(uint64_t seed, int64_t first_window_id, int32_t n_windows, int32_t n_samples, int32_t noise_steps,
                     int32_t n_corrupt, float* noise_out, void* stream);

/* Per-window condition-frame sets of MCD_STRATEGY_RANDOM_IMP drawn on the device: mask_out (n_windows,) int32 in the layout
 * mcd_window_view_t.cond_mask takes -- bit t set = frame t of the window conditions, exactly n_cond of the bits 0 .. seg_len-1
 * (bit 31 is the int32 sign bit and is legal).  Replaces nothing in the reference (which draws one torch.randperm per window on
 * the host and takes perm[t] < n_cond, mocodad.py:719-724,535): it is the same distribution, a uniform n_cond-subset, on a
 * different stream -- exactly as with the noise -- and exists so that the device draw can be exported, tested and replayed by an
 * oracle (mcd_score_view(cond_mask = these masks)), with no host work per batch.
 * The draw, fixed here so that it can be restated elsewhere bit for bit (tests/rndimp_ref.py): one thread per window b; random
 * words from Philox4x32-10 with the round function, multipliers and key schedule of the noise generator, key = (low, high) 32
 * bits of `seed`; call q = 0, 1, ... has the counter (c0, c1, c2, c3) = (q, 0xFFFFFFFF, 0xFFFFFFFF, (uint32)(first_window_id + b))
 * -- the noise streams use c1 = slot < noise_steps and c2 = sample < n_samples, so no call coincides with theirs; the window id
 * wraps at 32 bits like the noise key does -- and yields four words in output order.  Step i = 0 .. n_cond-1 takes word i % 4 of
 * call i / 4, r = ((uint64)word * (seg_len - i)) >> 32, and sets the bit of the r-th (0-based, ascending) frame not chosen yet.
 * Each step picks uniformly among the frames left; the multiply-high's bias is below seg_len / 2^32 per step.
 * 1 <= n_cond < seg_len <= 32 and n_windows >= 0, else MCD_EINVAL -- checked before any device call; n_windows == 0 is MCD_OK and
 * launches nothing. */
int mcd_random_imp_masks(uint64_t seed, int64_t first_window_id, int32_t n_windows, int32_t seg_len, int32_t n_cond,
                         int32_t* mask_out, void* stream);

/* Bytes of caller-provided device scratch a scoring call may need: condition embeddings when the condition encoder runs
 * as its own launch, (B,S) losses when an aggregation cannot be fused, scratch slabs of the runtime-shape kernels.
 * ALWAYS allocate it: workspace == NULL is accepted only by calls that end up as ONE launch (mcd_plan_split() == 1 with the
 * shipped condition encoder on a specialised frame count and a loss-based aggregation); every other form -- one trajectory
 * per workgroup for small or oddly sized batches, mcd_score without aggregation, another encoder architecture, more than 12
 * U-Net frames (the slab-tiled kernel's activations live in the workspace) -- fails with MCD_EINVAL ("workspace required")
 * without it. */
int64_t mcd_score_workspace_bytes(const mcd_weights_t* w, const mcd_score_cfg_t* cfg);

/* How the library would cut this scoring call into workgroups (a pure function of the shapes, the device and MCD_OPT_SPLIT):
 * 1 = a workgroup runs every sample of its windows -- condition encoder, trajectories and aggregation in ONE kernel launch,
 * the default for batches that fill the device (1024 windows x 5 samples on 256 CUs); n_samples = one trajectory per
 * workgroup with the encoder and the aggregation as their own launches (better fill for small batches); 0 = the call does
 * not run on score_kernel<T_u, ...> at all: 13 .. 32 U-Net frames (the slab-tiled kernel, persistent workgroups of one chain at a
 * time, aggregation as its own launch) or MCD_OPT_GENERIC_UNET.  Negative: MCD_E*. */
int32_t mcd_plan_split(const mcd_weights_t* w, const mcd_score_cfg_t* cfg);

/* Per-handle options (no environment variables; the only process-wide state is mcd_debug_set_prof's pointer).  Set them before the calls they affect, from the
 * thread that owns the handle; none is needed for normal use.
 *   MCD_OPT_VARIANT       alternative workgroup shapes of the trajectory kernel (tuning experiments only).
 *   MCD_OPT_COND_GENERIC  1: run the condition encoder through the runtime-channel-list kernel even when the shipped
 *                         architecture's MFMA kernel applies (used by the tests to cover both).
 *   MCD_OPT_GENERIC_UNET  1: run the trajectory through the plain-FMA runtime-shape kernel instead of the MFMA kernels (every
 *                         frame count 1 .. 32 has one; the tests use this to cross-check the two implementations).
 *   MCD_OPT_SPLIT         0 (default): the library chooses how many workgroups share a window's samples (1 = a workgroup
 *                         runs all samples of its windows: condition encoder and aggregation fused into the ONE launch;
 *                         n_samples = one trajectory per workgroup, better fill for odd batch sizes); n > 0 forces it
 *                         (tests).
 *   MCD_OPT_PHASE         tuning experiments on when co-resident workgroups of a scoring call start and take priority
 *                         (bench.py --phase).  0 (default): the library's behaviour.  The runtime-shape kernels ignore it; the
 *                         two MFMA trajectory-kernel families read it as follows:
 *                           value    1 .. 12 U-Net frames (score_kernel)            13 .. 32 frames (score_tiled_kernel)
 *                           n > 0    the second half of the grid starts             as 0
 *                                    n x 1024 clock cycles late
 *                           -1       no priority time slices                        no priority time slices (16-frame form;
 *                                                                                   the others never have them)
 *                           -2       slices from the host's estimate alone:         as 0 (this family has no self-calibration)
 *                                    the kernel's measurement of its previous
 *                                    launch is not used
 *                           n < -15  every workgroup starts at its own hashed       the slice length is forced to
 *                                    offset of 0 .. 63 x |n| x 16 cycles;           2^(-n - 16) ticks of the 100 MHz clock,
 *                                    slices as at 0                                 clamped to 2^10 .. 2^26 (16-frame form)
 *                           -3 .. -15  as 0                                         as 0
 *                         (n < -15 means different things to the two families: a start offset there, a slice length here.) */
enum { MCD_OPT_VARIANT = 0, MCD_OPT_COND_GENERIC = 1, MCD_OPT_GENERIC_UNET = 2, MCD_OPT_SPLIT = 3,
       MCD_OPT_PHASE = 4, /* tuning experiments: the table above */
       MCD_OPT_COUNT = 5 };
int mcd_set_option(mcd_weights_t* w, int32_t option, int32_t value);

/* Replaces: the hot loop of MoCoDAD.forward (mocodad.py:155-180) + the per-sample loss of :484.
 *   data        (B,C,T,V) windows
 *   noise       NULL -> in-kernel Philox4x32-10 keyed by (seed, first_window_id+b, s, step, element or joint-pair group);
 *               else (S, max(ns-1,1), B, C, Tx, V): slot 0 = x_T, slot k = z added at step i = ns-k
 *               (what torch.randn_like returns at mocodad.py:162,176 in call order)
 *   step_table  (ns, 4+emb_dim): row i = [1/sqrt(alpha_i), (1-alpha_i)/sqrt(1-alpha_hat_i), sqrt(beta_i), 0,
 *               pos_encoding(i)[0..emb_dim)]  (mocodad.py:172-178, stsae_unet.py:173-179)
 *   loss_out    (B,S)  per-sample window loss
 *   pose_out    NULL or (B,S,C,Tx,V) generated x_0
 * Chains are independent, as in the reference: a chain that diverges (NaN / Inf activations; a NaN in `noise`) returns a
 * non-finite loss and changes no other chain's result -- the persistent kernels clear their state behind it and re-run the
 * chains that shared its passes on their own.  Windows are independent as well (ABI version 11): a window with a NaN / Inf
 * pose, or whose condition encoding overflows, yields what it yields as the only window of a call -- non-finite per-sample
 * losses, as in the reference; under `inject` a NaN in a corrupt frame alone leaves pose_out finite -- and every other window's
 * losses, aggregated loss and poses are bit-identical to the same call without it, however the batch is cut into workgroups
 * (mcd_score_view and mcd_score_fused alike).  The call after such a call starts clean. */
int mcd_score(const mcd_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const float* noise,
              uint64_t seed, int64_t first_window_id, const float* step_table, void* workspace,
              float* loss_out, float* pose_out, void* stream);

/* Window view: lets the kernels read windows straight out of per-person trajectory buffers
 * and apply the dataset's test-time affine transform while loading, instead of the host materialising
 * seg_len x num_transform copies (reference: sliding windows utils/preprocessing.py:14-86, transforms
 * utils/dataset_utils.py:255-310 applied per item in utils/dataset.py:67-76).
 * Element (b, c, t, v) of window b is data[base[b] + c*stride_c + t*stride_t + v], then, when trans != NULL,
 * [x', y'] = A[trans[b]] @ [x, y, 1] with A = affine + 6*trans[b] = rows [a00 a01 a02 a10 a11 a12].
 * The view also carries the per-window condition-frame sets of the random_imp strategy. */
typedef struct {
    const int64_t* base;      /* device (B,) element offsets; NULL = dense (B,C,T,V) tensor */
    int64_t stride_c;         /* elements between the two coordinates of one joint */
    int64_t stride_t;         /* elements between consecutive frames */
    const int32_t* trans;     /* device (B,) transform index per window, or NULL */
    const float* affine;      /* device (n_transform, 6), required when trans != NULL */
    const int32_t* cond_mask; /* MCD_STRATEGY_RANDOM_IMP only: device (B,), bit t set = frame t of the window is a condition
                                 frame (exactly n_cond bits; mocodad.py:719-724 keeps both frame subsets in ascending
                                 order, so the mask is all the kernel needs); NULL otherwise */
} mcd_window_view_t;

/* mcd_score with a window view (view == NULL is exactly mcd_score). */
int mcd_score_view(const mcd_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                   const float* noise, uint64_t seed, int64_t first_window_id, const float* step_table, void* workspace,
                   float* loss_out, float* pose_out, void* stream);

/* mcd_score_view + the loss-based aggregation over the samples (mocodad.py:489-492,504-516: MCD_AGGR_BEST / WORST / MEAN /
 * MEDIAN / QUANTILE) in ONE call -- and, whenever the workgroups own whole windows, in ONE kernel launch: the condition
 * encoder runs in the workgroup that owns the window, the per-sample losses stay in its LDS, loss_agg (B,) is all that
 * is written.  loss_all (B,S) and pose_out are optional extra outputs (NULL = not wanted).  The *_pose strategies need the
 * generated poses of all samples: mcd_score + mcd_aggregate.  Any n_samples >= 1 (the reference's shipped test configs use
 * 50, config/<dataset>/mocodad_test.yaml): a workgroup keeps up to 64 per-sample losses of a window in LDS; with more samples the
 * per-sample losses go through the workspace and the aggregation runs as its own launch (as for mcd_plan_split() != 1). */
int mcd_score_fused(const mcd_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                    const float* noise, uint64_t seed, int64_t first_window_id, const float* step_table, void* workspace,
                    int32_t aggregation, float quantile, float* loss_agg, float* loss_all, float* pose_out, void* stream);

/* Replaces: MoCoDAD._aggregation_strategy (mocodad.py:454-520) on the (B,S) losses / (B,S,C,Tx,V) poses.
 * data/cfg give the ground-truth corrupt frames for the *_pose strategies.  loss_agg (B,), pose_agg
 * NULL or (B,C,Tx,V).  MCD_AGGR_ALL is the identity and is not handled here.  Any n_samples >= 1, like the reference: one
 * wave per window, order statistics (median = torch's lower middle value, quantile = torch's linear interpolation) by rank
 * counting over the samples, best / worst with the reference's strict comparisons (the first of equal samples is kept). */
int mcd_aggregate(const mcd_score_cfg_t* cfg, int32_t num_coords, int32_t n_joints, int32_t strategy, float quantile,
                  const float* loss_all, const float* pose_all, const float* data, float* loss_agg,
                  float* pose_agg, void* stream);

/* mcd_aggregate with a window view, for the *_pose strategies under MCD_STRATEGY_RANDOM_IMP (the reference computes them for
 * every conditioning strategy, mocodad.py:494-503).  With view->cond_mask given, the ground-truth corrupt frames of window b are
 * the frames whose bit is clear, in ascending order -- cfg->n_corrupt of them (exactly seg_len - n_corrupt bits of 0 .. seg_len-1
 * must be set, seg_len <= 32) -- and cfg->corrupt_idx is ignored.  `data` is the dense (B,C,T,V) tensor: a view with base != NULL
 * is MCD_EINVAL (materialise it first).  view == NULL, or a view without a mask, is exactly mcd_aggregate. */
int mcd_aggregate_view(const mcd_score_cfg_t* cfg, int32_t num_coords, int32_t n_joints, int32_t strategy, float quantile,
                       const float* loss_all, const float* pose_all, const float* data, const mcd_window_view_t* view,
                       float* loss_agg, float* pose_agg, void* stream);

/* Error maps (ABI version 15): WHERE a window's score comes from -- which joints, which forecast frames.  Replaces what a caller
 * would otherwise redo in PyTorch from pose_out: the per-element loss of mocodad.py:484 before its mean over C*Tx*V, with the
 * sample selection, tie rules and NaN behaviour of _aggregation_strategy (mocodad.py:454-520) as mcd_aggregate implements them.
 * It takes poses: mcd_score's, or for the latent model the decoded forecasts of mcd_latent_decode_samples (a latent itself has no
 * joints); num_coords must be 2 and n_joints 17, the layout the window loader reads.
 *   E[b,s,t,v] = (1/C) sum_c loss_elem(pose_all[b,s,c,t,v], x[b,c,t,v])       mean_{t,v} E[b,s] = loss_all[b,s] up to rounding
 * x = the ground-truth corrupt frame t of window b, read through `view` with the affine transform applied -- by the device function
 * the trajectory kernels load it with, so its bits are the ones the loss was computed on.  With view->cond_mask the corrupt frames of
 * window b are the clear bits of its mask in ascending order (cfg->corrupt_idx is ignored), else cfg->corrupt_idx.
 * maps_out (B,Tx,V) = M with mean_{t,v} M[b] = loss_agg[b] up to rounding:
 *   BEST / WORST   M[b] = E[b,s*], s* the sample aggregate_kernel selects (strict comparisons from 1e10 / -1 on the loss_all bits, the
 *                  first of equal samples stays); no sample selected (all NaN): a NaN map
 *   MEAN           the sum over s, in sample order, of E[b,s], divided by S
 *   MEDIAN         E[b,s_(r)], r = (S-1)/2, s_(r) the sample of rank r by (loss, sample index)
 *   QUANTILE       E_lo + wgt (E_hi - E_lo) in torch.lerp's two-sided form, lo / hi / wgt as for loss_agg
 *                  (MEDIAN / QUANTILE with a NaN among the window's S losses: a NaN map, as loss_agg is NaN)
 *   MEAN_POSE / MEDIAN_POSE   (1/C) sum_c loss_elem(p[b,c,t,v], x), p = the pose_agg of mcd_aggregate bit for bit (same device
 *                  functions, same order); loss_all is not read and may be NULL
 *   ALL            maps_out (B,S,Tx,V) = E itself; loss_all is not read and may be NULL
 * Selection is decided on the loss_all bits alone.  Unlike mcd_aggregate_view, a view with base != NULL is accepted: the dataset
 * and stream paths score through views.  One wave per window, any n_samples >= 1, one launch.  Argument errors are MCD_EINVAL before
 * any device call (with a mask: n_cond + n_corrupt must be seg_len <= 32, the bit count the mask carries); n_windows == 0 is MCD_OK
 * and launches nothing. */
int mcd_error_maps(const mcd_score_cfg_t* cfg, int32_t num_coords, int32_t n_joints, int32_t strategy, float quantile,
                   const float* loss_all, const float* pose_all, const float* data, const mcd_window_view_t* view,
                   float* maps_out, void* stream);

/* Frame-score assembly that follows the path (mocodad.py:386-401 + eval_utils.py:27-34): scatter-max of
 * window scores to their frames.  scores (N,), frames (N,seg_len) 1-based int32, row (N,) int32 = output
 * row (one per (transform, clip, person)), out (n_rows, n_frames) pre-zeroed by the callee; out[row, f] = the maximum of
 * max(score, 0) (a NaN adds 0) over the windows covering frame f.  Frames outside [1, n_frames] and rows outside [0, n_rows) are
 * ignored.  Argument errors (n, n_rows, n_frames < 0, seg_len < 1, a null pointer -- the inputs only when n > 0) are MCD_EINVAL
 * before any device call; an empty output is MCD_OK and launches nothing. */
int mcd_scatter_max(const float* scores, const int32_t* frames, const int32_t* row, int64_t n, int32_t seg_len,
                    int32_t n_rows, int32_t n_frames, float* out, void* stream);

/* The per-joint sibling of mcd_scatter_max (V = 17): maps (N,Tx,V) f32 (mcd_error_maps), frames (N,Tx) 1-based int32 = the frame id of each
 * map row, row (N,) int32 -> out (n_rows, n_frames, V), pre-zeroed by the callee; out[row, f, v] = the maximum of max(map, 0) (a NaN
 * adds 0) over the windows that forecast frame f.  Frames outside [1, n_frames] and rows outside [0, n_rows) are ignored; a cell no
 * window forecasts stays 0 -- the convention of the frame scores (for a tail forecast the first n_cond rows of a track stay 0). */
int mcd_joint_scatter_max(const float* maps, const int32_t* frames, const int32_t* row, int64_t n, int32_t n_corrupt,
                          int32_t n_rows, int32_t n_frames, float* out, void* stream);

/* Replaces: Trajectory._from_image_to_centre_bounding_box + compute_bounding_box (utils/data.py:11-43,165-186)
 * and scale_trajectories_robust (utils/data.py:350-359).  raw (n_frames, 34) f32 = the CSV columns 1..34
 * (x1,y1,...,x17,y17); out (n_frames, 2, 17) f32 = the frame-major buffer layout of mcd_window_view_t.
 * center/scale: device (34,) f64 in the CSV's interleaved feature order, or both NULL = no robust scaling.
 * Bit-exact to the reference under NumPy >= 2 (fp32 box arithmetic, round-half-even box sides; the scaler's subtraction and
 * division in float64, rounded to fp32 after each).  PRECONDITION: `raw` is finite (the Python wrapper checks it). */
int mcd_normalize_poses(const float* raw, int64_t n_frames, float vid_w, float vid_h,
                        const double* center, const double* scale, float* out, void* stream);

/* ---- Forecast tracks: expected poses per person and frame, in pixels (added without a change of MCD_ABI_VERSION, as the pretrain
 * stage was: two new exports and one new enum, no struct or existing signature touched).
 *
 * Replaces: compute_fig_matrix + extract_single_pose (utils/eval_utils.py:13-24, 37-72): the selected forecasts of many overlapping
 * windows collapsed into ONE pose per output cell, with the disagreement of the windows covering it.
 *   poses        (N, 2, Tx, 17) f32: the selected forecast of each window (pose_agg of mcd_aggregate)
 *   cell         (N, Tx) i32: the output cell of every forecast frame; a value outside [0, n_cells) means "ignore" (the convention
 *                mcd_scatter_max has for rows and frames).  A cell is whatever the caller numbers: a global trajectory row, or
 *                row * n_frames + f - 1 for a dense (row, frame) matrix in the reference's layout
 *   method       MCD_FORECAST_UNIQUE / MEAN / MEDIAN;  spread_method  MCD_FORECAST_MEAN / MEDIAN (over the 34 features)
 *   max_cover    1 .. 32: the (window, frame) pairs a cell's list holds
 *   workspace    n_cells * max_cover int32 words, caller-owned; it need not be initialised
 *   pose_out     (n_cells, 34) f32 in the CSV's interleaved order x1,y1,...,x17,y17 (the feature order of compute_fig_matrix)
 *   count_out    (n_cells,) i32: the pairs k covering the cell;  spread_out (n_cells,) f32
 * All three are written for every cell by the callee; a cell no window forecasts is 0 with count 0, the convention of the frame
 * scores.  Per cell, over its k pairs in ascending window index (within a window: ascending forecast frame), in float64, unfused,
 * rounded to fp32 once on store:
 *   UNIQUE  the pair of the lowest window index;  MEAN  the sum in that order / k;  MEDIAN  per feature the middle value, for an
 *           even k the half-sum of the two middle values (np.median)
 *   spread  per feature the population standard deviation in two passes -- the mean as above, then sqrt(sum((x - mean)^2) / k) --
 *           then the mean of the 34 values, summed in feature order, or their median (the half-sum of ranks 16 and 17)
 *   k > max_cover: count_out carries k, pose and spread are NaN.  (With fixed conditioning indices a frame is forecast by at most
 *           Tx windows, under random_imp by at most seg_len <= 32.)
 * A NaN in a forecast reaches only the cells that forecast covers.  The result does not depend on the order in which workgroups
 * reach a cell: pairs claim list slots with int32 atomics, the reduction orders the claimed indices before it combines them.
 * Two launches and one memset.  Argument errors (n, n_cells < 0, Tx outside 1 .. 32, max_cover outside 1 .. 32, an unknown method,
 * n * Tx > 2^31 - 1, a null pointer -- the inputs only when n > 0) are MCD_EINVAL before any device call; n == 0 or n_cells == 0 is
 * MCD_OK and launches nothing (n == 0: the outputs are zeroed, as mcd_scatter_max zeroes its own). */
enum { MCD_FORECAST_UNIQUE = 0, MCD_FORECAST_MEAN = 1, MCD_FORECAST_MEDIAN = 2 };
int mcd_forecast_assemble(const float* poses, const int32_t* cell, int64_t n, int32_t n_corrupt, int32_t n_cells, int32_t method,
                          int32_t spread_method, int32_t max_cover, int32_t* workspace, float* pose_out, int32_t* count_out,
                          float* spread_out, void* stream);

/* Forecasts from EVERY test-time transform (added without a change of MCD_ABI_VERSION: one new export, nothing existing touched):
 * mcd_forecast_assemble with the forecast of window i first mapped back through the inverse of its transform trans[i], so that the
 * windows of all transforms forecast a cell in the coordinates of transform 0.
 *   trans        (N,) i32 device: the transform of every window; a value outside [0, n_transform) makes the window's pairs ignored,
 *                as a cell outside [0, n_cells) is.  NULL: the call IS mcd_forecast_assemble (inv_affine and n_transform are not read,
 *                max_cover 1 .. 32)
 *   inv_affine   (n_transform, 6) f64 device rows [i00 i01 i02 i10 i11 i12]: the inverse of the 2 x 3 affine map of each transform
 *   max_cover    1 .. 64 (MCD_FORECAST_VIEW_COVER): 5 transforms x 12 forecast frames put 60 pairs on a cell
 * Per joint (x', y') of a forecast:  x = fp32((i00 x' + i01 y') + i02),  y = fp32((i10 x' + i11 y') + i12) -- products and sums in
 * float64, unfused, in that order, rounded to fp32 once.  A table row that equals (1,0,0,0,1,0) copies the value unchanged (a -0.0
 * keeps its sign, a NaN y' does not reach x).  The mapped fp32 values enter the reduction of mcd_forecast_assemble as they are, in
 * ascending pair index: with the dataset's transform-major window order that is transform, then window, then forecast frame.
 * Argument errors are those of mcd_forecast_assemble, plus trans without inv_affine and n_transform < 1 (MCD_EINVAL before any device
 * call). */
#define MCD_FORECAST_VIEW_COVER 64
int mcd_forecast_assemble_view(const float* poses, const int32_t* cell, const int32_t* trans, const double* inv_affine,
                               int32_t n_transform, int64_t n, int32_t n_corrupt, int32_t n_cells, int32_t method,
                               int32_t spread_method, int32_t max_cover, int32_t* workspace, float* pose_out, int32_t* count_out,
                               float* spread_out, void* stream);

/* Forecast fan: the distribution of ALL generated futures of a cell (added without a change of MCD_ABI_VERSION: one new export and two
 * constants, nothing existing touched).  Where mcd_forecast_assemble[_view] combines ONE selected forecast per covering pair, this
 * entry takes every sample of every covering pair and gives, per cell and coordinate, quantile bands, mean and standard deviation of
 * them all, and where the observed coordinate falls among them.
 *   poses_all    (N, S, 2, Tx, 17) f32: every sample of every window (pose_out of mcd_score, the poses of mcd_latent_decode_samples)
 *   cell, trans, inv_affine, n_transform, max_cover, workspace: exactly as in mcd_forecast_assemble_view (trans NULL: no map, max_cover
 *                1 .. 32; else 1 .. 64); the pairs of a cell are claimed by the same kernels and ordered by ascending pair index
 *   levels       HOST pointer: n_levels in 1 .. 8 (MCD_FORECAST_FAN_LEVELS) doubles in [0, 1], strictly ascending; read before the
 *                launch (they travel in the kernel's parameter block)
 *   observed     (n_cells, 2, 17) f32, the frame-major layout of mcd_window_view_t's buffer (a trajectory buffer can be passed as it
 *                lies), or NULL together with rank_out
 * The VALUE LIST of a cell and feature: for each of its k pairs in ascending pair index the samples s = 0 .. S-1 in order -- K = k S
 * values, each first mapped back by the rule of mcd_forecast_assemble_view when trans is given.  Outputs, all written for every cell by
 * the callee, every operation a float64 operation, unfused, rounded to fp32 once on store:
 *   count_out    (n_cells,) i32: k
 *   mean_out, std_out   (n_cells, 34) f32 interleaved x1,y1,...: the sum in list order / K, then sqrt(sum((x - mean)^2) / K) in a second
 *                pass (the definitions of mcd_forecast_assemble's spread)
 *   quant_out    (n_levels, n_cells, 34) f32, level-major: each level is an (n_cells, 34) block mcd_denormalize_poses takes as it is.
 *                With x the list sorted ascending, ties by list position (-0.0 == +0.0; np.sort(kind='stable')) and a level q:
 *                h = q (K - 1), i = floor(h), g = h - i; the value is x[i] when g == 0, else (1 - g) x[i] + g x[i + 1].  (q = 0.5 is
 *                np.median's half-sum; with S = 1 it is MCD_FORECAST_MEDIAN bit for bit.)
 *   rank_out     (n_cells, 34) f32: (below + equal / 2) / K, below = #{x < observed}, equal = #{x == observed} over the list
 * k = 0: every output of the cell is 0.  k > max_cover or K > 1024 (MCD_FORECAST_FAN_VALUES): count_out carries k, every other output
 * of the cell is NaN.  A NaN among a feature's values makes that feature's outputs NaN and no others (under a transform that is no
 * identity row a NaN reaches both coordinates of its joint, as in mcd_forecast_assemble_view); a NaN observed makes only its rank NaN.
 * The result depends neither on the order in which workgroups claim list slots nor on the workspace's prior contents.  One workgroup
 * per cell sorts (value, list position) keys in LDS, the joints in groups.  Two launches and one memset.  Argument errors -- those of
 * mcd_forecast_assemble_view, n_samples < 1, n_levels outside 1 .. 8, a level outside [0, 1] or not above its predecessor, observed
 * and rank_out not both NULL or both non-NULL -- are MCD_EINVAL before any device call; n_cells == 0 is MCD_OK and launches nothing,
 * n == 0 zeroes the outputs. */
#define MCD_FORECAST_FAN_VALUES 1024
#define MCD_FORECAST_FAN_LEVELS 8
int mcd_forecast_fan(const float* poses_all, const int32_t* cell, const int32_t* trans, const double* inv_affine, int32_t n_transform,
                     int64_t n, int32_t n_samples, int32_t n_corrupt, int32_t n_cells, const double* levels, int32_t n_levels,
                     int32_t max_cover, const float* observed, int32_t* workspace, float* quant_out, float* mean_out, float* std_out,
                     float* rank_out, int32_t* count_out, void* stream);

/* The inverse of mcd_normalize_poses: norm (n, 34) f32 interleaved (what mcd_forecast_assemble writes) back to image pixels in the
 * bounding box of raw (n, 34) f32, the observed CSV row of the same person and frame -> out (n, 34) f32 interleaved.
 * The box L, R, T, B is computed exactly as mcd_normalize_poses computes it (fp32 margin, clip, round-half-even); per element k,
 * with s = R - L, c = (L + R) / 2 for an x feature and s = B - T, c = (T + B) / 2 for a y feature,
 *   out = ((p * scale_k + center_k) * s + c)
 * every operation in float64 and unfused, rounded to fp32 once (center / scale: device (34,) f64, or both NULL: p * s + c).
 * A degenerate side (s = 0, where mcd_normalize_poses writes zeros) gives c.  count: NULL, or (n,) i32 -- a row with count 0 comes
 * back all zero, the CSV's convention for "missing".  One thread per row.  Argument errors are MCD_EINVAL before any device call;
 * n == 0 is MCD_OK and launches nothing.  PRECONDITION: `raw` is finite. */
int mcd_denormalize_poses(const float* norm, const float* raw, const int32_t* count, int64_t n, float vid_w, float vid_h,
                          const double* center, const double* scale, float* out, void* stream);

/* Live pose streams: the state between two ticks of an online scorer (many tracked people, one new pose row per track per
 * video frame), in two CALLER-owned device rings.  Replaces, one tick at a time, what the dataset path does once per dataset: the
 * per-row normalisation of mcd_normalize_poses, the sliding windows over consecutive rows of a trajectory
 * (utils/preprocessing.py:14-86) and the per-frame maximum over the windows covering a frame (compute_var_matrix + np.nanmax,
 * eval_utils.py:27-34, mocodad.py:392-393).
 *   ring          (n_slots, 2 * ring_len, 2, 17) f32 in the frame-major row layout mcd_window_view_t reads with stride_c 17 and stride_t 34.
 *                 Row r of a track (0-based count of the rows pushed for it) is stored TWICE, at positions r % ring_len and
 *                 r % ring_len + ring_len: the seg_len rows from row s on are contiguous from position s % ring_len, so a window is
 *                 one base offset, slot * 2 * ring_len * 34 + (s % ring_len) * 34, and the scoring entries read it as they read a
 *                 trajectory buffer.
 *   frame_scores  (n_slots, num_transform, ring_len) f32: cell r % ring_len = running maximum over the windows that cover row r.
 * A slot is one track; which track owns which slot, its row count and its frame ids are the host's business.  A tick holds AT MOST
 * ONE row per slot, a GROUP of ticks -- what the entries below take; a tick is a group of one -- at most ring_len - seg_len + 1
 * (the kernels use plain loads and stores).  One state is driven from one stream. */
typedef struct {
    float* ring;
    float* frame_scores;
    int32_t n_slots;
    int32_t ring_len;      /* L >= seg_len */
    int32_t seg_len;
    int32_t num_transform;
} mcd_stream_state_t;

/* A GROUP of consecutive ticks in one launch each: mcd_stream_push_group, ONE scoring call on all of the group's windows,
 * mcd_stream_frame_scores_group -- with the result of one such triple per tick, bit for bit.  A track may receive up to
 * ring_len - seg_len + 1 rows in a group (so ring_len > seg_len is what makes a group longer than a tick): then its
 * rows r0 - seg_len + 1 .. r0 + R - 1, the pending ones and the R new ones, sit at distinct ring positions, and no cell that is
 * zeroed aliases a pending one.  No track that receives a row in the group may be closed inside it (its slot is not handed out
 * again within the group); the caller cuts groups accordingly (mocodad_amd/stream.py: pack_ticks).
 * The group's windows are TICK-major, and inside a tick transform-major like the dataset order (utils/dataset.py:67-71): with
 * ne_i windows emitted by tick i and off_i = num_transform * (ne_0 + ... + ne_{i-1}), the window of the j-th emitting row of
 * tick i under transform t is at batch position off_i + t * ne_i + j -- consecutive ticks are consecutive slices, and a caller
 * that numbers windows globally gives each the id sequential ticks would have given it.
 * A SINGLE TICK is a group of one: at most one row per slot, pos0 = j (the row's position among the tick's n_emit windows),
 * ne = n_emit, w = j; n_windows = n_emit.
 *
 * mcd_stream_push_group: raw (n, 34) f32 as for mcd_normalize_poses, same arithmetic bit for bit (center / scale (34,) f64 or
 * both NULL; PRECONDITION: finite); desc (n, 4) i32 device = [slot, row index r, pos0, ne] per row: pos0 = off_i + j, the batch
 * position of the row's window under transform 0 (-1 while the track has fewer than seg_len rows), ne = ne_i, the stride between
 * transforms.  Slots may repeat (rows of one track, ascending r).  Per row: the normalised pose goes to both ring positions, the
 * row's frame-score cell is zeroed for every transform (which also makes a reused slot start clean), and for pos0 >= 0 the
 * window descriptors of the window ENDING at row r are written for every transform: base_out[pos0 + t * ne] (i64 element offsets
 * into `ring`), trans_out[pos0 + t * ne] = t -- the `base` / `trans` of a mcd_window_view_t over `ring` for mcd_score_view /
 * mcd_score_fused; base_out / trans_out hold num_transform * n_windows entries, n_windows = the sum of the ne_i.  Rows whose slot
 * is out of range are ignored, window positions outside the outputs are not written. */
int mcd_stream_push_group(const mcd_stream_state_t* s, const float* raw, const int32_t* desc, int32_t n, int32_t n_windows,
                          float vid_w, float vid_h, const double* center, const double* scale, int64_t* base_out,
                          int32_t* trans_out, void* stream);

/* The group's window scores into the frame-score ring (replaces mocodad.py:392-393 + eval_utils.py:27-34 for the rows in
 * flight).  scores (num_transform * n_windows,) f32 in the order of base_out; win (n_windows, 5) i32 device =
 * [slot, r_last, pos0, ne, w], SORTED by slot and within a slot by r_last; r_last = the row the window ends at, w = the window's
 * index in (tick, j) order.  Per window max(score, 0) -- the clamp of mcd_scatter_max; a NaN score adds 0 -- is taken into the
 * cells of rows r_last - seg_len + 1 .. r_last.  The windows of one track overlap within the launch: one thread per (track,
 * transform) applies them in row order with plain loads and stores (no atomics, no race).
 * final_out (n_windows, num_transform) f32 in (tick, j) order: row w = the cell of row r_last - seg_len + 1 once window w is in,
 * which no later window covers: that row's final frame score. */
int mcd_stream_frame_scores_group(const mcd_stream_state_t* s, const float* scores, const int32_t* win, int32_t n_windows,
                                  float* final_out, void* stream);

/* Tracks being closed: win (n, 2) i32 device = [slot, r_last = index of the track's last row]; out (n, seg_len - 1, num_transform)
 * f32 = the cells of the still-pending rows r_last - seg_len + 2 .. r_last.  (Tracks of fewer than seg_len rows have no window,
 * hence no frame score -- the dataset path drops them, utils/preprocessing.py:4-10 -- and are not passed here.) */
int mcd_stream_flush(const mcd_stream_state_t* s, const int32_t* win, int32_t n, float* out, void* stream);

/* Per-joint frame scores of a live stream (ABI version 15): a second CALLER-owned ring beside mcd_stream_state_t, which -- like the
 * three entries above -- stays as it is.
 *   joint_scores  (n_slots, num_transform, ring_len, 17) f32: cell (r % ring_len, v) = running maximum, over the windows that
 *                 FORECAST row r, of max(map value, 0) at joint v.
 * Cell rules (nothing here depends on the push kernel): a cell is initialised by the window that ENDS at its row -- with that window's
 * map value if it forecasts the row, else 0 -- and the first window of a track (r_last = seg_len - 1) initialises all seg_len cells;
 * so a reused slot and a wrapped ring start clean.  Every older row a window forecasts takes the maximum.  The cell of the window's
 * oldest row is then final.  The finals equal mcd_joint_scatter_max over the same track's windows bit for bit. */
typedef struct {
    float* joint_scores;
} mcd_stream_joint_state_t;

/* maps (num_transform * n_windows, n_corrupt, 17) f32 in the order of base_out (mcd_error_maps on the group's windows); win
 * (n_windows, 5) the SAME sorted table mcd_stream_frame_scores_group takes; cfg gives the forecast rows: seg_len (must equal the
 * state's), n_corrupt and corrupt_idx (ascending positions inside the window; n_cond + n_corrupt = seg_len).  One thread per (track,
 * transform, joint) walks the track's windows in row order with plain loads and stores.
 * final_out (n_windows, num_transform, 17) f32 in (tick, j) order. */
int mcd_stream_joint_scores_group(const mcd_stream_state_t* s, const mcd_stream_joint_state_t* js, const float* maps,
                                  const int32_t* win, int32_t n_windows, const mcd_score_cfg_t* cfg, float* final_out, void* stream);

/* Tracks being closed, as for mcd_stream_flush: win (n, 2) = [slot, r_last] -> out (n, seg_len - 1, num_transform, 17) f32. */
int mcd_stream_joint_flush(const mcd_stream_state_t* s, const mcd_stream_joint_state_t* js, const int32_t* win, int32_t n,
                           float* out, void* stream);

/* Forecast ring of a live stream (added without a change of MCD_ABI_VERSION, as the forecast exports were: two new exports and a new
 * struct, nothing existing touched): the EXPECTED POSE of a track row, leaving the device with the tick that makes the row final --
 * what mcd_forecast_assemble + mcd_denormalize_poses give for the row on the dataset path, bit for bit.  A third CALLER-owned state
 * beside mcd_stream_state_t and mcd_stream_joint_state_t, which stay as they are.
 *   forecast  (n_slots, ring_len, n_corrupt, 34) f32: cell (r % ring_len, j) = row r of the track as corrupt frame j of its ONE
 *             window, the window that ends at row r + seg_len - 1 - corrupt_idx[j]: that window's selected forecast of the row
 *             (pose_agg of mcd_aggregate under MCD_AGGR_BEST / WORST, zeros when no sample passes), interleaved x1,y1,...,x17,y17.
 *             Only windows of transform 0, the identity, are stored.
 *   observed  (n_slots, ring_len, 34) f32: cell r % ring_len = the raw row r as pushed.
 *   n_corrupt the model's number of forecast frames, 1 .. 32.
 * Cell rule (nothing is stored about validity, and nothing needs initialising): a cell has exactly one writer; cell (r, j), seen
 * from a track whose last row so far is r_hi, is valid iff its window exists -- corrupt_idx[j] <= r and
 * r + seg_len - 1 - corrupt_idx[j] <= r_hi.  corrupt_idx must ascend, so ascending window order is descending j.  A reused slot and
 * a wrapped ring start clean because an invalid cell is never read.
 * The row's result, over its k valid cells in ascending window order, is mcd_forecast_assemble's per cell (float64, unfused, rounded
 * once; UNIQUE / MEAN / MEDIAN, the two-pass population standard deviation per feature, its mean or median over the 34 features),
 * then mcd_denormalize_poses' per row in the box of the observed row.  A row with k = 0 (the first rows of a track) is all zero in
 * expected, norm and spread.  A row is final with the window whose oldest row it is: all k <= n_corrupt windows covering it are in.
 *
 * mcd_stream_forecast_group: behind the group's scoring call.  raw (n, 34), desc (n, 4): what mcd_stream_push_group was given;
 * loss_all (num_transform * n_windows, n_samples) and poses_all (num_transform * n_windows, n_samples, 2, n_corrupt, 17): the
 * per-sample losses and poses of that call, in the order of base_out; win (n_windows, 5): the table of
 * mcd_stream_frame_scores_group; cfg: seg_len (the state's), n_corrupt (the forecast state's), corrupt_idx (ascending; n_cond +
 * n_corrupt = seg_len), n_samples; aggregation: MCD_AGGR_BEST or MCD_AGGR_WORST; method / spread_method: MCD_FORECAST_*; vid_w,
 * vid_h, center, scale: as for mcd_denormalize_poses.  Two launches: (1) one 64-lane wave per transform-0 window selects its sample
 * and stores the n_corrupt x 34 values, further workgroups store the raw rows; (2) one wave per window reduces that window's oldest
 * row.  Outputs, row w of each = the row window w (in (tick, j) order) finalised: expected_out (n_windows, 34) f32 image pixels,
 * norm_out (n_windows, 34) f32 normalised, observed_out (n_windows, 34) f32 the raw row, count_out (n_windows,) i32 = k,
 * spread_out (n_windows,) f32.  n == 0 launches nothing; n_windows == 0 stores the raw rows only (the outputs may be NULL).
 * mcd_stream_forecast_flush: win (n, 2) = [slot, r_last] of tracks being closed, as for mcd_stream_flush -> the same five outputs
 * with n * (seg_len - 1) rows: the pending rows r_last - seg_len + 2 .. r_last, which see only the windows that exist.
 * Argument errors -- a null state, cfg or (where rows are produced) pointer, n_corrupt outside 1 .. 32 or not cfg's, a seg_len that is
 * not the state's, corrupt_idx not ascending, an unknown method or spread_method, an aggregation other than best / worst, negative
 * counts, n_windows > n, more rows than a group holds -- are MCD_EINVAL before any device call. */
typedef struct {
    float* forecast;
    float* observed;
    int32_t n_corrupt;
} mcd_stream_forecast_state_t;

int mcd_stream_forecast_group(const mcd_stream_state_t* s, const mcd_stream_forecast_state_t* fs, const float* raw, const int32_t* desc,
                              int32_t n, const float* loss_all, const float* poses_all, const int32_t* win, int32_t n_windows,
                              const mcd_score_cfg_t* cfg, int32_t aggregation, int32_t method, int32_t spread_method, float vid_w,
                              float vid_h, const double* center, const double* scale, float* expected_out, float* norm_out,
                              float* observed_out, int32_t* count_out, float* spread_out, void* stream);
int mcd_stream_forecast_flush(const mcd_stream_state_t* s, const mcd_stream_forecast_state_t* fs, const int32_t* win, int32_t n,
                              const mcd_score_cfg_t* cfg, int32_t method, int32_t spread_method, float vid_w, float vid_h,
                              const double* center, const double* scale, float* expected_out, float* norm_out, float* observed_out,
                              int32_t* count_out, float* spread_out, void* stream);

/* Forecast ring of a live stream over EVERY transform (added without a change of MCD_ABI_VERSION: two new exports and a new struct,
 * nothing existing touched): what mcd_forecast_assemble_view + mcd_denormalize_poses give for a row on the dataset path, bit for
 * bit.  A fourth CALLER-owned state; the three above stay as they are.
 *   forecast      (n_slots, ring_len, num_transform, n_corrupt, 34) f32: cell (r % ring_len, t, j) = row r as corrupt frame j of its
 *                 ONE window under transform t, ALREADY mapped back through the inverse of that transform (the per-joint map of
 *                 mcd_forecast_assemble_view; when no sample passes, the zeros are mapped)
 *   observed      (n_slots, ring_len, 34) f32: the raw row r as pushed
 *   n_corrupt     the model's number of forecast frames;  num_transform  the stream state's;  num_transform * n_corrupt <= 64
 * The cell rule is that of mcd_stream_forecast_state_t; it does not depend on t, and nothing needs initialising.  A row's k valid
 * cells (k <= num_transform * n_corrupt) are combined in the dataset's order: transform ascending, within a transform ascending
 * window (= descending j).
 * mcd_stream_forecast_group_tta / mcd_stream_forecast_flush_tta: the arguments, outputs and checks of mcd_stream_forecast_group /
 * mcd_stream_forecast_flush, plus inv_affine (num_transform, 6) f64 device, the table of mcd_forecast_assemble_view (read by the group
 * entry's store launch; the cells the flush entry reads are already mapped).  Store launch: one 64-lane wave per window of every
 * transform.  Plain loads and stores, no atomics.  Further argument errors: a null inv_affine, a num_transform that is not the
 * stream state's, num_transform * n_corrupt > 64 (MCD_EINVAL before any device call). */
typedef struct {
    float* forecast;
    float* observed;
    int32_t n_corrupt;
    int32_t num_transform;
} mcd_stream_forecast_tta_state_t;

int mcd_stream_forecast_group_tta(const mcd_stream_state_t* s, const mcd_stream_forecast_tta_state_t* fs, const float* raw,
                                  const int32_t* desc, int32_t n, const float* loss_all, const float* poses_all, const int32_t* win,
                                  int32_t n_windows, const mcd_score_cfg_t* cfg, int32_t aggregation, int32_t method,
                                  int32_t spread_method, float vid_w, float vid_h, const double* center, const double* scale,
                                  const double* inv_affine, float* expected_out, float* norm_out, float* observed_out,
                                  int32_t* count_out, float* spread_out, void* stream);
int mcd_stream_forecast_flush_tta(const mcd_stream_state_t* s, const mcd_stream_forecast_tta_state_t* fs, const int32_t* win, int32_t n,
                                  const mcd_score_cfg_t* cfg, int32_t method, int32_t spread_method, float vid_w, float vid_h,
                                  const double* center, const double* scale, const double* inv_affine, float* expected_out,
                                  float* norm_out, float* observed_out, int32_t* count_out, float* spread_out, void* stream);

/* Online clip scores of a live stream: the last stage of post_processing -- the person aggregation
 * mean_p s + (max_p log1p s - min_p log1p s) (mocodad.py:399-401), score_process = shift + gaussian_filter1d (eval_utils.py:100-106)
 * and the mean over the transforms (mocodad.py:424) -- incrementally, one value per video frame of a clip, from the final per-row
 * frame scores the entries above return (final_out of mcd_stream_frame_scores_group, out of mcd_stream_flush).
 * Semantics (mocodad_amd/stream.py: ClipTable holds the host half):
 *   raw(f, t)   = sum_p s_p / n + (max_p log1p(s_p) - min_p log1p(s_p)) over the n persons that have a final score at frame f,
 *                 in float64, 0 when n = 0.  (The dataset path counts every person of the WHOLE clip, absent ones as zeros; a live
 *                 clip has no final roster.  Where every person is present on every frame the two coincide, bit for bit.)
 *   shifted(k)  = raw(k - shift) for k - origin >= shift, else 0; origin = the first frame id of the clip's current segment.
 *   out(j, t)   = scipy gaussian_filter1d(shifted, sigma; truncate 4, 'reflect') over the segment origin .. head, summed as
 *                 mcd_frame_scores sums it: the centre tap, then the pairs from the outermost inwards;
 *   score(j)    = sum_t out(j, t) / num_transform, transforms added in ascending order.
 * pad_size and the HR masks of mcd_frame_cfg_t are not applied: they need the clip's final length.
 * State, CALLER-owned device memory, per (clip slot, transform, ring position) one cell = the aggregate of one frame so far:
 *   sum, lmax, lmin  (n_clips, num_transform, clip_ring_len) f64
 *   n                (n_clips, num_transform, clip_ring_len) i32 persons added
 * Which frame sits at which position, and which cells are open, complete or emitted, is the host's business.  One state is driven
 * from one stream. */
typedef struct {
    double* sum;
    double* lmax;
    double* lmin;
    int32_t* n;
    int32_t n_clips;
    int32_t clip_ring_len;
    int32_t num_transform;
} mcd_clip_state_t;

/* Final frame scores into their cells.  runs (n_runs, 5) i32 device = [clip slot, ring position, first contribution, count,
 * zero-first] per cell touched -- a cell is named AT MOST ONCE per call (one thread per (run, transform) owns it: plain loads and
 * stores); zero-first != 0 opens the cell (aggregate and count start from zero; a newly opened cell without a contribution is a
 * run with count 0).  contrib (n_contrib, 2) i32 device = [source, row]: source 0 = finals (n_finals, num_transform) f32, source
 * 1 = tails (n_tails, num_transform) f32 (either may be NULL with a count of 0); the contributions first .. first + count - 1 of a
 * run are added in list order.  Runs whose slot or position is out of range, runs whose contribution range leaves the list, and
 * contributions whose source or row is out of range are ignored.  0 <= n_runs <= n_clips * clip_ring_len. */
int mcd_stream_clip_update(const mcd_clip_state_t* c, const int32_t* runs, int32_t n_runs, const int32_t* contrib,
                           int32_t n_contrib, const float* finals, int32_t n_finals, const float* tails, int32_t n_tails,
                           void* stream);

/* Clip scores of the frames that became computable.  outs (n_out, 4) i32 device = [clip slot, frame offset j from the segment's
 * origin, segment length m (the segment has ended: 'reflect' at both ends) or -1 (open: every tap right of j lies inside the
 * segment; 'reflect' at the origin only), ring position of the origin]: the cell of offset k is at position (origin position + k)
 * % clip_ring_len.  gauss (2 * radius + 1,) f64 device = the normalised weights; shift >= 0, radius >= 0.  out (n_out,) f64 device
 * = score(j) as defined above.  Outputs whose slot, offset (j < 0, j >= m, j >= 2^29) or origin position is out of range come back
 * as 0.  0 <= n_out <= n_clips * clip_ring_len; num_transform <= 256. */
int mcd_stream_clip_emit(const mcd_clip_state_t* c, const int32_t* outs, int32_t n_out, const double* gauss, int32_t radius,
                         int32_t shift, double* out, void* stream);

/* Frame-score assembly after the path, whole: replaces the (transform, clip, person) loops of
 * MoCoDAD.post_processing (mocodad.py:362-425) with compute_var_matrix + np.nanmax (eval_utils.py:27-34, mocodad.py:392-393),
 * pad_scores (eval_utils.py:133-149), the person aggregation mean + (max - min of log1p) (mocodad.py:401-403), the HR frame
 * masks (:405-413), score_process = shift + scipy gaussian_filter1d(sigma = filter_kernel_size; truncate 4, 'reflect')
 * (eval_utils.py:100-106) and the mean over the transforms (:422); float64 like the NumPy code.  What is left for the host is
 * roc_auc_score.  All table pointers are DEVICE memory built once per dataset by the caller. */
typedef struct {
    int32_t n_clips;              /* ground-truth files, in sorted file-name order */
    int32_t num_transform;
    int32_t n_persons;            /* dense person-id range: ids 0 .. n_persons-1 (max id + 1) */
    int32_t max_frames;           /* row stride: max over the clips of len(gt) */
    int32_t pad_size;             /* anomaly_score_pad_size, -1 = no padding */
    int32_t frames_shift;         /* anomaly_score_frames_shift (>= 1) */
    int32_t gauss_radius;         /* int(4 * sigma + 0.5) */
    const int64_t* clip_keys;     /* (n_clips,) ascending (scene << 32 | clip) */
    const int32_t* clip_n_frames; /* (n_clips,) len(gt) */
    const int32_t* frame_dst;     /* (n_clips, max_frames) position of the frame in the clip's output after the HR masks, -1 = dropped */
    const int32_t* clip_out_len;  /* (n_clips,) frames kept */
    const int64_t* clip_out_off;  /* (n_clips,) offset of the clip's scores in `out` (sorted file-name order, concatenated) */
    const double* gauss_weights;  /* (2 * gauss_radius + 1,) scipy's normalised kernel */
} mcd_frame_cfg_t;
int64_t mcd_frame_scores_workspace_bytes(const mcd_frame_cfg_t* cfg);
/* scores (N,) f32, trans (N,) i64, meta (N,4) i64 = [scene, clip, person, first_frame], frames (N,seg_len) i32 1-based
 * (the arrays MoCoDAD.post_processing receives, on the device) -> out (sum clip_out_len,) f64 = `pds` of mocodad.py:422. */
int mcd_frame_scores(const mcd_frame_cfg_t* cfg, const float* scores, const int64_t* trans, const int64_t* meta,
                     const int32_t* frames, int64_t n_windows, int32_t seg_len, void* workspace, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * MoCoDADlatent (models/mocodad_latent.py, stage 'diffusion'): the reverse diffusion runs on a D-dimensional latent code of the
 * corrupt frames, through a small conditioned MLP.  A latent model has its own handle type: none of the entry points above
 * takes it.  Two launches per scoring call for the shipped configuration: encode (condition encoder + the U-Net's down path +
 * to_time_dim) and chain (every denoiser pass, the DDPM updates, the loss and the aggregation).  Any other condition encoder
 * runs as a launch of its own in front of the encode launch: three launches, or four for a runtime channel list, whose kernel
 * reads gathered condition frames (gather, cond_encode_kernel, encode, chain); see mcd_pack_latent_weights.  At 5 .. 12 corrupt
 * frames to_time_dim is a launch of its own between encode and chain (latent_project_kernel: one MFMA product over all windows
 * instead of a pass over the matrix per workgroup): condition encoder, encode, project, chain -- four launches, five for a runtime
 * channel list. */

#define MCD_LATENT_MAX_LAYERS 8
/* Denoiser of models/common/components.py:203-241 as MoCoDADlatent.build_model constructs it (mocodad_latent.py:51-57):
 * latent_dim = latent_embedding_dim, hidden = hidden_sizes (the last one equals latent_dim).  latent_dim and every hidden size:
 * a multiple of 16 in 16 .. 128; 1 .. 8 layers; anything else is MCD_EUNSUPPORTED. */
typedef struct {
    int32_t latent_dim;
    int32_t n_layers;
    int32_t hidden[MCD_LATENT_MAX_LAYERS];
} mcd_latent_cfg_t;

typedef struct mcd_latent_weights mcd_latent_weights_t;

/* Replaces: load_state_dict + eval() of a diffusion-stage MoCoDADlatent checkpoint (mocodad_latent.py:42-57; eval_MoCoDAD.py:36-38).
 * Reads model.{st_gcnnsp1a,st_gcnnsd1..3,down1,down2,to_time_dim}.* (STSE_Unet with embeddings, stsae_unet.py:50-154; there is no
 * up path), condition_encoder.* (encoder and bottleneck; the AE decoder is dead work at evaluation) and
 * denoiser.{net,cond_layers}.*.  BatchNorm2d / BatchNorm1d are folded into the preceding conv / Linear in double, the matrices
 * repacked into MFMA fragment order.  cfg: strategy MCD_STRATEGY_INJECT (mocodad_latent.py:32), t_unet = corrupt frames,
 * t_cond = condition frames.  Supported:
 *   t_unet       3 or 5 .. 12 (the rows of MCD_LATENT_ENCODE_INSTANCES: the down path's LDS plan is instantiated per count; another
 *                count is MCD_EUNSUPPORTED, naming "<t_unet> corrupt + <t_cond> condition frames" and the counts the library holds)
 *   t_cond       1 .. 12
 *   cond_layers  a channel list of 1 .. MCD_MAX_COND_LAYERS entries (channels + [h_dim], 'AE' / 'E'), or MCD_COND_UNET ('E_unet')
 * The shipped configuration (cond_layers 4, channels 32,16,32,32, t_cond = t_unet = 3) runs its condition encoder inside the
 * encode launch.  Every other one is packed as mcd_pack_weights packs it and runs as the pose model's kernel, in a launch of
 * its own that writes cond_emb (B,16) into the workspace: cond_fast_kernel (the shipped channel list at another t_cond),
 * cond_unet_kernel ('E_unet'), or cond_encode_kernel behind a gather of the condition frames (any other channel list); the
 * encode launch then reads cond_emb instead of computing it.  At t_unet 5 .. 12 the condition encoder is always a launch of
 * its own (there is no fused form and MCD_LATENT_OPT_SPLIT_ENCODE changes nothing), the encode launch writes the last layer's
 * output H (B, 640 t_unet) into the workspace, and to_time_dim.weight is packed with its columns in H's order as the MFMA
 * fragments of the projection launch.  A missing tensor is MCD_EMISSING with its name -- reported, like
 * the refusals above, before the device is touched. */
int mcd_pack_latent_weights(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg,
                            const mcd_latent_cfg_t* latent_cfg, int32_t device, mcd_latent_weights_t** out);
void mcd_free_latent_weights(mcd_latent_weights_t* w);

/* Bytes of device scratch mcd_latent_score needs for n_windows windows: cond_emb (B,16) and z0 (B,D) between its launches, plus
 * what the handle's condition-encoder kernel needs: nothing for the fused form, cond_fast_kernel and cond_unet_kernel; the
 * gathered condition frames (B,2,t_cond,17) for cond_encode_kernel, and its third activation buffer when three do not fit the
 * LDS; at t_unet 5 .. 12 also H (B, 640 t_unet) between the encode and the projection launch (nothing at t_unet 3: the size of
 * such a handle's workspace is what it was).  A pure function of the handle and n_windows (MCD_LATENT_OPT_SPLIT_ENCODE does not change it). */
int64_t mcd_latent_workspace_bytes(const mcd_latent_weights_t* w, int32_t n_windows);

/* Test and diagnostic aid in the style of mcd_set_option.
 *   MCD_LATENT_OPT_SPLIT_ENCODE  1: the shipped configuration takes the three-launch form too (cond_fast_kernel, then the encode
 *                                launch reading cond_emb), so the two forms can be compared on the same weights.  0: default.
 *   MCD_LATENT_OPT_DECODE_SPW    n > 0: a workgroup of mcd_latent_decode_samples' decode launch takes n samples of its window (at
 *                                most all of them) instead of what the launcher's rule gives.  0: the rule.  No result depends on it.
 *   MCD_LATENT_OPT_DECODE_CHUNK  n > 0: mcd_latent_decode_samples walks the batch in chunks of at most n windows (and at most what
 *                                its bound on G holds); mcd_latent_decode_workspace_bytes follows.  0: the bound alone.  No result
 *                                depends on it.
 * (The two decode options are new enumerators behind the existing one: no value a caller compiled against changes.) */
enum { MCD_LATENT_OPT_SPLIT_ENCODE = 0, MCD_LATENT_OPT_DECODE_SPW = 1, MCD_LATENT_OPT_DECODE_CHUNK = 2, MCD_LATENT_OPT_COUNT = 3 };
int mcd_latent_set_option(mcd_latent_weights_t* w, int32_t option, int32_t value);

/* The latent step table: (noise_steps + 1, 4 + emb_dim) -- rows 0 .. ns-1 as for mcd_score (update coefficients of
 * mocodad_latent.py:117-123 and pos_encoding(i), components.py:244-262), row ns = [0, 0, 0, 0, pos_encoding(-1)]: the constant
 * time step the encoder is given (mocodad_latent.py:95). */

/* Replaces: _encode_condition + _unet_forward(corrupt_data, t = -1, condition_embedding) (mocodad_latent.py:98-104 ->
 * STSE_Unet.forward, stsae_unet.py:222-249).  cfg: n_windows, seg_len, noise_steps (locates the table's last row) and the frame
 * index lists; data / view as for mcd_score_view -> cond_emb_out (B,16), z0_out (B,D).  One launch for the shipped
 * configuration, two otherwise (three with the gather of a runtime channel list), one more at t_unet 5 .. 12 (the projection); the
 * gather buffer of such an encoder and H of such a frame count come from the stream-ordered allocator (hipMallocAsync /
 * hipFreeAsync on `stream`) because this entry has no workspace argument.
 * Windows are independent (ABI version 11, see mcd_score): a non-finite pose in a condition frame (cond_emb and z0) or in a
 * corrupt frame (z0 alone) stays with its window; every other window's cond_emb and z0 are bit-identical to the call without it.
 * Alignment: at t_unet 5 .. 12 z0_out must be 16-byte aligned (the projection launch stores four floats at a time), else
 * MCD_EINVAL before any launch; at t_unet 3 any float alignment is taken. */
int mcd_latent_encode(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                      const float* step_table, float* cond_emb_out, float* z0_out, void* stream);

/* TEST ENTRY.  Replaces: Denoiser.forward (components.py:265-291) for n_rows arbitrary rows at one time step t >= 0 shared by
 * them: x (N,D), cond (N,16), step_table with at least t + 1 rows -> eps_out (N,D).  Runs the chain kernel's layer code.
 * Alignment: x and eps_out must be 16-byte aligned (rows are read and stored four floats at a time), else MCD_EINVAL. */
int mcd_latent_denoise(const mcd_latent_weights_t* w, const float* x, const float* cond, const float* step_table, int32_t t,
                       int32_t n_rows, float* eps_out, void* stream);

/* Replaces: MoCoDADlatent.forward, stage 'diffusion' (mocodad_latent.py:93-127) with the loss-based aggregations of
 * _aggregation_strategy (mocodad.py:484-516).
 *   noise        NULL -> in-kernel Philox4x32-10 keyed by (seed, first_window_id + b, s, slot, group of 4 latent elements);
 *                else (S, max(ns-1,1), B, D): slot 0 = x_T (torch.randn at mocodad_latent.py:109), slot k = the z of step
 *                i = ns - k (torch.randn_like at :121), in call order
 *   step_table   the latent step table above
 *   workspace    mcd_latent_workspace_bytes (required).  Behind the call (in stream order) its first n_windows x 16 floats hold
 *                cond_emb (B,16), until the workspace is used again: what mcd_latent_decode_samples takes as cond_emb_in
 *   aggregation  MCD_AGGR_ALL (loss_all required, loss_agg unused) or BEST / WORST / MEAN / MEDIAN / QUANTILE -> loss_agg (B,)
 *   loss_all (B,S), latent_all (B,S,D) generated latents, latent_code (B,D) = z0: optional outputs (NULL = not wanted)
 * cfg->loss_fn is applied to (generated latent, z0) and averaged over D.  1 .. 1024 samples per call.  Chains are independent:
 * one whose state becomes non-finite returns a non-finite loss and changes no other chain's result; `best` / `worst` skip it
 * like the reference's strict comparisons do.  Windows are independent too (ABI version 11, see mcd_score and
 * mcd_latent_encode): a window with non-finite poses has non-finite losses, and no other window's losses, latents or code
 * change by a bit.
 * Alignment: noise (when given) and workspace must be 16-byte aligned, else MCD_EINVAL before any launch; the regions carved
 * from the workspace (cond_emb, z0, gather, H) then are too.  The outputs take any float alignment. */
int mcd_latent_score(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                     const float* noise, uint64_t seed, int64_t first_window_id, const float* step_table, void* workspace,
                     int32_t aggregation, float quantile, float* loss_agg, float* loss_all, float* latent_all, float* latent_code,
                     void* stream);

/* ---- MoCoDADlatent, stage 'pretrain': the bottleneck autoencoder (added without a change of MCD_ABI_VERSION: two new exports, no
 * struct, enum or existing signature touched -- a caller built against version 15 without them runs unchanged, and a stale
 * library shows as a missing symbol when the binding is made).
 *
 * Replaces: build_model, stage 'pretrain' (mocodad_latent.py:58-64): STSAE_Unet(use_bottleneck, inject_condition) + the condition
 * encoder.  Reads 'model.{st_gcnnsp1a,st_gcnnsd1..3,down1,down2,to_time_dim}' as mcd_pack_latent_weights does, + 'model.{st_gcnnsu4,
 * st_gcnnsu3,up3,up2,rev_to_time_dim}', + 'condition_encoder.*'; no 'denoiser.*'.  3 or 5 .. 12 corrupt frames, 1 .. 12 condition
 * frames, latent_dim a multiple of 16 in 16 .. 128; anything else is MCD_EUNSUPPORTED by name, a missing tensor MCD_EMISSING with
 * its name, both before the device is touched.  The handle is a mcd_latent_weights_t of the autoencoder kind: freed by
 * mcd_free_latent_weights, sized by mcd_latent_workspace_bytes (cond_emb, z0, the condition encoder's scratch, and one region that
 * holds H and then G = rev_to_time_dim(z), 640 floats per corrupt frame and window), taken by mcd_latent_encode and
 * mcd_latent_reconstruct (and by mcd_latent_decode_samples, which has a workspace size of its own).  mcd_latent_score /
 * mcd_latent_denoise on it, and mcd_latent_reconstruct / mcd_latent_decode_samples on a diffusion-stage handle, return
 * MCD_EUNSUPPORTED naming the kind the call needs. */
int mcd_pack_latent_ae_weights(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, int32_t latent_dim,
                               int32_t device, mcd_latent_weights_t** out);

/* Replaces: MoCoDADlatent.forward, stage 'pretrain' (mocodad_latent.py:93-100, 131: _unet_forward at t = -1 -> STSAE_Unet.forward,
 * stsae_unet.py:406-438) and the per-window term of post_processing (mocodad_latent.py:218): launches [condition encoder] ->
 * encode -> [project, 5 .. 12 corrupt frames] -> unproject (rev_to_time_dim, all windows as one MFMA product) -> decode (the up
 * path with both skips, + X).  The decode launch forms the skips d1 / d2 again from the window's corrupt frames; nothing but G
 * crosses the launch boundary.
 *   z_in          NULL: the decoder takes the window's own code z0; else (B,D), 16-byte aligned: the caller's latents, decoded with
 *                 the window's own skips and condition
 *   pose_out      NULL or (B, 2, t_unet, 17): the reconstructed corrupt frames
 *   loss_out      NULL or (B): mean over (c,t,v) of cfg->loss_fn(pose, corrupt frames), summed in a fixed order
 *   cond_emb_out  NULL or (B,16);  z0_out  NULL or (B,D): the window's own code, also when z_in is given
 * cfg: n_windows, seg_len, noise_steps (locates the table's row of t = -1), loss_fn and the frame lists; n_samples is not read.
 * n_windows <= 0 returns MCD_OK before anything is touched.  Windows are independent: a non-finite pose or z_in row stays with
 * its window, every other window's four outputs keep their bits.
 * Alignment: workspace and z_in (when given) 16-byte aligned, else MCD_EINVAL before any launch; the outputs take any float
 * alignment. */
int mcd_latent_reconstruct(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                           const float* step_table, void* workspace, const float* z_in, float* pose_out, float* loss_out,
                           float* cond_emb_out, float* z0_out, void* stream);

/* ---- Generated latents back to poses (added without a change of MCD_ABI_VERSION, as the pretrain stage was: two new exports).
 *
 * The diffusion stage scores in latent space; the stage-1 autoencoder's rev_to_time_dim and up path are the decoder of the latents
 * it generates (the reference freezes the down path, to_time_dim and the condition encoder when it trains stage 2, so those
 * tensors are the same in both checkpoints).  On an AUTOENCODER handle (a diffusion-stage handle: MCD_EUNSUPPORTED naming the kind
 * the call needs):
 *   latents      (B,S,D), 16-byte aligned: e.g. latent_all of mcd_latent_score
 *   cond_emb_in  NULL: the handle's own condition encoder runs as a launch in front; else (B,16), what mcd_latent_encode /
 *                mcd_latent_score produced for these windows
 *   pose_all     NULL or (B,S,2,t_unet,17): sample s of window b decoded with the window's own skips and condition, + its corrupt frames
 *   loss_all     (B,S): mean over (c,t,v) of cfg->loss_fn(pose, corrupt frames), summed in the fixed order of mcd_latent_reconstruct
 *   workspace    mcd_latent_decode_workspace_bytes(w, n_windows, n_samples), 16-byte aligned
 * pose_all[:, s] and loss_all[:, s] are bit for bit what mcd_latent_reconstruct(z_in = latents[:, s]) returns.  Both have the
 * layout of mcd_score's outputs: mcd_aggregate, mcd_aggregate_view and mcd_error_maps take them as they take those.
 * Launches: [condition encoder] -> per chunk of windows: latent_unproject_kernel over the chunk's latent rows -> the decode launch,
 * one workgroup per window and range of its samples: the down stem for the skips runs once per workgroup, not once per sample.
 * Cost: G = rev_to_time_dim of a row is 640 t_unet floats; the call walks the batch in chunks of windows so that G stays under
 * 256 MB, and the workspace is cond_emb (B,16) + the condition encoder's scratch + that bounded G.  1 .. 1024 samples per call.
 * Samples and windows are independent: a non-finite latent row gives that sample a non-finite loss and changes no other sample's
 * or window's bits; neither do the chunking nor the split of a window's samples over workgroups.
 * n_windows <= 0 returns MCD_OK before any device call; n_samples < 1, a NULL latents / loss_all / workspace, a misaligned latents or
 * workspace are MCD_EINVAL before any launch. */
int64_t mcd_latent_decode_workspace_bytes(const mcd_latent_weights_t* w, int32_t n_windows, int32_t n_samples);
int mcd_latent_decode_samples(const mcd_latent_weights_t* w, const mcd_score_cfg_t* cfg, const float* data, const mcd_window_view_t* view,
                              const float* step_table, void* workspace, const float* cond_emb_in, const float* latents, float* pose_all,
                              float* loss_all, void* stream);

/* ---- The latent model scored in pose space, one call (added without a change of MCD_ABI_VERSION, as the decode exports were: two
 * new exports, no struct, enum or existing signature touched).
 *
 * Replaces: the caller's sequence mcd_latent_score(MCD_AGGR_ALL, latent_all) -> mcd_latent_decode_samples(cond_emb_in = the head of
 * the first call's workspace) -> mcd_aggregate_view -> [mcd_error_maps] -- what MoCoDADlatent.forward does in pose space
 * (latent_score_space 'pose'; of the reference: mocodad_latent.py:93-127 for the latents, stsae_unet.py:406-438 for the decoder,
 * mocodad.py:454-520 for the aggregation).  On the caller's stream it makes exactly the launches of those entries, in that order, so
 * every output is bit for bit theirs; what changes is that cond_emb, the latents and (where nobody asked for them) the per-sample
 * losses and poses never leave the one workspace, whose layout the library owns.
 *   w / ae       the diffusion-stage handle (mcd_pack_latent_weights) and its decoder, an autoencoder handle
 *                (mcd_pack_latent_ae_weights); swapped or of one kind: MCD_EUNSUPPORTED naming the kind needed.  They must agree
 *                on t_unet, t_cond, latent_dim and the device (MCD_EINVAL naming the field); cfg's seg_len and frame lists serve both
 *   noise, seed, first_window_id, step_table     as for mcd_latent_score
 *   workspace    mcd_latent_pose_workspace_bytes(w, ae, n_windows, n_samples), 16-byte aligned: [mcd_latent_score's workspace, cond_emb
 *                at its head][loss_all (B,S)][latent_all (B,S,D)][pose_all (B,S,2,t_unet,17)][mcd_latent_decode_samples's workspace];
 *                the size does not depend on which outputs are passed (0 for a NULL or wrong-kind handle or sizes out of range)
 *   aggregation  BEST / WORST / MEAN / MEDIAN / QUANTILE (with `quantile`) -> loss_agg (B,), required
 *   optional outputs (NULL = not wanted): loss_all (B,S) the pose-space losses; pose_all (B,S,2,t_unet,17); pose_agg (B,2,t_unet,17) the
 *                selected forecast (BEST / WORST only, else MCD_EINVAL); maps (B,t_unet,17) as mcd_error_maps writes them under the
 *                aggregation; latent_all (B,S,D) the generated latents, 16-byte aligned (the decode launches read it).  pose_all is
 *                written into the workspace when it is NULL but pose_agg or maps is asked for; when none of the three is, the
 *                decode launches write losses only
 * Checks come before any launch and name what failed: the handles' kinds and agreement, NULL data / step_table / workspace /
 * loss_agg, the sizes and alignment rules of mcd_latent_score and mcd_latent_decode_samples, the frame lists, a view with a
 * cond_mask (the latent model has fixed frame lists).  n_windows <= 0 returns MCD_OK before anything is touched.  Windows and
 * samples are independent as in the four entries. */
int64_t mcd_latent_pose_workspace_bytes(const mcd_latent_weights_t* w, const mcd_latent_weights_t* ae, int32_t n_windows,
                                        int32_t n_samples);
int mcd_latent_score_pose(const mcd_latent_weights_t* w, const mcd_latent_weights_t* ae, const mcd_score_cfg_t* cfg, const float* data,
                          const mcd_window_view_t* view, const float* noise, uint64_t seed, int64_t first_window_id,
                          const float* step_table, void* workspace, int32_t aggregation, float quantile, float* loss_agg,
                          float* loss_all, float* pose_all, float* pose_agg, float* maps, float* latent_all, void* stream);

/* The draws of mcd_latent_score's perf mode in its `noise` layout (S, max(ns-1,1), B, D): feeding them back reproduces the perf
 * mode bit for bit.  Replaces nothing in the reference (torch.randn / randn_like, mocodad_latent.py:109,121).
 * KEY LAYOUT (key, c1 = slot k, c2 = sample s, c3 = window id, u, r and a as for mcd_philox_noise): for every slot c0 = d0 / 4,
 * one call per group of four elements d0 .. d0 + 3, which are r(w0) cos(a(w1)), r(w0) sin(a(w1)), r(w2) cos(a(w3)),
 * r(w2) sin(a(w3)) in this order.
 * Alignment: noise_out must be 16-byte aligned (an element group of four floats is one store), else MCD_EINVAL. */
int mcd_latent_philox_noise(uint64_t seed, int64_t first_window_id, int32_t n_windows, int32_t n_samples, int32_t noise_steps,
                            int32_t latent_dim, float* noise_out, void* stream);

/* Profiling builds only (-DMCD_PROFILE, tools/stage_profile.py): device buffer of 96 uint64 per-stage cycle accumulators
 * written by workgroup 0 of the trajectory kernel; NULL (the default) disables it.  A no-op in the shipped build. */
void mcd_debug_set_prof(void* device_buffer);

/* Test aid: fills the LDS of every CU with NaN bit patterns (4096 workgroups of 160 KB on `stream`), so that a later kernel
 * that reads shared memory it never wrote yields NaNs instead of whatever the previous kernel left behind
 * (tests/test_hip_parity.py::test_no_uninitialised_reads). */
int mcd_debug_poison_lds(void* stream);

/* Test aid, host only (no device call, no GPU needed): runs the packer of mcd_pack_weights -- or, with latent_cfg != NULL, of
 * mcd_pack_latent_weights -- and returns the packed buffer's float count and a 64-bit FNV-1a digest over the buffer's bytes
 * followed by the tables the handle would keep.  The packers' argument and tensor errors come back as theirs do.
 * tests/test_pack_layout_host.py pins the layout with it. */
int mcd_debug_pack_digest(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, const mcd_latent_cfg_t* latent_cfg,
                          int64_t* n_floats_out, uint64_t* digest_out);

/* ... the same for the packer of mcd_pack_latent_ae_weights (the autoencoder of stage 'pretrain'). */
int mcd_debug_pack_ae_digest(const mcd_tensor_t* tensors, int32_t n_tensors, const mcd_model_cfg_t* cfg, int32_t latent_dim,
                             int64_t* n_floats_out, uint64_t* digest_out);

const char* mcd_last_error(void);
int32_t mcd_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MOCODAD_HIP_H */
