/*
 * tdnnf_hip.h -- C-ABI of libtdnnf_hip.so: the MI355X (gfx950) implementation of the
 * LF-MMI TDNN-F / DARTS hot path of skhu101/TDNN-F_NAS.
 *
 * Every entry point replaces one nnet3 Component virtual (or one optimizer helper)
 * of the reference; the reference symbol is cited next to it as
 * /root/reference-relative file:line.  INTEGRATION.md shows the Kaldi-side adapter
 * that forwards CuMatrixBase<float> views to these functions.
 *
 * Conventions
 *  - tdnnf_mat is exactly Kaldi's CuMatrixBase<float> view: device pointer, rows,
 *    cols, row stride in ELEMENTS, row-major (usage: src/nnet3/nnet-tdnn-component.cc:815-819).
 *  - Pointers named *_dev are device memory; "host" pointers are small index
 *    arrays read during the call.  The caller owns every buffer.
 *  - stream is a hipStream_t (NULL = default stream).  No call synchronises the
 *    stream or the device; scalars (objf, dot products, taps' s_i) are written
 *    to device memory.  Random draws are INPUTS (device buffers) so results are
 *    reproducible (SURVEY.md 7 "Randomness").
 *  - Return value: 0 = ok, TDNNF_EINVAL = bad argument (nothing launched),
 *    TDNNF_EHIP = a HIP runtime call failed.  tdnnf_last_error() gives the text.
 *    Nothing throws across this boundary (the reference's KALDI_ERR/KALDI_ASSERT
 *    become error codes; the C++ adapter turns them back into exceptions).
 *  - kBackpropAdds / kPropagateAdds semantics of the reference are kept: where
 *    the reference adds into its output, so do we.
 */
#ifndef TDNNF_HIP_H_
#define TDNNF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDNNF_OK 0
#define TDNNF_EINVAL 1
#define TDNNF_EHIP 2

#define TDNNF_MAX_OFFSETS 16

typedef struct {
  float *data;
  int rows, cols, stride;
} tdnnf_mat;

typedef void *tdnnf_stream;
typedef struct tdnnf_ng tdnnf_ng; /* OnlineNaturalGradient state (A8, below) */

const char *tdnnf_last_error(void);
int tdnnf_abi_version(void);
/* Tuning options: process-wide integers selecting between code paths (the library reads no environment variable for them; which
   values the test suite exercises: csrc/common.h, struct Options).  Unknown names fail with TDNNF_EINVAL.
     "ng_grouped"    1 (default) natural-gradient side chain of a gradient bucket as grouped launches, 0 per object   [read by tdnnf_net_create]
     "ng_fuse"       1 (default) output-side statistic inside the BatchNorm / ReLU backward sweep when that pays, 0 own GEMM, 2 always
     "ng_early_in"   1 (default) input-side statistics ahead of the backward pass, 0 with the component's backward call [tdnnf_net_create]
     "wgrad_stream"  -1 (default) parameter gradients on their own stream for small minibatches, 0 never, 1 always       [tdnnf_net_create]
     "gemm_ring"     1 (default) persistent LDS-DMA-ring rows GEMM where it applies, 0 the plain tile kernel
     "planes"        1 (default) gemm_precision 2 runs the pre-split bf16-plane GEMMs where they apply, 0 the in-kernel split
     "den_mw_test_abort", "planes_check_bound": test hooks (0 = off), see tests/test_gpu_parity.py, tests/test_gpu_net.py
     "den_split"     -1 (default) and 1: the trainer runs the denominator's two recursions side by side; 0 never (read at a net's first step)
                     (set before the first tdnnf_net_forward_backward of a net: it sizes the chain workspace)
     "num_form"      0 (default) the numerator by the supervision's width: one wave per sequence for at most 4 states per frame on average,
                     one workgroup per sequence with the frontier in LDS for wider ones; 1 / 2 force one (A/B runs, tests).  A narrow
                     supervision can take form 2 only if it was created while the option was 2 (tdnnf_supervision_create builds the tables then)
     "align_form"    0 (default) best-path alignment keeps its two state vectors in LDS where they fit, in the workspace otherwise; 1 / 2
                     force one (tests); read by tdnnf_align_workspace_bytes and tdnnf_align_best_path, and in the same way by
                     tdnnf_align_posteriors_workspace_bytes, tdnnf_align_posteriors, tdnnf_align_posteriors_compact, the two
                     tdnnf_align_posteriors_sparse entries and the label entries (tdnnf_align_best_path_labels, tdnnf_align_label_posteriors_*)
     "align_checkpoint"  0 (default) forward-backward keeps alpha of every frame in the workspace; C >= 1: alpha of every C-th frame only, and
                     the backward pass recomputes each segment of C frames from its checkpoint -- the same bits, about one forward sweep more;
                     -1: C = ceil(sqrt(frames of the call's longest utterance)).  Anything else: TDNNF_EINVAL from the calls, 0 from the
                     workspace questions.  Read by tdnnf_align_posteriors_workspace_bytes (want_posteriors != 0) and by tdnnf_align_posteriors
                     (post_out != NULL), tdnnf_align_posteriors_compact, the sparse and the label posterior entries and their workspace
                     questions alike: set it before both.  Ignored where no alpha is kept (want_posteriors = 0, post_out == NULL)
     "align_path_checkpoint"  0 (default) best-path alignment keeps one back-pointer per (frame, state) in the workspace; C >= 1: the state
                     scores of every C-th frame and the back-pointers of C frames at a time, and the trace-back recomputes each earlier segment
                     of C frames from its checkpoint -- the same path, score and ok flag, up to one more sweep over the arcs; -1: C =
                     ceil(sqrt(frames of the call's longest utterance)).  Anything else: TDNNF_EINVAL from the calls, 0 from the workspace
                     question.  Read by tdnnf_align_workspace_bytes, tdnnf_align_best_path and tdnnf_align_best_path_labels alike: set it
                     before both.  Not read by the posterior entries, as "align_checkpoint" is not read by the best path
     "num_frontier_cap": test hook (0 = off): frames of more states than this keep the wide form's frontier in global memory
     "gemm_arith_test": test hook (0 = off): 1 / 3 = the stand-alone GEMM entries (tdnnf_tdnn_*, tdnnf_affine_*) run the in-kernel split-bf16
                     kernels (bf16x3 / bf16x6) wherever exact f32 would be their default; the natural-gradient statistics and the orthonormal
                     constraint keep exact f32
   The GEMM planners' options (gemm_ring, splitk_partial_round, splitk_per_cu, gemm_alt_taps, ng_bk, wgrad_small) are tested value by
   value against float64 in tests/test_gpu_gemm_forms.py. */
int tdnnf_set_option(const char *name, int value);
int tdnnf_get_option(const char *name, int *value_out);
/* diagnostics, tests: how often the rows GEMM and the weight gradient took each kernel and launch form since the last reset.  Counter i is
   named tdnnf_gemm_launch_form_name(i) (NULL outside the range; the string is valid until the calling thread's next call):
     "rows.<tile>.<arithmetic>.<form>"  tile = rows x cols k K-step (128x128k16 ...), arithmetic f32 / bf16x3 / bf16x6, form one of
         plain, ring, splitk (every tile split over K), partial_s2 .. partial_s8 (one partly filled round, K split by S), main_split_tail /
         main_plain_tail (whole rounds -- counted as plain or ring as well -- then the last rows as a split-K or a plain launch),
         sumsq_plain / sumsq_splitk (the passes with the ||row||^2 by-product), post (inference epilogue), grouped;
     "rows.launches_vec4" / "rows.launches_scalar"  kernel launches of the above that load 16 bytes at a time / float by float;
     "planes.plain", "planes.main_split_tail", "planes.main_plain_tail"  rows GEMMs routed onto the pre-split plane kernels, ONE of the
         three per call (here the whole rounds of a main + tail call are not counted as plain as well); "planes.alt_chunked": calls
         whose two taps went in alternating chunks of K blocks (option gemm_alt_taps 2);
     "wgrad.<tile>.<arithmetic>" weight gradients per tile, "wgrad.planes" those on the plane kernels, and "wgrad.last_slabs", which is not
         a count but the number of row slabs of the last weight gradient; "rows.last_slices" likewise: the K slices of the rows GEMM's
         last split-K launch.
   Writes min(capacity, count) values to counts (may be NULL), clears all counters when reset != 0 and returns the number of counters.
   Counting never changes a decision and never synchronises. */
int tdnnf_gemm_launch_forms(long long *counts, int capacity, int reset);
const char *tdnnf_gemm_launch_form_name(int index);
/* the same for the trainer's fused BatchNorm / ReLU sweeps (one count per call of the sweep, none per kernel thread):
     "apply_bypass.<vec4|scalar|planes>[.super][.mask][.rev]"  the forward pass out = BN(x) * mask + bypass * prev: the kernel instance (16-byte
         accesses, float by float, vec4 with the f16 plane stores), whether the view was a super row, a dropout mask was given, the walk reversed;
     "bwd.reduce.<vec4|scalar>.<stats|nostats>"  the backward sweep's reduction, with or without the ReLU statistics;
     "bwd.finalize.<train|test>"  its finalize launch (test: the BatchNorm is in test mode);
     "bwd.apply.<vec4|scalar|planes>[.mask][.rev]"  its apply launch; "bwd.apply.rows_unrolled" / "bwd.apply.rows_tail": those apply launches in
         which some row lane runs the 16-row unrolled loop / the 4-row tail loop; "bwd.apply.short_last_chunk": whose last row chunk is short;
     "bwd.apply_ng.nt<1|2|3>[.mask][.planes][.rev]"  the apply launch that carries the natural-gradient statistic, by the output rank's class
         (up to 32, 64, 96); "bwd.apply_ng.partial_block" / "bwd.apply_ng.full_blocks": its last 128-row block was partial / every block whole;
     "bwd.repair"  backward sweeps called with the self-repair term on.
   Arguments and return value as tdnnf_gemm_launch_forms. */
int tdnnf_fused_launch_forms(long long *counts, int capacity, int reset);
const char *tdnnf_fused_launch_form_name(int index);

/* ---- TdnnDARTSV3Component coefficient flags (nnet-tdnn-component.cc:150-163) */
#define TDNNF_DARTS_USE_GUMBEL 1
#define TDNNF_DARTS_FREE_SELECT 2
#define TDNNF_DARTS_UNIFORM_SAMPLE 4
#define TDNNF_DARTS_USE_ENTROPY 8
#define TDNNF_DARTS_UPDATE_ALPHA 16

/* precomputed indexes: TdnnDARTSV3Component::PrecomputedIndexes
   (src/nnet3/nnet-convolutional-component.h:208-218) */
typedef struct {
  int row_stride;
  int num_offsets;
  int row_offsets[TDNNF_MAX_OFFSETS];
} tdnnf_tdnn_indexes;

/* ======================================================================= A1/A2
 * TdnnComponent / TdnnDARTSV3Component (src/nnet3/nnet-tdnn-component.cc).
 * linear_params_dev is Do x (K*Di) with row stride ldw (column block i = tap i).
 */

/* Coefficients of Propagate :250-289.  Reads log_alpha (bias_params_[0:K]),
   the K uniform draws for the Gumbel noise and ONE uniform draw for the tap
   sample; writes coef_memo_dev[K] (the memo of :330-332) and eff_coef_dev[K] (the
   weight each tap's GEMM gets in :292-328).  share_index per :232-240. */
int tdnnf_tdnn_darts_coef(const float *log_alpha_dev, int K, int flags, float temp_proportion,
                          const float *gumbel_u_dev, const float *sample_u_dev, int share_index,
                          float *coef_memo_dev, float *eff_coef_dev, tdnnf_stream stream);

/* Propagate :214-333 (plain TdnnComponent: eff_coef_dev == NULL, all ones).
   init_mode 0: out += ... (no bias, kPropagateAdds); 1: out = bias + ... (:233-235);
   2: out = 0 + ... (:238, reference quirk q1 for layers whose offsets[1] < 0). */
int tdnnf_tdnn_propagate(const tdnnf_tdnn_indexes *indexes, const tdnnf_mat *in,
                         const float *linear_params_dev, int ldw, int Do, int Di,
                         const float *bias_dev, const float *eff_coef_dev, int init_mode,
                         tdnnf_mat *out, tdnnf_stream stream);

/* Backprop, data part :366-416: in_deriv views += c_i * out_deriv * W_i (kBackpropAdds). */
int tdnnf_tdnn_backprop_data(const tdnnf_tdnn_indexes *indexes, const tdnnf_mat *out_deriv,
                             const float *linear_params_dev, int ldw, int Do, int Di,
                             const float *eff_coef_dev, tdnnf_mat *in_deriv, tdnnf_stream stream);

/* UpdateSimple :433-455 (raw gradient, is_gradient_ path): bias_acc += lr*colsum(dY),
   W_acc_i += lr * c_i * dY^T X_i.  workspace: tdnnf_tdnn_update_workspace_bytes(). */
size_t tdnnf_tdnn_update_workspace_bytes(int Do, int Di, int K, int num_rows);
int tdnnf_tdnn_update_simple(const tdnnf_tdnn_indexes *indexes, const tdnnf_mat *in_value,
                             const tdnnf_mat *out_deriv, int Do, int Di,
                             const float *eff_coef_dev, float lr, float *W_acc_dev, int ldw,
                             float *bias_acc_dev, void *workspace_dev, size_t workspace_bytes,
                             tdnnf_stream stream);

/* scratch of tdnnf_tdnn_darts_alpha_update: s_i (K doubles), then K x TDNNF_TAP_DOTS_SLABS row-slab partials (added in slab order) */
#define TDNNF_TAP_DOTS_SLABS 64
#define TDNNF_TAP_DOTS_DOUBLES(K) ((K) * (1 + TDNNF_TAP_DOTS_SLABS))

/* Architecture-logit update of UpdateNaturalGradient :490-590.  s_i = <X_i W_i^T, dY>
   is obtained as <dW_i, W_i> from tap_grad_dev (K blocks of dY^T X_i, Do x K*Di,
   UNSCALED by coefficients and lr), avoiding the reference's extra forward GEMM
   per tap (:534-539).  alpha_acc_dev = to_update->bias_params_[0:K]. */
int tdnnf_tdnn_darts_alpha_update(const float *tap_grad_dev, int ldg, const float *linear_params_dev,
                                  int ldw, int Do, int Di, int K, const float *coef_memo_dev,
                                  int flags, int share_index, float temp_proportion, float lr,
                                  float *alpha_acc_dev, double *tap_dots_dev /* TDNNF_TAP_DOTS_DOUBLES(K) doubles: the first K receive s_i */,
                                  tdnnf_stream stream);
/* (in TDNNF_DARTS_UNIFORM_SAMPLE mode no gradient is added -- the reference computes and discards it, :502-507 --
   only the trailing scalings :565-590 run; tap_grad_dev may then be NULL) */

/* UpdateNaturalGradient :457-626 -- the branch Backprop takes whenever use_natural_gradient_ is set and the component is
   not a gradient holder (:427-430), i.e. in every recipe.  Literal order of the reference: architecture-logit update
   (:490-590, as tdnnf_tdnn_darts_alpha_update), in_value_temp = [c_i X_i ..., 1] (:466-532; the share tap unscaled
   unless free_select, a zero-coefficient tap left zero), out_deriv_temp = out_deriv (:592), both preconditioned in
   place by the caller's OnlineNaturalGradient objects (:598-599), then with local_lrate = in_scale * out_scale *
   learning_rate: linear_params_ += local_lrate out_deriv_temp^T in_value_temp[:, :K Di] (:621-624) and
   bias_params_[K:] += local_lrate out_deriv_temp^T in_value_temp[:, K Di] (:606-616).
   Plain TdnnComponent (UPSTREAM): coef_memo_dev = eff_coef_dev = alpha_acc_dev = NULL (linear_params_dev unused).
   bias_acc_dev (Do floats = to_update->bias_params_ + K, or NULL when the component has no bias: no ones column),
   alpha_acc_dev (K floats = to_update->bias_params_).  coef_memo_dev / eff_coef_dev: the two halves of the memo
   tdnnf_tdnn_darts_coef wrote in Propagate.  learning_rate == 0 returns at once (:423-424).  Nothing synchronises:
   the two scales stay on the device (tdnnf_ng_scale_dev). */
size_t tdnnf_tdnn_update_natural_gradient_workspace_bytes(int Do, int Di, int K, int num_rows, int has_bias);
int tdnnf_tdnn_update_natural_gradient(const tdnnf_tdnn_indexes *indexes, const tdnnf_mat *in_value,
                                       const tdnnf_mat *out_deriv, int Do, int Di,
                                       const float *linear_params_dev, int ldw_params,
                                       const float *coef_memo_dev, const float *eff_coef_dev, int flags,
                                       int share_index, float temp_proportion,
                                       tdnnf_ng *preconditioner_in, tdnnf_ng *preconditioner_out,
                                       float learning_rate, float *W_acc_dev, int ldw, float *bias_acc_dev,
                                       float *alpha_acc_dev, void *workspace_dev, size_t workspace_bytes,
                                       tdnnf_stream stream);

/* ======================================================================= A3/A4
 * BatchNormComponent / BatchNormTestComponent (src/nnet3/nnet-normalize-component.cc) */

/* Column reductions (BatchNorm statistics, ReLU stats, bias/alpha column sums) are done in two
   deterministic stages through a caller-supplied scratch buffer of this size. */
size_t tdnnf_colreduce_workspace_bytes(int rows, int cols);

/* train-mode Propagate :421-452; memo_dev is the 5 x D Memo::mean_uvar_scale. */
int tdnnf_batchnorm_propagate(const tdnnf_mat *in, float epsilon, float target_rms, tdnnf_mat *out,
                              float *memo_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream);
/* train-mode Backprop :505-542 */
int tdnnf_batchnorm_backprop(const tdnnf_mat *out_value, const tdnnf_mat *out_deriv, float target_rms,
                             float *memo_dev, tdnnf_mat *in_deriv, void *workspace_dev, size_t workspace_bytes,
                             tdnnf_stream stream);
/* StoreStats :551-589; stats are double as in the reference (h:458-462); stats_dev = [count, sum[D], sumsq[D]] */
int tdnnf_batchnorm_store_stats(const float *memo_dev, int D, int num_frames, double *stats_dev,
                                tdnnf_stream stream);
/* ComputeDerived :682-715 -> scale_dev[D], offset_dev[D] */
int tdnnf_batchnorm_compute_derived(const double *stats_dev, int D, float epsilon, float target_rms,
                                    float *scale_dev, float *offset_dev, tdnnf_stream stream);
/* BatchNormTestComponent::Propagate :872-874 / Backprop :919-920 */
int tdnnf_batchnorm_test_propagate(const tdnnf_mat *in, const float *scale_dev, const float *offset_dev,
                                   tdnnf_mat *out, tdnnf_stream stream);
int tdnnf_batchnorm_test_backprop(const tdnnf_mat *out_deriv, const float *scale_dev, tdnnf_mat *in_deriv,
                                  tdnnf_stream stream);

/* ========================================================================== A5
 * DARTS mixing ops (src/nnet3/nnet-simple-component.cc) */

/* SoftmaxFlopsComponent::Propagate :9968-9981 (gumbel_u_dev NULL, temp 1) and
   GumbelSoftmax[Flops]Component::Propagate :10088-10113 / :9774-9799. */
int tdnnf_softmax_flops_propagate(const tdnnf_mat *in, const float *gumbel_u_dev, float temp_proportion,
                                  tdnnf_mat *out, tdnnf_stream stream);
/* Backprop :9984-10020 / :10116-10158: out_deriv[:, :dim] += scale/(rows*cols)*flops (IN PLACE, as the
   reference does), in_deriv = DiffSoftmax(out_value, out_deriv) / temp.  flops_dev NULL = no penalty. */
int tdnnf_softmax_flops_backprop(const tdnnf_mat *out_value, tdnnf_mat *out_deriv, float scale,
                                 const float *flops_dev, int dim, float temp_proportion,
                                 tdnnf_mat *in_deriv, tdnnf_stream stream);
/* OnehotFunctionComponent::Propagate :9504-9519 (one uniform draw, device) */
int tdnnf_onehot_propagate(const float *sample_u_dev, tdnnf_mat *out, tdnnf_stream stream);
/* OnehotFunctionComponent::Backprop :9521-9552, non-natural-gradient branch (the recipes' configuration
   "is-updatable=true use-natural-gradient=false"): output_ += lr * colsum(out_deriv); no input derivative.
   workspace: tdnnf_colreduce_workspace_bytes(rows, cols). */
int tdnnf_onehot_backprop(const tdnnf_mat *out_deriv, float lr, float *output_acc_dev, void *workspace_dev,
                          size_t workspace_bytes, tdnnf_stream stream);
/* CopyNComponent :4843-4867 (AddMatBlocks: both directions ADD) */
int tdnnf_copyn_propagate(const tdnnf_mat *in, float scale, tdnnf_mat *out, tdnnf_stream stream);
int tdnnf_copyn_backprop(const tdnnf_mat *out_deriv, float scale, tdnnf_mat *in_deriv, tdnnf_stream stream);
/* ConstantFunctionComponent :2602-2642 (non-NG branch: output += 5*lr*colsum) */
int tdnnf_constant_function_propagate(const float *output_dev, tdnnf_mat *out, tdnnf_stream stream);
int tdnnf_constant_function_backprop(const tdnnf_mat *out_deriv, float lr, float *output_acc_dev,
                                     void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream);
/* FlopsConstraintComponent::Backprop :9465-9478 */
int tdnnf_flops_constraint_backprop(const float *flops_dev, float scale, int rows_in, int cols_in,
                                    tdnnf_mat *in_deriv, tdnnf_stream stream);

/* ========================================================================== A6 */
/* ElementwiseProductComponent :256-299 */
int tdnnf_elementwise_product_propagate(const tdnnf_mat *in, int output_dim, tdnnf_mat *out, tdnnf_stream);
int tdnnf_elementwise_product_backprop(const tdnnf_mat *in_value, const tdnnf_mat *out_deriv, int output_dim,
                                       tdnnf_mat *in_deriv, tdnnf_stream);
/* RectifiedLinearComponent :958-1091 */
int tdnnf_relu_propagate(const tdnnf_mat *in, tdnnf_mat *out, tdnnf_stream);
int tdnnf_relu_backprop(const tdnnf_mat *out_value, const tdnnf_mat *out_deriv, tdnnf_mat *in_deriv, tdnnf_stream);
/* RepairGradients :990-1074 after the coin flip; stats_dev = [count, value_sum[D], deriv_sum[D]] doubles */
int tdnnf_relu_repair(const double *stats_dev, int dim, float self_repair_scale, float lower, float upper,
                      tdnnf_mat *in_deriv, tdnnf_stream);
int tdnnf_relu_store_stats(const tdnnf_mat *out_value, double *stats_dev, void *workspace_dev,
                           size_t workspace_bytes, tdnnf_stream);
/* AffineComponent :1235-1279 / LinearComponent :3211-3254 (bias_dev NULL).  Same MFMA kernels as Tdnn. */
int tdnnf_affine_propagate(const tdnnf_mat *in, const float *W_dev, int ldw, const float *bias_dev, int Do,
                           tdnnf_mat *out, tdnnf_stream);
int tdnnf_affine_backprop(const tdnnf_mat *out_deriv, const float *W_dev, int ldw, int Di, tdnnf_mat *in_deriv,
                          tdnnf_stream);
int tdnnf_affine_update_simple(const tdnnf_mat *in_value, const tdnnf_mat *out_deriv, float lr, float *W_acc_dev,
                               int ldw, float *bias_acc_dev, void *workspace_dev, size_t workspace_bytes,
                               tdnnf_stream);
/* NaturalGradientAffineComponent::Update :2980-3024 (bias_acc_dev != NULL) and the natural-gradient branch of
   LinearComponent::Backprop :3240-3243 (bias_acc_dev == NULL: no ones column): [X, 1] and a copy of out_deriv are
   preconditioned by the caller's two OnlineNaturalGradient objects, W += lr a b dY'^T X', bias += lr a b dY'^T 1'. */
size_t tdnnf_affine_update_natural_gradient_workspace_bytes(int Do, int Di, int num_rows, int has_bias);
int tdnnf_affine_update_natural_gradient(const tdnnf_mat *in_value, const tdnnf_mat *out_deriv,
                                         tdnnf_ng *preconditioner_in, tdnnf_ng *preconditioner_out,
                                         float learning_rate, float *W_acc_dev, int ldw, float *bias_acc_dev,
                                         void *workspace_dev, size_t workspace_bytes, tdnnf_stream);
/* LogSoftmaxComponent :3607-3632 */
int tdnnf_log_softmax_propagate(const tdnnf_mat *in, tdnnf_mat *out, tdnnf_stream);
int tdnnf_log_softmax_backprop(const tdnnf_mat *out_value, const tdnnf_mat *out_deriv, tdnnf_mat *in_deriv,
                               tdnnf_stream);
/* out = sa*a + sb*b  (descriptor Sum(Scale(..), ..) into NoOpComponent, composite_layers.py:205-213);
   b may be NULL (plain scaled copy).  In-place (out aliasing a or b) is allowed. */
int tdnnf_sum_scaled(const tdnnf_mat *a, float sa, const tdnnf_mat *b, float sb, tdnnf_mat *out, tdnnf_stream);
/* out += s * a */
int tdnnf_add_scaled(const tdnnf_mat *a, float s, tdnnf_mat *out, tdnnf_stream);
/* GeneralDropoutComponent (UPSTREAM), continuous mask shared over time: row r uses mask row r % num_seq */
int tdnnf_general_dropout(const tdnnf_mat *in, const float *mask_dev, int num_seq, tdnnf_mat *out, tdnnf_stream);
/* GeneralDropoutComponent::GetMemo (UPSTREAM; factory /root/reference/src/nnet3/nnet-component-itf.cc:194): the mask from n uniform
   draws -- continuous: 1 - 2p + 4p U (expected value 1); otherwise Heaviside(U - p) / (1 - p) */
int tdnnf_general_dropout_mask(const float *uniform_dev, long long n, float proportion, int continuous, float *mask_dev, tdnnf_stream);

/* ========================================================================== A7
 * chain::ComputeChainObjfAndDeriv (UPSTREAM; options from
 * local/chain_NAS/run_TDNN_DARTSV3_fbk_stride_pretrain.sh:185-195). */
typedef struct tdnnf_den_graph tdnnf_den_graph;       /* device-resident denominator HMM */
typedef struct tdnnf_supervision tdnnf_supervision;   /* device-resident numerator graphs of one minibatch */

/* host arrays in, device copy out.  initial_probs may be NULL (computed as 100-step average occupancy
   from start_state, DenominatorGraph::SetInitialProbs). */
int tdnnf_den_graph_create(int num_states, int num_arcs, int num_pdfs, const int *arc_src, const int *arc_dst,
                           const int *arc_pdf, const float *arc_prob, const float *initial_probs, int start_state,
                           tdnnf_den_graph **out);
void tdnnf_den_graph_destroy(tdnnf_den_graph *);
int tdnnf_supervision_create(int num_sequences, int frames_per_sequence, const int *seq_state_begin,
                             const int *seq_arc_begin, const int *state_time, const float *final_logprob,
                             const int *arc_src, const int *arc_dst, const int *arc_pdf, const float *arc_logprob,
                             float weight, tdnnf_supervision **out);
void tdnnf_supervision_destroy(tdnnf_supervision *);
/* What a supervision may be: per sequence ANY time-synchronous acceptor over frames 0 .. frames_per_sequence -- every arc goes from a state
   of time t to one of time t + 1, the states of a sequence are sorted by time and its first state is its only state of time 0.  There is no
   bound on the number of states or arcs per frame (alignments, lattices with a frame tolerance, several alternative transcripts).  A
   supervision of more than 4 * (frames_per_sequence + 1) states per sequence on average holds its own numerator scratch on the device
   (16 bytes per state) and a second copy of its arcs (20 bytes per arc); the chain workspace does not depend on the supervision.
   Any of the out-pointers may be NULL; *wide: 1 if the supervision is over that mark.
   A supervision of this kind is either CREATED (above: one minibatch for its lifetime) or RESERVED and assigned a minibatch at a time
   (below); the functions that take a supervision do not tell the two apart. */
int tdnnf_supervision_info(const tdnnf_supervision *, int *num_states, int *num_arcs, int *max_states_per_frame, int *wide);
/* The time-synchronous kind, REUSABLE: the egs readers give a new supervision every minibatch, and tdnnf_supervision_create builds its
   tables on the host, allocates and copies synchronously array by array and (at destroy) waits for the whole device array by array.
   tdnnf_supervision_reserve makes every allocation once, for minibatches of at most max_sequences sequences of at most max_frames frames
   with max_states states and max_arcs arcs between them: every array a supervision of this kind can carry -- the second copy of the arcs
   ordered by pdf within a frame and the numerator's own scratch included, whatever the minibatch's width -- the build's scratch and a
   device staging area in ONE device allocation (48 bytes per state, 72 per arc, 8 per (sequence, frame + 2), 8 per (sequence, 8 frames)
   and 2 KB), and two pinned staging buffers (8 bytes per state, 16 per arc, 4 per (sequence, frame + 2) each) with an event each.
   Until the first assign it holds no minibatch, and every function that takes a supervision refuses it (TDNNF_EINVAL naming
   tdnnf_supervision_assign).
   tdnnf_supervision_assign gives it the next minibatch in stream order, with the arrays of tdnnf_supervision_create.  On the host,
   O(states + arcs + sequences * frames): what tdnnf_supervision_create refuses is refused in the same words under this entry's name
   (and, because the device build indexes by them, begin arrays that do not start at 0 or a seq_arc_begin that decreases); a minibatch over
   a capacity is refused naming the capacity, its value and the excess; the widths and `wide` are found as tdnnf_supervision_create finds
   them.  A refused assign leaves the supervision on its previous minibatch (an error of the runtime behind this point, TDNNF_EHIP from a
   copy or a launch, leaves it without one: refused like a fresh handle until an assign succeeds -- the failure rule of
   tdnnf_align_graphs_assign below).  Then the raw arrays are staged in pinned memory, and their
   copies and two build kernels are enqueued on `stream`: the by-destination and by-source lists in original arc order and the per-frame
   lists ordered stably by pdf, byte for byte what tdnnf_supervision_create uploads.  Nothing is allocated, freed or waited for
   device-wide; the only wait is for the copies of the assign before last out of the staging buffer that is written again.  Work enqueued
   on `stream` before the assign still sees the previous minibatch; work that uses the supervision on ANOTHER stream must be ordered
   against `stream` by the caller.  num_sequences, frames_per_sequence, weight, the counts and `wide` follow the minibatch; the numerator
   takes the form and the scratch it takes for a created supervision of the same arrays (option "num_form" 2 works for any assigned
   minibatch), and gives the same bits.
   tdnnf_supervision_capacity: the four capacities, the assigns so far, the device and pinned allocations made for the handle since
   tdnnf_supervision_reserve returned (0, always) and the bytes of the device allocation; any out-pointer may be NULL.  TDNNF_EINVAL for a
   supervision that tdnnf_supervision_reserve did not make. */
int tdnnf_supervision_reserve(int max_sequences, int max_frames, int max_states, int max_arcs, tdnnf_supervision **out);
int tdnnf_supervision_assign(tdnnf_supervision *, int num_sequences, int frames_per_sequence, const int *seq_state_begin,
                             const int *seq_arc_begin, const int *state_time, const float *final_logprob, const int *arc_src,
                             const int *arc_dst, const int *arc_pdf, const float *arc_logprob, float weight, tdnnf_stream stream);
int tdnnf_supervision_capacity(const tdnnf_supervision *, int *max_sequences, int *max_frames, int *max_states, int *max_arcs, int *assigns,
                               int *allocations_since_reserve, long long *device_bytes);
/* diagnostics (tests), time-synchronous kind, created or assigned: one device table by name, copied to host memory as 4-byte elements --
   "seq_state_begin", "state_time", "final_logprob", "frame_state_begin", "in_begin", "in_src", "in_pdf", "in_lp", "out_begin", "out_dst",
   "out_pdf", "out_lp", "pf_src", "pf_dst", "pf_pdf", "pf_t", "pf_lp" (ints; the three *_lp and final_logprob are floats).  *count: the
   table's elements, 0 for a table the supervision does not carry (pf_* of a narrow created one); out NULL: the size query alone.
   Synchronises `stream` (and the stream of the last assign) itself. */
int tdnnf_supervision_dump(const tdnnf_supervision *, const char *table, void *out, long long capacity, long long *count, tdnnf_stream stream);
/* The second kind of supervision: flat-start ("end-to-end") LF-MMI, Kaldi's GenericNumeratorComputation branch of
   chain::ComputeChainObjfAndDeriv.  Per sequence ONE cyclic, epsilon-free acceptor with pdf-ids on its arcs (a transcript graph with
   self-loops), every path of exactly frames_per_sequence arcs from an initial to a final state counts.  Host arrays in, device copy out;
   state and arc numbering and the -inf conventions are tdnnf_align_graphs_create's (below): sequence s owns the states
   [seq_state_begin[s], seq_state_begin[s + 1]) and the arcs [seq_arc_begin[s], seq_arc_begin[s + 1]).  TDNNF_EINVAL as there: a pdf outside
   [0, num_pdfs), a state outside its sequence, a sequence with no initial or no final state.  A graph without a path of exactly
   frames_per_sequence arcs is NOT refused here: its sequence's log-prob is -inf at run time, which is the objective's failure path
   ([0] = -10 * weight * B * T, [5] = 0, [6] = 0, both derivative matrices zero).
   Every function that takes a tdnnf_supervision works with this kind (the chain entries below, tdnnf_net_forward_backward,
   tdnnf_net_objective); they require num_pdfs <= the denominator graph's.  With y_t = row t * B + s of nnet_output, all in double
   (tdnnf_align_posteriors' arithmetic with acoustic_scale 1, see "forward-backward" below):
     term(arc, t) = arc_logprob + y_t[arc_pdf]          no clamp
     alpha_0 = initial_logprob;  alpha_t+1[d] = LSE over arcs into d of alpha_t[src] + term(arc, t)
     num_lp[s] = LSE_st alpha_T[st] + final_logprob[st]
     beta_T = final_logprob;     beta_t[st] = LSE over arcs out of st of term(arc, t) + beta_t+1[dst]
     gamma[t, p] = sum over arcs with pdf p of exp(alpha_t[src] + term + beta_t+1[dst] - num_lp[s])
   results[3] = weight * sum_s num_lp[s]; nnet_output_deriv[row, p] += (float)(weight * gamma) on top of the denominator's term (elements
   whose pdf no arc of the sequence names are not touched); xent_deriv gets xent_regularize times the same float; results[6] = the sum of
   that float times xent_output[row, p].  One owner per (t, p), no atomics: two calls give the same bits.
   The device copy holds the arcs three times (48 bytes an arc, as a tdnnf_align_graphs) and the numerator's scratch, alpha_t and beta_t
   of every frame:  16 * (frames_per_sequence + 1) * sum_s S_s bytes  [+ 16 * sum_s S_s where the two state vectors of the recursion do
   not live in LDS: option "align_form" 2, or a graph of more than about 9 600 states; the option is read HERE] -- 150 output frames x
   128 transcripts of 200 states: 62 MB.  The chain workspace formulas do not change.
   tdnnf_supervision_info: the total states and arcs, max_states_per_frame = the largest graph's states, wide = 0.
   Not built: reading end-to-end egs (the egs readers below still refuse <End2End> supervisions), transition-id level output.  Graphs
   from transcripts: tdnnf_supervision_assign_e2e_transcripts below, for a reserved supervision.  All sequences of a call share frames_per_sequence. */
int tdnnf_supervision_create_e2e(int num_sequences, int frames_per_sequence, int num_pdfs, const int *seq_state_begin, const int *seq_arc_begin,
                                 const int *arc_src, const int *arc_dst, const int *arc_pdf, const float *arc_logprob,
                                 const float *initial_logprob, const float *final_logprob, float weight, tdnnf_supervision **out);
/* The same kind, REUSABLE: flat-start training has new transcripts in every minibatch, and tdnnf_supervision_create_e2e allocates, copies
   synchronously and (at destroy) waits for the whole device every time.  tdnnf_supervision_reserve_e2e makes every allocation once -- a
   reserved graph set (tdnnf_align_graphs_reserve below: max_sequences graphs, max_states states and max_arcs arcs between them) and the
   numerator's scratch at the capacities, 16 * (max_frames + 1) * max_states bytes, plus the two state vectors (16 * max_states, always:
   the launch form now follows the minibatch).  tdnnf_supervision_assign_e2e gives it the next minibatch in stream order, with the arrays of
   tdnnf_supervision_create_e2e: num_sequences, frames_per_sequence, weight and the graphs may all change, within the capacities
   (TDNNF_EINVAL naming the capacity and the excess: max_sequences, max_frames here, max_states and max_arcs from tdnnf_align_graphs_assign,
   which also validates the arrays; a refused assign leaves the supervision on its previous minibatch, and where an error of the runtime
   leaves the graph set without a batch -- tdnnf_align_graphs_assign's failure rule -- the supervision holds no minibatch either).  The launch form of the recursion is
   planned here from the minibatch's largest graph (option "align_form" is read HERE).  No allocation, no free, no device-wide wait; stream
   order as tdnnf_align_graphs_assign documents.  Every function that takes a supervision runs what it runs for a created one and gives the
   same bits; before the first assign they refuse it. */
int tdnnf_supervision_reserve_e2e(int max_sequences, int max_frames, int num_pdfs, int max_states, int max_arcs, tdnnf_supervision **out);
int tdnnf_supervision_assign_e2e(tdnnf_supervision *, int num_sequences, int frames_per_sequence, const int *seq_state_begin,
                                 const int *seq_arc_begin, const int *arc_src, const int *arc_dst, const int *arc_pdf, const float *arc_logprob,
                                 const float *initial_logprob, const float *final_logprob, float weight, tdnnf_stream stream);
/* tdnnf_supervision_assign_e2e from transcripts: the next minibatch of a supervision of tdnnf_supervision_reserve_e2e compiled on the
   device from unit sequences ("transcript graphs" below: the unit set, the slots, the graph of a transcript and what is refused;
   tdnnf_align_graphs_assign_transcripts does the work on the supervision's graph set).  num_sequences transcripts, one per sequence.
   The capacities, the launch form planned from the largest graph, stream order and what a refusal leaves in place are
   tdnnf_supervision_assign_e2e's.  A transcript with more mandatory slots than frames_per_sequence is not refused: the objective's
   failure path, as for any graph without an accepting path of that length. */
int tdnnf_supervision_assign_e2e_transcripts(tdnnf_supervision *, const struct tdnnf_unit_set *units, int num_sequences, int frames_per_sequence,
                                             const int *slot_begin, const int *slot_unit, const int *slot_optional, float weight,
                                             tdnnf_stream stream);
/* 0 time-synchronous (tdnnf_supervision_create), 1 end-to-end (tdnnf_supervision_create_e2e); -1 for NULL */
int tdnnf_supervision_kind(const tdnnf_supervision *);
/* diagnostics, end-to-end kind only: the launch form of its recursion -- threads per workgroup (64 up to 64 states in the largest graph,
   256 up to 1024, 1024 above), whether the two state vectors live in LDS, whether the output rows are staged in LDS one frame ahead
   (two rows of num_pdfs floats fit beside the vectors and num_pdfs <= 8 * threads).  Any out-pointer may be NULL. */
int tdnnf_supervision_e2e_form(const tdnnf_supervision *, int *threads, int *vectors_in_lds, int *rows_in_lds);

/* The denominator recursion has two forms: one persistent workgroup per sequence with the state vectors in LDS (graphs up
   to ~10 000 states), and one launch per frame over all sequences on sequence-minor arrays (larger graphs).  0 = chosen by
   graph size (default), 1 / 2 force one (tests, experiments); 3 = the persistent form with ONE workgroup per sequence even for
   few sequences (otherwise up to 32 sequences take four workgroups each, which must be co-resident: checked against the
   occupancy calculator before the launch, a bounded poll behind it, and the one-workgroup kernels redo a minibatch whose
   multi-workgroup launch gave up -- reported on stderr once, not used again in the process); 4 = persistent, forward then
   one-kernel backward on one stream (the trainer's den_split 0 form): tdnnf_chain_objf_and_deriv runs the forward recursion and
   then ONE kernel for the backward recursion and the occupancies, where modes 1 and 3 run the two recursions side by side and an
   occupancy pass over all frames; plan, workspace size and the fallback to state vectors in global memory are mode 1's, and
   tdnnf_chain_objf is unaffected.  Affects the workspace size: set it before tdnnf_chain_workspace_bytes / tdnnf_net_create. */
int tdnnf_chain_set_denominator_mode(int mode);
/* diagnostics: minibatches the one-workgroup kernels redid behind a multi-workgroup launch that gave up; whether that form is switched off for
   the process; reset != 0 clears both (synchronises the device) */
int tdnnf_chain_den_mw_status(int *fallbacks, int *disabled, int reset);
size_t tdnnf_chain_workspace_bytes(const tdnnf_den_graph *, int num_sequences, int frames_per_sequence);
/* diagnostics: bytes at the END of a workspace of tdnnf_chain_workspace_bytes that only the side-by-side recursions and their occupancy pass
   touch (0 where the plan has no such form).  The one-kernel backward pass (mode 4, the trainer's den_split 0) leaves them alone, which is
   why a trainer that never runs the side-by-side form allocates that much less. */
size_t tdnnf_chain_split_region_bytes(const tdnnf_den_graph *, int num_sequences, int frames_per_sequence);
/* results_dev (device doubles): [0] objf, [1] l2_term, [2] weight, [3] num logprob (weighted),
   [4] den logprob (weighted), [5] ok flag (1.0 / 0.0), [6] xent objf when xent_output given.
   nnet_output_deriv is OVERWRITTEN; xent_deriv (may be NULL) receives the numerator posteriors
   already multiplied by xent_regularize (NnetChainTrainer::ProcessOutputs).
   The l2 term is summed in a fixed order (per-workgroup partial sums in 2 KB that every supervision owns, added in ascending order): two
   calls on the same inputs give the same bits in results_dev[1], with either kind of supervision. */
int tdnnf_chain_objf_and_deriv(const tdnnf_den_graph *, const tdnnf_supervision *, const tdnnf_mat *nnet_output,
                               const tdnnf_mat *xent_output /* may be NULL */, float leaky_hmm_coefficient,
                               float l2_regularize, float xent_regularize, double *results_dev,
                               tdnnf_mat *nnet_output_deriv, tdnnf_mat *xent_deriv, void *workspace_dev,
                               size_t workspace_bytes, tdnnf_stream);
/* The objective alone -- chain::ComputeChainObjfAndDeriv with null derivative pointers, what nnet3-chain-compute-prob and
   nnet3-chain-combine call.  results_dev as above, the failure path included (an objf that is not finite: [0] = -10 * weight, [5] = 0,
   [6] = 0); nothing but results_dev and the workspace is written.  nnet_output and xent_output may be sub-matrix views.
   The denominator runs its forward recursion only and keeps no alpha per frame: the persistent form alternates between two state
   vectors (in LDS, or in the workspace for graphs whose vectors do not fit), the wide form between two alpha frames.  The form follows
   tdnnf_chain_set_denominator_mode and the graph's size as for tdnnf_chain_objf_and_deriv, except that the persistent form is ALWAYS one
   workgroup per sequence (modes 1 and 3 are the same here): an evaluation call should not need its workgroups co-resident, as the
   multi-workgroup recursion does, and its result should not depend on how many sequences the minibatch has, as the choice of that
   recursion does.  Everything runs on the caller's stream.  The numerator runs its recursion, and its posterior pass only when
   xent_output is given (it then forms the xent objective and writes no posterior matrix).
   The workspace holds the per-sequence sums, the numerator's scratch and the denominator's two vectors (wide form: also its
   transposed exp(nnet_output) and partial rows) -- at 4 000 states, 128 x 500 frames a few MB against 1 GB; a workspace of
   tdnnf_chain_workspace_bytes is never smaller and is accepted too.  The l2 term is summed in a fixed order: two calls give the same bits. */
size_t tdnnf_chain_objf_workspace_bytes(const tdnnf_den_graph *, int num_sequences, int frames_per_sequence);
int tdnnf_chain_objf(const tdnnf_den_graph *, const tdnnf_supervision *, const tdnnf_mat *nnet_output,
                     const tdnnf_mat *xent_output /* may be NULL */, float leaky_hmm_coefficient, float l2_regularize,
                     double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream);
/* diagnostics (tools/num_bench.py): ONE part of the numerator's work as tdnnf_chain_objf_and_deriv enqueues it -- part 1 the forward-backward
   recursion, 4 the posterior pass behind the xent head (xent_deriv, xent objective), 2 the pass that adds the posteriors to nnet_output_deriv
   (with the kernels that finish the objective).  Parts 4 and 2 read what part 1 left in the workspace / the supervision. */
int tdnnf_chain_numerator_part(const tdnnf_den_graph *, const tdnnf_supervision *, const tdnnf_mat *nnet_output, int part, double *results_dev,
                               tdnnf_mat *nnet_output_deriv, tdnnf_mat *xent_deriv, void *workspace_dev, size_t workspace_bytes, tdnnf_stream);

/* ------------------------------------------------------------------ A7, best-path alignment
 * The best path (Viterbi) of a cyclic, epsilon-free acceptor with pdf-ids on its arcs, scored on rows of the model's output: forced
 * alignment on transcript graphs (what nnet3-align-compiled | ali-to-pdf prints) and the free best path through the denominator graph.
 * Not a decoder: no beam, no lattice.  Graphs are the caller's arrays, or compiled on the device from unit sequences for the chain
 * topology (tdnnf_align_graphs_assign_transcripts below); lexicon and tree handling stay the caller's job.  Transition-ids, phones and word positions
 * are the caller's: a second integer per arc, the arc's LABEL (tdnnf_align_graphs_create_labelled), which the labelled entries below report
 * per frame (tdnnf_align_best_path_labels) and form posteriors over (tdnnf_align_label_posteriors_compact / _sparse).
 *
 *   term(arc, t)  = (double)arc_logprob + (double)acoustic_scale * (double)y[t, arc_pdf]
 *   alpha_0[s]    = (double)initial_logprob[s]
 *   alpha_t+1[d]  = max over arcs into d of  alpha_t[src] + term(arc, t)
 *   score         = max over s of  alpha_T[s] + (double)final_logprob[s]
 * No clamp on y.  -inf marks "not reachable" / "not final"; an arc is a candidate only if its sum is greater than -inf (a NaN never is).
 * Ties: among equal candidates the arc that comes first in the caller's arc list wins; among equal final states the lowest state.
 * An utterance with no accepting path of its length gets ok = 0, score = -inf and every pdf-id (and state) -1, the other utterances of the
 * call are unaffected; a score that is not finite for another reason (+inf) gives ok = 0 and the -1s too.
 *
 * One workgroup per utterance walks its frames; the state scores are doubles, two vectors alternating, in LDS when 2 * S * 8 bytes fit
 * (about 9 600 states), in the workspace otherwise.  Option "align_form": 0 (default) chosen by size, 1 LDS, 2 workspace (read by
 * tdnnf_align_workspace_bytes and tdnnf_align_best_path alike: set it before both).  The workgroup has 64 threads when the largest graph
 * that an utterance of the call names has at most 64 states, 256 up to 1024 states, 1024 above.  In the LDS form the output row of the
 * next frame is loaded coalesced one frame ahead and gathered from LDS where two rows of num_pdfs floats fit beside the vectors and
 * num_pdfs <= 8 * threads; otherwise y[t, pdf] is gathered from global memory.  Same results either way.
 *
 * Back-pointer checkpointing (option "align_path_checkpoint", default 0 = off; read by the workspace question and by both calls: set it
 * before both).  The back-pointers are 4 * T * S bytes an utterance.  With an interval C >= 1 (or -1: one C for the call,
 * ceil(sqrt(its longest utterance's frames)), at least 1; a C above the longest utterance counts as that length) an utterance is cut into
 * the segments [kC, min(kC + C, T)); the forward pass stores alpha_kC of every segment start -- one CHECKPOINT of S doubles -- and keeps
 * back-pointers only in a buffer of min(C, T) frames, each segment over the one before.  The trace-back walks the last segment as the
 * forward pass left it, then for every earlier segment, from the last to the first, reloads its checkpoint, reruns its C frames into the
 * buffer and walks on; the chosen arc of every frame goes to a path of T ints.  The rerun is the forward pass's own step on the same
 * doubles in the same order: pdfs, states, labels, arcs, score and ok flag are those of option 0, in every form
 * (tests/test_gpu_align_checkpoint.py).  T <= C is one segment and recomputes nothing.  The arcs are swept 2 - 1/ceil(T / C) times where
 * option 0 sweeps them once; measured 1.7 x (64 x 500 frames on 301-state transcript graphs) and 1.9 x (128 x 500 on the 4 000-state
 * graph) the option-0 time at -1.  At C = 1 the region is LARGER than option 0's (8 S T against 4 S T bytes): the caller chooses. */
typedef struct tdnnf_align_graphs tdnnf_align_graphs; /* device-resident set of graphs */

/* host arrays in, device copy out.  States are numbered as tdnnf_supervision_create numbers a sequence's: graph g owns the states
   [graph_state_begin[g], graph_state_begin[g + 1]) and the arcs [graph_arc_begin[g], graph_arc_begin[g + 1]); arc_src / arc_dst are these
   global state numbers; initial_logprob / final_logprob have one entry per state (-inf: not initial / not final).
   TDNNF_EINVAL: a pdf outside [0, num_pdfs) (so: an epsilon arc), a state outside its graph, a graph without a state whose
   initial_logprob is above -inf or without one whose final_logprob is.  The device copy holds the arcs three times -- by destination
   (best path, forward recursion), by source (backward recursion) and by pdf (posteriors) -- 48 bytes an arc plus the padding of the slices. */
int tdnnf_align_graphs_create(int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                              const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob,
                              const float *final_logprob, tdnnf_align_graphs **out);
/* The same with one caller-defined label per arc: arc_label has one int per arc in the caller's arc order, every value in [0, num_labels)
   (else TDNNF_EINVAL, naming the arc) -- a transition-id, a phone, a word position, the arc's own index.  The handle serves every entry that
   takes a tdnnf_align_graphs with the bits of an unlabelled handle of the same graphs, and the label entries, which refuse an unlabelled
   handle with TDNNF_EINVAL.  Memory on top of the above: a fourth copy of the arcs, by label (16 bytes an arc plus the padding of the
   slices; the entry carries the arc's pdf where the other tables carry its index), 4 bytes an arc for the labels themselves, and per graph
   the ascending list of its distinct labels (4 bytes a label on the host and on the device) and 20 bytes of ranges and counts. */
int tdnnf_align_graphs_create_labelled(int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                                       const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob,
                                       const float *final_logprob, const int *arc_label, int num_labels, tdnnf_align_graphs **out);
void tdnnf_align_graphs_destroy(tdnnf_align_graphs *);
/* A REUSABLE graph set: allocated once for a capacity, then assigned a new batch of graphs per call in stream order -- forced alignment of a
   corpus has new transcript graphs for every batch of utterances, and tdnnf_align_graphs_create allocates, copies synchronously and (at
   destroy) waits for the whole device every time.
   tdnnf_align_graphs_reserve makes every allocation the handle will ever need: max_graphs graphs with max_states states and max_arcs arcs
   BETWEEN them (totals over a batch); num_labels 0 reserves an unlabelled handle, > 0 one whose every batch carries labels.  ONE device
   allocation holds the per-state and per-arc arrays, the tables at their bounds (per table and graph at most 63 empty slots and 63 * 64
   padding entries on top of the rows and arcs: csrc/align_tables.h align_table_bound), the column lists, the build's scratch and the device
   staging -- about 75 bytes a state, 125 bytes an arc (185 with labels) and 197 KB a graph of capacity (262 KB with labels: the padding bound
   of three or four tables); two pinned host buffers of 28 bytes an arc and 8 a state stage the batches.  The device pointers never change afterwards.  Until the first assign the handle holds no graphs, and every
   entry that takes it refuses with TDNNF_EINVAL and says so.
   tdnnf_align_graphs_assign takes the eight host arrays of tdnnf_align_graphs_create and arc_label (non-NULL exactly when the handle was
   reserved with labels), validates what create validates with the same messages under its own name, and refuses a batch beyond one of the
   three capacities with TDNNF_EINVAL, naming the capacity and the excess.  All checks run before anything is written: a refused assign
   leaves the handle serving its previous batch.  ONE FAILURE RULE for every assign of a reserved handle (this one,
   tdnnf_align_graphs_assign_transcripts, tdnnf_supervision_assign): from the first enqueued copy until the call succeeds the handle holds
   NO batch, so an error of the runtime behind that point (TDNNF_EHIP from a copy or a launch, when the tables are already being
   overwritten) leaves a handle that every entry refuses like a fresh one until an assign succeeds.  It then copies the arrays into pinned staging, enqueues asynchronous copies and three
   kernels on `stream` that build the tables on the device -- the bytes tdnnf_align_graphs_create uploads for the same arrays, so every
   entry gives the same bits -- and returns.  No allocation, no free, no device-wide or stream-wide wait; the one host wait there can be is
   for the staging copy of the assign BEFORE LAST (the two staging buffers take turns).  The host arrays may be reused when it returns.
   Calls enqueued on `stream` before the assign still see the previous batch, calls enqueued on it afterwards the new one; a call on another
   stream must be ordered against the assign by the caller (an event), in both directions.  The host-side answers (tdnnf_align_graphs_info,
   _pdfs, _labels, workspace and layout questions) follow the new batch at once.  A handle of tdnnf_align_graphs_create* is refused.  Not
   capturable into a HIP graph (host validation and staging). */
int tdnnf_align_graphs_reserve(int max_graphs, int num_pdfs, int num_labels /* 0: unlabelled */, int max_states, int max_arcs,
                               tdnnf_align_graphs **out);
int tdnnf_align_graphs_assign(tdnnf_align_graphs *, int num_graphs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                              const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob,
                              const float *final_logprob, const int *arc_label /* NULL iff unlabelled */, tdnnf_stream stream);
/* reserved handles only: the three capacities, the bytes of the handle's device allocation, the number of device allocations made for it
   since it exists (the witness that assign makes none) and the assigns that succeeded.  Any out-pointer may be NULL. */
int tdnnf_align_graphs_capacity(const tdnnf_align_graphs *, int *max_graphs, int *max_states, int *max_arcs, long long *device_bytes,
                                int *device_allocs, int *assigns);
/* TRANSCRIPT GRAPHS: a reserved handle's batch compiled on the device from unit (phone) sequences, so that the caller hands over
   transcripts and never builds an arc array.
   A UNIT SET is made once and is device-resident: num_units units over num_pdfs pdfs with the chain topology -- one state per unit, an
   entry pdf on its first frame, a loop pdf on every later frame.  context 0 (context-independent): entry_pdf and loop_pdf have num_units
   ints each.  context 1 (left-biphone): (num_units + 1) * num_units ints each, at index (left + 1) * num_units + u, left = -1 meaning
   "nothing before it".  loop_logprob[u] and leave_logprob[u] (num_units floats each) weigh the self-loop and EVERY arc that leaves the
   unit (for a transcript's last unit: its final weight); take_logprob and skip_logprob apply to a slot marked optional when it is taken or
   skipped (optional silence).  TDNNF_EINVAL: a pdf outside [0, num_pdfs), num_units above 32767.
   A TRANSCRIPT is n >= 1 slots, slot k a unit u_k and a flag opt_k; transcript g owns the slots [slot_begin[g], slot_begin[g + 1]) of
   slot_unit and slot_optional (slot_begin[0] = 0).  Refused with TDNNF_EINVAL naming the transcript and the slot: a unit outside
   [0, num_units), two adjacent optional slots, a transcript without a mandatory slot.  Its graph:
     states   0 the start; then for every slot k in order A_k, whose left neighbour is slot k-1 (nothing for k = 0), and directly behind it
              B_k -- only in context 1, for k >= 1 and opt_k-1 -- whose left neighbour is slot k-2 (nothing for k = 1): slot k-1 was skipped.
              A state's pdfs are entry_pdf and loop_pdf at (unit of its left neighbour or -1, u_k).  S = 1 + n + #B.
     arcs     on every unit state a self-loop with its loop pdf and loop_logprob[u_k];
              into A_k from every state of slot k-1 with leave_logprob[u_k-1], from the start with 0 for k = 0, plus take_logprob if opt_k;
              where opt_k-1, k >= 1: from every state of slot k-2 with leave_logprob[u_k-2] + skip_logprob (from the start with
              skip_logprob for k = 1) into B_k in context 1, into A_k in context 0;
              an arc that enters a state carries the state's entry pdf.  Every weight is a float formed by at most one float addition.
              Ordered by (source, destination), no pair twice; every state of slot k has 1 + [k+1 < n] + [k+2 < n and opt_k+1] arcs, the
              start 1 + [n >= 2 and opt_0]; at most 3 arcs enter a state.
     initial  0 at state 0;  final  leave_logprob[u_n-1] on the states of slot n-1 and, if opt_n-1, leave_logprob[u_n-2] + skip_logprob on
              those of slot n-2;  -inf elsewhere.
     labels   (labelled handles) an arc's label is the slot of its destination: tdnnf_align_best_path_labels gives every frame's position
              in the transcript, and its run lengths are the segmentation.  num_labels must cover the longest transcript's slots.
   With context 0 and entry_pdf = loop_pdf this is the graph of one unit per entry with skips over the optional ones.
   tdnnf_transcript_graph_sizes is host-only: the states and arcs of every transcript (either out-pointer may be NULL), for sizing a
   reserve; it refuses what the assign refuses with the same messages under its own name.
   tdnnf_align_graphs_assign_transcripts is tdnnf_align_graphs_assign from transcripts: reserved handles only, of the unit set's num_pdfs
   (else TDNNF_EINVAL); it validates the slots and the three capacities (named with their excess as assign names them) and, for a labelled
   handle, num_labels before anything is written, so a refused call leaves the previous batch in place.  The host works in O(slots): from
   the closed forms it derives the begins, per graph the arcs and the largest in-degree, and the column lists, stages 4 bytes a slot where
   assign stages 28 bytes an arc, and enqueues on `stream` the copies, ONE kernel that writes the arcs, initial and final weights and labels
   (csrc/align_compile_kernels.h) and the three build kernels of tdnnf_align_graphs_assign, unchanged: the tables are the bytes an assign
   of the same graphs builds.  No allocation, no free, no device-wide or stream-wide wait; the one host wait there can be is for the
   staging copy of the assign before last.  Stream order, the host-side answers and tdnnf_align_graphs_capacity's `assigns` are
   tdnnf_align_graphs_assign's, and so is the failure rule (a refusal leaves the previous batch, an error of the runtime no batch); both
   kinds of assign may alternate on one handle, on the one pair of staging buffers.
   Pronunciation alternatives: "PRONUNCIATION GRAPHS" below.
   Not built: adjacent optional slots, lexicon and tree handling (the caller maps words to units and (left, unit) to pdfs), right context,
   units of several states, capture into a HIP graph. */
typedef struct tdnnf_unit_set tdnnf_unit_set;
int tdnnf_unit_set_create(int num_units, int num_pdfs, int context, const int *entry_pdf, const int *loop_pdf, const float *loop_logprob,
                          const float *leave_logprob, float take_logprob, float skip_logprob, tdnnf_unit_set **out);
void tdnnf_unit_set_destroy(tdnnf_unit_set *);
int tdnnf_transcript_graph_sizes(const tdnnf_unit_set *, int num_transcripts, const int *slot_begin, const int *slot_unit,
                                 const int *slot_optional, int *states_out, int *arcs_out);
int tdnnf_align_graphs_assign_transcripts(tdnnf_align_graphs *, const tdnnf_unit_set *, int num_transcripts, const int *slot_begin,
                                          const int *slot_unit, const int *slot_optional, tdnnf_stream stream);
/* PRONUNCIATION GRAPHS: transcript graphs whose positions (words) have several pronunciations, compiled on the device as the transcript
   graphs above are, with the unit set (context 0 or 1) as it is.
   A transcript is n >= 1 POSITIONS; position p has a flag opt_p and A_p >= 1 ALTERNATIVES; alternative (p, a) is L >= 1 units of the unit set
   and a float alt_logprob.  An ENTRY is one unit of one alternative; a transcript's entries are numbered from 0 in flat order: position,
   alternative, unit.  The flat arrays of a batch: transcript g owns the positions [pos_begin[g], pos_begin[g + 1]) of pos_optional;
   position P (counted over the batch) the alternatives [pos_alt_begin[P], pos_alt_begin[P + 1]) of alt_logprob; alternative Q the units
   [alt_unit_begin[Q], alt_unit_begin[Q + 1]) of alt_units.  All three begin arrays start at 0.
   The PREDECESSORS of position p: the near ones, the alternatives of p-1 in order (for p = 0 the start); then the far ones, only if
   opt_p-1, the alternatives of p-2 in order (for p = 1 the start).  The graph:
     states   0 the start; the entries follow in flat order.  An inner entry (j > 0) has one state; its left unit is the unit before it in
              its alternative.  A first entry (j = 0) has one state in context 0 and, in context 1, one state per predecessor in their
              order -- not merged even where two predecessors end in the same unit -- whose left unit is the predecessor's last unit, -1 for
              the start.  A state's pdfs are entry_pdf and loop_pdf at (left unit, unit).
     arcs     out of a state of entry (p, a, j) with unit u: a self-loop with the loop pdf and loop_logprob[u];
              if j + 1 < L one arc to the next entry's state with leave_logprob[u];
              if j = L - 1, for every alternative a' of p+1 an arc into the state of (p+1, a', 0) that belongs to predecessor (p, a) -- in
              context 0 its one state -- with leave_logprob[u], then + take_logprob if opt_p+1, then + alt_logprob(p+1, a') if A_p+1 >= 2;
              if j = L - 1, opt_p+1 and p + 2 < n, for every alternative a'' of p+2 an arc into its far state for (p, a), with
              leave_logprob[u] + skip_logprob, then + alt_logprob(p+2, a'') if A_p+2 >= 2.
              The start behaves as the last entry of a position -1 with no leave term: 0.0f + take_logprob or 0.0f into position 0,
              skip_logprob into position 1 over an optional position 0, then the alternative's term.
              An arc that enters a state carries that state's entry pdf.  Every weight is a float formed left to right in the order given.
              Ordered by (source, destination), no pair twice.  The arcs into a state are its loop and the states of its predecessor's last
              entry, so the in-degree is not bounded: 1 + N where that alternative has one unit and N states.
     initial  0 at state 0;  final  leave_logprob[u] on the states of the last entries of position n-1 and, if opt_n-1 and n >= 2,
              leave_logprob[u] + skip_logprob on those of position n-2;  -inf elsewhere.
     labels   (labelled handles) an arc's label is the entry number of its destination: tdnnf_align_best_path_labels gives per frame the
              position, the alternative chosen and the unit.  num_labels must cover the most entries of any transcript.
   A transcript whose every position has one alternative of one unit is the slot transcript above, and its tables are the bytes
   tdnnf_align_graphs_assign_transcripts builds.  The best path's units and the frames they start at go into
   tdnnf_supervision_assign_alignments unchanged, so the alignment supervision needs no alternatives.
   Refused with TDNNF_EINVAL naming the transcript, the position and the alternative: a position without an alternative, an empty alternative,
   a unit outside [0, num_units), an alt_logprob that is NaN or infinite, two adjacent optional positions, a transcript without a mandatory
   position; and the capacities and num_labels, in tdnnf_align_graphs_assign's words.  All of it before anything is written: a refusal
   leaves the previous batch in place.
   tdnnf_pronunciation_graph_sizes is host-only: the states and arcs of every transcript (either out-pointer may be NULL), for sizing a
   reserve; it gives the same refusals under its own name.
   tdnnf_align_graphs_assign_pronunciations is tdnnf_align_graphs_assign_transcripts from these arrays.  The host works in O(entries +
   first-entry states) (csrc/align_pronunciations.h): the begins, per graph the arcs and the largest in-degree, the column lists, and the
   first state of every position.  It stages 4 bytes an entry, 12 an alternative and 8 a position inside the staging the reserve made -- a
   batch within max_states and max_arcs fits, because arcs >= entries + alternatives and states >= entries; a batch that would not is refused
   by name -- and enqueues ONE kernel (csrc/align_pron_compile_kernels.h) in front of the three unchanged build kernels.  Stream order, the
   failure rule, `assigns` and the alternation with the other assigns on the one pair of staging buffers are
   tdnnf_align_graphs_assign_transcripts's; tdnnf_supervision_assign_e2e_pronunciations carries those of
   tdnnf_supervision_assign_e2e_transcripts.
   Not built: adjacent optional positions, right context, units of several states, capture into a HIP graph. */
int tdnnf_pronunciation_graph_sizes(const tdnnf_unit_set *, int num_transcripts, const int *pos_begin, const int *pos_optional,
                                    const int *pos_alt_begin, const float *alt_logprob, const int *alt_unit_begin, const int *alt_units,
                                    int *states_out, int *arcs_out);
int tdnnf_align_graphs_assign_pronunciations(tdnnf_align_graphs *, const tdnnf_unit_set *, int num_transcripts, const int *pos_begin,
                                             const int *pos_optional, const int *pos_alt_begin, const float *alt_logprob,
                                             const int *alt_unit_begin, const int *alt_units, tdnnf_stream stream);
int tdnnf_supervision_assign_e2e_pronunciations(tdnnf_supervision *, const tdnnf_unit_set *, int num_sequences, int frames_per_sequence,
                                                const int *pos_begin, const int *pos_optional, const int *pos_alt_begin,
                                                const float *alt_logprob, const int *alt_unit_begin, const int *alt_units, float weight,
                                                tdnnf_stream stream);
/* ALIGNMENT SUPERVISIONS: the next minibatch of a supervision of tdnnf_supervision_reserve compiled on the device from alignments and a
   frame tolerance -- the supervision regular LF-MMI trains on: an alignment whose unit boundaries may each move by +- tolerance frames.
   The caller hands over (unit, start frame) pairs and never builds a state or an arc array; the alignment may be this library's
   (tdnnf_align_graphs_assign_transcripts on a labelled handle, then the run lengths of tdnnf_align_best_path_labels).
   Sequence s owns the entries [unit_begin[s], unit_begin[s + 1]) of `units` and `starts` (unit_begin[0] = 0): n >= 1 units u_0 .. u_n-1
   of the unit set (context 0 or 1) that start at the OUTPUT frames b_0 = 0 < b_1 < ... < b_n-1 < T = frames_per_sequence; unit k covers
   the frames [b_k, b_k+1).  Refused with TDNNF_EINVAL naming the sequence and the unit's position: a sequence without a unit, a unit
   outside [0, num_units), b_0 != 0, a start that is not behind the one before it, a start >= T; and a negative tolerance.
   The lattice of one sequence, with tol = tolerance:
     windows  lo_k = max(b_k - tol, 0), hi_k = min(b_k + tol, T - 1); lo_0 = hi_0 = 0; tightened from the left, lo_k = max(lo_k, lo_k-1 + 1),
              and from the right against the virtual lo_n = hi_n = T, hi_k = min(hi_k, hi_k+1 - 1): every unit keeps a frame, and
              lo_k <= b_k <= hi_k, so the alignment itself is always a path.  Unit k may be entered at any frame of [lo_k, hi_k].
     states   the start, at time 0; E(t, k) for t in [lo_k + 1, hi_k + 1]: unit k was entered at frame t - 1; L(t, k) for t in
              [lo_k + 2, hi_k+1]: frame t - 1 was a later frame of unit k.  Ordered by time, within one time all E by k, then all L by k.
     arcs     start -> E(1, 0) with the entry pdf at (-1, u_0).  From X(t, k), X either kind: the enter arc to E(t + 1, k + 1) with the entry
              pdf at (u_k, u_k+1), if k + 1 < n and lo_k+1 <= t <= hi_k+1; the stay arc to L(t + 1, k) with the loop pdf at
              (u_k-1 or -1, u_k), if t + 1 <= hi_k+1.  (Context 0 reads both tables at the unit alone.)  Ordered by (source, destination);
              a state has 0, 1 or 2.  Every arc_logprob is 0.
     final    0 on the time-T states of unit n - 1, -inf elsewhere.
   This is Kaldi's supervision FST, which is unweighted: the unit set's loop_logprob, leave_logprob, take_logprob and skip_logprob are NOT
   used here.  tolerance 0 gives the one path of the alignment (T + 1 states); a tolerance >= T lets every boundary go anywhere.
   tdnnf_alignment_supervision_sizes is host-only: the states and arcs of every sequence's lattice (either out-pointer may be NULL), for
   sizing a reserve; it refuses what the assign refuses with the same messages under its own name.
   tdnnf_supervision_assign_alignments is tdnnf_supervision_assign from alignments: supervisions of tdnnf_supervision_reserve only (an
   end-to-end or a created supervision is refused, TDNNF_EINVAL).  The host works in O(units + sequences * (frames + 2)): the windows, and
   from the closed form of a frame (csrc/chain_sup_alignment.h) the begins, frame_state_begin, the counts, the widths and `wide` -- what
   tdnnf_supervision_assign finds on the lattice's arrays -- then the four capacities, named with their excess as assign names them, all
   before anything is written: a refused call leaves the previous minibatch.  It stages 12 bytes a unit where assign stages 16 bytes an arc
   and 8 a state, inside the staging tdnnf_supervision_reserve made, and enqueues on `stream` the copies, ONE kernel that writes state_time,
   final_logprob and the arcs (csrc/chain_sup_compile_kernels.h) and the two build kernels of tdnnf_supervision_assign, unchanged: the
   tables are the bytes an assign of the lattice's arrays builds, and the objective's bits with them.  No allocation, no free, no
   device-wide or stream-wide wait; the one host wait there can be is for the staging copy of the assign before last.  Stream order,
   tdnnf_supervision_capacity's `assigns` and the failure rule are tdnnf_supervision_assign's (a refusal leaves the previous minibatch, an
   error of the runtime none); both kinds of assign may alternate on one handle, on the one pair of staging buffers.
   Not built: alternative unit sequences (pronunciations), frame-subsampling of a frame-rate alignment (the starts are output frames),
   composition with a normalisation FST (the lattice's paths are not restricted to the denominator graph's), capture into a HIP graph,
   input that stays on the device (the alignment comes from host arrays). */
int tdnnf_alignment_supervision_sizes(const tdnnf_unit_set *, int num_sequences, int frames_per_sequence, const int *unit_begin, const int *units,
                                      const int *starts, int tolerance, int *states_out, int *arcs_out);
int tdnnf_supervision_assign_alignments(tdnnf_supervision *, const tdnnf_unit_set *, int num_sequences, int frames_per_sequence,
                                        const int *unit_begin, const int *units, const int *starts, int tolerance, float weight,
                                        tdnnf_stream stream);
/* ALIGNMENT CHUNKS: the supervision of a fixed-length chunk cut out of an utterance, compiled on the device from the alignment of the
   WHOLE utterance -- what regular LF-MMI trains on (chunks of 150 output frames in the recipes).  A chunk may begin and end in the middle of
   a unit, and boundaries that lie outside it may still be moved into it by the tolerance; Kaldi's SupervisionSplitter::GetFrameRange,
   before its determinisation.
   Sequence s is given by the alignment of its utterance -- the entries [unit_begin[s], unit_begin[s + 1]) of `units` and `starts`, exactly
   what "ALIGNMENT SUPERVISIONS" takes with T replaced by utt_frames[s]: n >= 1 units, b_0 = 0 < b_1 < ... < utt_frames[s] -- and by
   chunk_begin[s] = o with 0 <= o and o + T <= utt_frames[s], T = frames_per_sequence common to the minibatch.  Two chunks of one utterance
   are two sequences that repeat its alignment.  Refused with TDNNF_EINVAL naming the sequence: everything "ALIGNMENT SUPERVISIONS"
   refuses, utt_frames[s] < 1, chunk_begin[s] < 0, chunk_begin[s] + T > utt_frames[s].
   Let U be the utterance's lattice as defined above: the windows from `tolerance`, tightened over the whole utterance, states E(t, k) and
   L(t, k).  The chunk's lattice:
     states   a new start at time 0, then every state of U with time t in [o + 1, o + T], in U's order (time, then all E by unit, then all L
              by unit), re-timed to t - o.
     arcs     every arc of U between two kept states, unchanged; and out of the start one arc to every kept state of time o + 1, in state
              order, with the pdf that all arcs into that state carry in U: for E(o + 1, k) the entry pdf at (u_k-1 or -1, u_k), for
              L(o + 1, k) the loop pdf at (u_k-1 or -1, u_k).  (Context 0 reads both tables at the unit alone.)  For o = 0 this is the one arc
              into E(1, 0).  Every arc_logprob is 0; ordered by (source, destination).
     final    0 on every state of time o + T, -inf elsewhere; for o + T = utt_frames[s] these are the states of unit n - 1 only.
   o = 0 and T = utt_frames[s] give U itself, and the bytes tdnnf_supervision_assign_alignments builds.  The accepting paths of a chunk are
   exactly the restrictions to [o, o + T) of U's accepting paths (every state of U lies on one, so nothing has to be trimmed).
   tdnnf_alignment_chunk_supervision_sizes is host-only: the states and arcs of every chunk's lattice (either out-pointer may be NULL), for
   sizing a reserve; it refuses what the assign refuses with the same messages under its own name.
   tdnnf_supervision_assign_alignment_chunks is tdnnf_supervision_assign_alignments from chunks: supervisions of tdnnf_supervision_reserve
   only.  The host works in O(units of the utterances + sequences * (frames + 2)): the utterance's windows, the frames o + 1 .. o + T from the
   same closed form (csrc/chain_sup_alignment.h), and from them the begins, frame_state_begin, the counts, the widths and `wide`; then the
   four capacities, named with their excess as assign names them.  It stages, per sequence, only the units the chunk's frames can name and
   their neighbours (12 bytes each) and 16 bytes of scalars.  The reserve's sizes stay as they are, and short chunks can need more staging
   than it made for 8 bytes a state and 16 an arc (a one-frame chunk has 2 states, 1 arc and up to 3 staged units): such a minibatch is
   refused, TDNNF_EINVAL naming the shortfall in bytes.  All of it before anything is written: a refused call leaves the previous
   minibatch.  Then the copies, the ONE compile kernel of tdnnf_supervision_assign_alignments (csrc/chain_sup_compile_kernels.h: a whole
   alignment is its chunk o = 0) and the two unchanged build kernels on `stream`.  No allocation, no free, no device-wide or stream-wide
   wait; stream order, tdnnf_supervision_capacity's `assigns` and the failure rule are tdnnf_supervision_assign's (a refusal leaves the
   previous minibatch, an error of the runtime none), and all three kinds of assign may alternate on one handle.
   Not built: frame-subsampling of a frame-rate alignment, chunks shorter than T at an utterance's end, sharing one utterance's units
   between sequences, determinisation, composition with a normalisation FST, capture into a HIP graph. */
int tdnnf_alignment_chunk_supervision_sizes(const tdnnf_unit_set *, int num_sequences, int frames_per_sequence, const int *unit_begin,
                                            const int *units, const int *starts, const int *utt_frames, const int *chunk_begin, int tolerance,
                                            int *states_out, int *arcs_out);
int tdnnf_supervision_assign_alignment_chunks(tdnnf_supervision *, const tdnnf_unit_set *, int num_sequences, int frames_per_sequence,
                                              const int *unit_begin, const int *units, const int *starts, const int *utt_frames,
                                              const int *chunk_begin, int tolerance, float weight, tdnnf_stream stream);
/* diagnostics (tests): a copy-out of the device arrays of a created or an assigned handle, as ints, after waiting for the stream of the last
   assign.  table 0 by destination, 1 by source, 2 by pdf, 3 by label (labelled handles): which 0 the slots, 1 the heavy-row descriptors,
   2 the arc entries, 4 ints each.  table 4: which 0 the graph descriptors (14 ints a graph), 1 the by-label ranges (4 ints a graph), 2 the
   lengths of the pdf column lists and the lists, 3 the same for labels, 4 / 5 the bits of initial_logprob / final_logprob, 6 the labels.
   *count: the ints of the answer; out may be NULL to ask for it, else capacity (ints) must cover it. */
int tdnnf_align_graphs_dump(const tdnnf_align_graphs *, int table, int which, int *out, long long capacity, long long *count);
/* states, arcs and largest in-degree of one graph; any out-pointer may be NULL */
int tdnnf_align_graphs_info(const tdnnf_align_graphs *, int graph, int *num_states, int *num_arcs, int *max_in_degree);
/* utt_graph[u] (host) names the graph of utterance u -- many utterances may share one; NULL: graph 0 if there is one graph, else graph u
   (then num_utts must be num_graphs).  utt_frames[u] >= 0.  With S_u the states of utterance u's graph:
     bytes = 16 + roundup(32 * num_utts, 256) + 4 * sum_u roundup(utt_frames[u] * S_u, 2)  [+ 16 * sum_u S_u in the workspace form]
   (alignment slack; the per-utterance table; one back-pointer per (frame, state); the two state vectors).  0 for bad arguments.
   Under option "align_path_checkpoint" with the interval C, K_u = ceil(utt_frames[u] / C) (0 for no frames) and B_u = min(C, utt_frames[u]):
     bytes = 16 + roundup(32 * num_utts, 256) + sum_u [ 8 * K_u * S_u + 4 * roundup(B_u * S_u, 2) + 4 * roundup(utt_frames[u], 2) ]
                                              [+ 16 * sum_u S_u in the workspace form]
   (the checkpoints; the segment buffer; the path) -- 20 000 frames on 3 001 states at -1 (C = 142): 5.2 MB against 240 MB; 128 x 500 frames
   on 4 000 states at -1 (C = 23): 137 MB against 1 GB.  0 for an option below -1 as well. */
size_t tdnnf_align_workspace_bytes(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames);
/* Frame t of utterance u is row utt_row_begin[u] + t * row_stride of nnet_output (which may be a sub-matrix view): row_stride 1 reads the
   concatenated utterances tdnnf_infer_compute writes, row_stride B a t-major minibatch of B sequences (utt_row_begin[u] = u).
   pdf_out_dev: sum(utt_frames) ints, utterance after utterance.  state_out_dev (may be NULL): the path's states, local to the graph,
   utt_frames[u] + 1 per utterance, utterance after utterance.  results_dev: two doubles per utterance, the score and the ok flag
   (1.0 / 0.0).  Everything runs on the caller's stream and nothing waits for the device (the per-utterance table goes to the workspace
   by hipMemcpyAsync from pageable memory).  TDNNF_EINVAL: a workspace smaller than tdnnf_align_workspace_bytes, a row outside the
   matrix, fewer columns than num_pdfs. */
int tdnnf_align_best_path(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                          int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, int *pdf_out_dev, int *state_out_dev,
                          double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream);

/* The best path with the identity of its arcs.  pdf_out_dev, state_out_dev, results_dev and the workspace (tdnnf_align_workspace_bytes) are
   tdnnf_align_best_path's, which runs unchanged; behind it on the same stream a second kernel reads the chosen arc of every frame from
   where the trace-back left it and writes, laid out as pdf_out_dev (sum(utt_frames) ints each, utterance after utterance):
     arc_out_dev[t]    (may be NULL) the caller's index of the arc taken at frame t -- the index into the arrays given at creation, global
                       over the graphs (subtract graph_arc_begin[g] for the index within graph g);
     label_out_dev[t]  arc_label of that arc.
   Both are -1 for every frame of an utterance with ok = 0.  Ties are the best path's: of two parallel arcs that differ only in their label
   the first in the caller's list is reported.  Every element of both outputs is written, by one thread each.  Under option
   "align_path_checkpoint" the second kernel reads the path the checkpointed trace-back left: the same outputs.  TDNNF_EINVAL: as
   tdnnf_align_best_path, a handle without labels, a null label_out_dev. */
int tdnnf_align_best_path_labels(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                                 int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, int *pdf_out_dev, int *state_out_dev,
                                 int *label_out_dev, int *arc_out_dev /* may be NULL */, double *results_dev, void *workspace_dev,
                                 size_t workspace_bytes, tdnnf_stream);

/* ------------------------------------------------------------------ A7, forward-backward
 * The summing counterpart of the best path on the same graphs (a tdnnf_align_graphs holds its arcs three times: by destination, by source,
 * by pdf): the total log-likelihood of each utterance through its graph and, on request, the per-frame pdf posteriors -- the score of a
 * transcript graph to set against the free path, soft alignments (what ali-to-post and its relatives consume).  It is also the arithmetic of
 * the numerator of flat-start ("end-to-end") LF-MMI; to TRAIN on such graphs use tdnnf_supervision_create_e2e above, whose kernels run the
 * same recursion beside the denominator and add the posteriors into the chain derivative.  No beam, epsilon-free graphs, as above; per pdf
 * here, per caller-defined label (a transition-id, a phone) under "label posteriors" below.  All in double; term is the best path's:
 *
 *   term(arc, t)   = (double)arc_logprob + (double)acoustic_scale * (double)y[t, arc_pdf]
 *   alpha_0[s]     = (double)initial_logprob[s]
 *   alpha_t+1[d]   = LSE over arcs into d   of  alpha_t[src] + term(arc, t)
 *   logprob        = LSE over s             of  alpha_T[s] + (double)final_logprob[s]
 *   beta_T[s]      = (double)final_logprob[s]
 *   beta_t[s]      = LSE over arcs out of s of  term(arc, t) + beta_t+1[dst]
 *   gamma[t, p]    = sum over arcs with pdf p of exp(alpha_t[src] + term(arc, t) + beta_t+1[dst] - logprob)
 *   post[t, p]     = (float)(weight * gamma[t, p])          for every p in [0, num_pdfs)
 *
 * LSE(v_1..v_n) = m + log(sum exp(v_i - m)) with m the greatest candidate; an empty or all -inf set gives -inf.  As for the best path a
 * candidate counts only if it compares greater than -inf: a NaN or -inf one contributes nothing and a NaN never enters a state vector.
 * No clamp on y.  ok = 1 iff logprob is finite (+inf in y can make it +inf, which is reported as it is); with ok = 0 every post element
 * of that utterance's rows is 0, the other utterances of the call are unaffected.  A zero-frame utterance has logprob = LSE(init + final)
 * and writes no row.  The order of a sum is the library's, so results are held to a tolerance (tests/test_gpu_posteriors.py), but it is
 * fixed: every (t, p) element has one owner, there are no atomics, and two calls on the same inputs give the same bits, in either form.
 *
 * One workgroup per utterance with the best path's thread counts and option "align_form" for where the two state vectors live (read by
 * both functions below: set it before both).  Where they fit, a third vector (alpha_t) and two output rows are staged in LDS beside
 * them; otherwise those gathers read global memory.  Same results either way.
 *
 * Alpha checkpointing (option "align_checkpoint", default 0 = off; read by the workspace question and by the calls: set it before both).
 * With posteriors the forward pass keeps alpha_t of every frame, 8 * (T + 1) * S bytes an utterance.  With an interval C >= 1 (or -1: one C
 * for the call, ceil(sqrt(its longest utterance's frames)), at least 1; a C above the longest utterance counts as that length) it keeps
 * alpha_kC only -- one CHECKPOINT per segment [kC, min(kC + C, T)) -- and the backward pass, segment by segment from the last, first
 * recomputes alpha_kC+1 .. of the segment from its checkpoint into a buffer of min(C, T) - 1 vectors, then walks the segment's frames.  The
 * recomputation is the forward pass's own step in its own order: every output, logprob and ok flag has the bits it has with the option
 * off, in every form (tests/test_gpu_posteriors_checkpoint.py).  Vectors of alpha per utterance of T frames:
 *     V(T, C) = ceil(T / C) + min(C, T) - 1   for T >= 1,   V(0, C) = 1,   V(T, 0) = T + 1;      V(T, C) <= T for C >= 1, T >= 1
 * -- 500 frames: 501 vectors off, 44 at C = 23 (automatic); 20 000 frames: 20 001 off, 282 at C = 142.  The cost is one more sweep over the
 * arcs by destination for every frame that is not a checkpoint (about 4 sweeps with an exp per arc where there are 3).  The option does not
 * touch the call without a posterior matrix, the best path or the end-to-end numerator. */
/* With S_u the states of utterance u's graph and V the vectors of alpha above (V = utt_frames[u] + 1 unless option "align_checkpoint" is set):
     bytes = 16 + roundup(32 * num_utts, 256)  [+ 8 * sum_u V(utt_frames[u], C) * S_u with want_posteriors]
                                               [+ 16 * sum_u S_u in the workspace form]
   (alignment slack; the per-utterance table; alpha; the two state vectors).  With every frame kept the alpha region is twice the best
   path's back-pointers: about 2 GB for 128 x 500 frames on 4 000 states, 180 MB at C = 23.  0 for bad arguments, an
   "align_checkpoint" below -1 with want_posteriors among them. */
size_t tdnnf_align_posteriors_workspace_bytes(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames,
                                              int want_posteriors);
/* utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, acoustic_scale as for tdnnf_align_best_path.  results_dev: two doubles per
   utterance, logprob and the ok flag (1.0 / 0.0).  post_out (may be NULL) is addressed like nnet_output -- row utt_row_begin[u] + t *
   row_stride; it may be a sub-matrix view and may have more than num_pdfs columns: columns [0, num_pdfs) of each of the call's frame rows
   are OVERWRITTEN (zeros for the pdfs no arc names), nothing else of it is touched.  post_out == NULL (workspace: want_posteriors = 0):
   only the forward recursion runs, on its two alternating vectors, and keeps no alpha per frame.  Everything runs on the caller's stream
   and nothing waits for the device.  TDNNF_EINVAL: as for tdnnf_align_best_path (a workspace smaller than
   tdnnf_align_posteriors_workspace_bytes, a row outside the matrix, fewer columns than num_pdfs), and a post_out with fewer than num_pdfs
   columns or without one of the call's rows. */
int tdnnf_align_posteriors(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                           int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight, tdnnf_mat *post_out /* may be NULL */,
                           double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream);

/* ---- compact posteriors: the same pass writing only the columns a graph can fill.
 * A transcript graph names a few hundred of the num_pdfs pdfs, and what consumes posteriors (a Posterior archive, soft targets) wants
 * (pdf, value) pairs.  The COLUMN LIST of a graph is the ascending list of the distinct pdfs its arcs name, D_g of them
 * (tdnnf_align_graphs_pdfs); the compact output of an utterance on graph g is frames x D_g floats, element [t, k] = post[t, pdfs_g[k]] of the
 * dense call above -- the same arithmetic in the same order by the same owner, so the same bits -- and every pdf outside the list has
 * posterior 0 by construction.  Every element of a block has an owner, so nothing is zeroed first and nothing outside the blocks is
 * touched.  ok = 0: the utterance's whole block is 0.  The layout is a function of (utt_graph, utt_frames) alone. */
/* distinct pdfs of one graph, ascending; pdfs_out (host, may be NULL) gets *num of them */
int tdnnf_align_graphs_pdfs(const tdnnf_align_graphs *, int graph, int *num, int *pdfs_out);
/* layout of a call's compact output: utterance u owns floats [utt_begin[u], utt_begin[u + 1]),
   frames[u] rows of D_graph(u) floats, row t then column k.  utt_begin_out (host, num_utts + 1,
   may be NULL); *elems_out = utt_begin[num_utts] (may be 0 for a call of zero-frame utterances) */
int tdnnf_align_posteriors_compact_layout(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames, long long *elems_out,
                                          long long *utt_begin_out);
/* as tdnnf_align_posteriors with a posterior matrix, but writing the compact layout.  Workspace:
   tdnnf_align_posteriors_workspace_bytes(..., want_posteriors = 1), unchanged.
   TDNNF_EINVAL as there, plus: null post_compact_dev with elems > 0, post_compact_elems smaller than the layout's, and a call in which an
   utterance's block starts beyond float 2^31 - 1 of the output (8 GiB: split the call).  Everything runs on the caller's stream, nothing
   waits for the device; options "align_form" and "align_checkpoint" are read as by the dense call. */
int tdnnf_align_posteriors_compact(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                                   int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight, float *post_compact_dev,
                                   size_t post_compact_elems, double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream);

/* ---- sparse posteriors: per frame the at most K (pdf, value) pairs above a floor.
 * What a Posterior archive, soft targets and data clean-up take: of the D_g floats of a frame a handful carry mass.  The compact pass above
 * runs into a block of the workspace (the caller never sees it) and a selection pass (csrc/align_sparse_kernels.h) reads it; everything below
 * is a function of the floats the compact call writes, v[k] = compact[t, k] for frame t of utterance u on graph g, with its column list pdfs_g:
 *   candidates  the columns with v[k] > min_post -- strict; min_post is finite and >= 0, so a zero, a negative value and a NaN never are;
 *               n of them;
 *   kept        all candidates if n <= K = max_per_frame (1 <= K <= 64), else the K of greatest value, among equal values the lower pdf;
 *   written     in ascending pdf order: frame f = frame_begin[u] + t, frame_begin the exclusive prefix sum of utt_frames (whatever
 *               utt_row_begin and row_stride are), owns slots [f * K, (f + 1) * K) of pdf_out_dev and post_out_dev; count_out_dev[f] =
 *               min(n, K); slots [0, count) hold the kept pairs (pdfs_g[k], v[k]) -- the compact call's bits, NOT renormalised -- and slots
 *               [count, K) hold (-1, 0.f).  Every slot and count of the call is written, nothing is zeroed first, nothing else is touched.
 * ok = 0: every count of the utterance 0, every slot (-1, 0.f).  results_dev: FOUR doubles per utterance -- logprob and ok as above, the
 * number of its frames with n > K (truncated frames) and the greatest n over its frames (the K a retry needs), both exact integers.
 * No atomics, one owner per slot: two calls on the same inputs give the same bits. */
/* With W = tdnnf_align_posteriors_workspace_bytes(..., want_posteriors = 1) and elems that of tdnnf_align_posteriors_compact_layout:
     bytes = 16 + roundup(W, 16) + 48 * num_utts + 8 * sum_u ceil(utt_frames[u] / 16) + 4 * elems
   (alignment slack; the compact call's workspace; its results and the selection's table, 16 + 32 bytes an utterance; the selection's
   (truncated frames, greatest n) per 16 frames; the compact block).  0 for bad arguments, max_per_frame outside [1, 64] among them. */
size_t tdnnf_align_posteriors_sparse_workspace_bytes(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames,
                                                     int max_per_frame);
/* utt_graph .. weight as for tdnnf_align_posteriors_compact.  pdf_out_dev, post_out_dev: sum(utt_frames) * max_per_frame elements each,
   count_out_dev: sum(utt_frames) ints (all three may be NULL for a call of zero-frame utterances, which writes results only).
   TDNNF_EINVAL, with a message and nothing launched: all that tdnnf_align_posteriors_compact refuses (its limit of 8 GiB to the start of an
   utterance's block included), max_per_frame outside [1, 64], min_post negative or not finite, a null output with frames to write, a
   workspace smaller than tdnnf_align_posteriors_sparse_workspace_bytes.  Everything runs on the caller's stream, nothing waits for the
   device; options "align_form" and "align_checkpoint" are read as by the dense call (and by the workspace question above, through W). */
int tdnnf_align_posteriors_sparse(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                                  int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight, float min_post, int max_per_frame,
                                  int *pdf_out_dev, float *post_out_dev, int *count_out_dev, double *results_dev, void *workspace_dev,
                                  size_t workspace_bytes, tdnnf_stream);

/* ---- label posteriors: the compact and the sparse form per caller-defined label instead of per pdf.
 * For a handle of tdnnf_align_graphs_create_labelled.  The LABEL COLUMN LIST of a graph is the ascending list of the distinct labels its arcs
 * carry, L_g of them (tdnnf_align_graphs_labels); an utterance on graph g gets frames x L_g floats,
 *   element [t, k] = (float)(weight * sum over the arcs with label labels_g[k], in the caller's order, of
 *                            exp(alpha_t[src] + term(arc, t) + beta_t+1[dst] - logprob))
 * with alpha, beta, term (its y is that of the ARC's pdf) and logprob those of tdnnf_align_posteriors, formed in the compact call's
 * association by the same walk on a fourth arc table, by label: with arc_label = arc_pdf the output is tdnnf_align_posteriors_compact's bit
 * for bit.  One owner per (t, label), no zeroing pass, no atomics: two calls give the same bits.  ok = 0: the utterance's block is 0.
 * Summed over the labels that share a pdf the values are the pdf posteriors up to rounding; the sum of a row is weight as there.
 * No dense num_labels-wide form. */
/* distinct labels of one graph, ascending; labels_out (host, may be NULL) gets *num of them.  TDNNF_EINVAL for a handle without labels */
int tdnnf_align_graphs_labels(const tdnnf_align_graphs *, int graph, int *num, int *labels_out);
/* as tdnnf_align_posteriors_compact_layout with L_graph(u) for D_graph(u) */
int tdnnf_align_label_posteriors_compact_layout(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames,
                                                long long *elems_out, long long *utt_begin_out);
/* as tdnnf_align_posteriors_compact on the label layout.  Workspace: tdnnf_align_posteriors_workspace_bytes(..., want_posteriors = 1),
   unchanged.  TDNNF_EINVAL as there (the 8 GiB limit to the start of an utterance's block included), and a handle without labels. */
int tdnnf_align_label_posteriors_compact(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames,
                                         const int *utt_row_begin, int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight,
                                         float *post_compact_dev, size_t post_compact_elems, double *results_dev, void *workspace_dev,
                                         size_t workspace_bytes, tdnnf_stream);
/* the formula of tdnnf_align_posteriors_sparse_workspace_bytes with elems that of tdnnf_align_label_posteriors_compact_layout.  0 for bad
   arguments, a handle without labels and max_per_frame outside [1, 64] among them. */
size_t tdnnf_align_label_posteriors_sparse_workspace_bytes(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames,
                                                           int max_per_frame);
/* tdnnf_align_posteriors_sparse over the label block and the label column list: semantics, layout and the four result doubles are those of
   "sparse posteriors" above with labels_g for pdfs_g ("the lower pdf" reads "the lower label"); label_out_dev takes the place of
   pdf_out_dev.  The selection kernels are the same. */
int tdnnf_align_label_posteriors_sparse(const tdnnf_align_graphs *, int num_utts, const int *utt_graph, const int *utt_frames,
                                        const int *utt_row_begin, int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight,
                                        float min_post, int max_per_frame, int *label_out_dev, float *post_out_dev, int *count_out_dev,
                                        double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream);

/* ========================================================================== A8
 * OnlineNaturalGradient::PreconditionDirections (UPSTREAM; call sites
 * src/nnet3/nnet-tdnn-component.cc:598-599, nnet-simple-component.cc:3001-3002). */
int tdnnf_ng_create(int rank, int update_period, float num_samples_history, float alpha, tdnnf_ng **out);
void tdnnf_ng_destroy(tdnnf_ng *);
/* OnlineNaturalGradient::Freeze (UpdatableComponent::FreezeNaturalGradient, nnet-tdnn-component.cc:979-982): freeze != 0 keeps the
   current low-rank state (no refresh steps) */
int tdnnf_ng_freeze(tdnnf_ng *, int freeze);
/* X is modified in place; *scale_host (may be NULL) receives the scalar, which costs a stream synchronisation.
   The R x R eigen-problem of a refresh step is solved on a host worker thread and W_{t+1} is installed at the
   next call on the same object, so a call with scale_host == NULL never blocks.  rank <= 128. */
int tdnnf_ng_precondition(tdnnf_ng *, tdnnf_mat *X, float *scale_host, tdnnf_stream);
/* The N-sized statistics pass of one PreconditionDirections call by itself (what X W_t^T costs; tests, micro-benchmarks):
   H (N x rank, ld = H->stride) = X~ WT, row m of X~ = the concatenation over the taps of eff[i] * X[m * ix->row_stride + ix->row_offsets[i]]
   (Di columns each; eff_dev NULL = ones) [+ bias_dev: the row of W_t^T that meets the appended column of ones]; WT_dev is W_t^T, (taps * Di) x
   rank, k-major, followed by at least 64 finite rows; sumsq_dev (NULL or sumsq_cap doubles): their sum = ||X~||_F^2.  use_valu != 0: the
   form: 0 the MFMA rows GEMM, one tap after the other (needs W_dev = W_t, rank x ldw); 1 the vector-ALU kernel (csrc/ng_valu.hip; rank 20 / 40 / 80,
   TDNNF_EINVAL otherwise); 2 the one-pass form for taps that are row shifts of one matrix (csrc/ng_stats.hip ng_pform_pass: P = X [W_0^T | W_1^T ..], then
   H[m] = sum_i P[m + o_i][block i]; taps whole 128-row tiles apart, N % 128 == 0, N >= 32768, taps x rank <= 64, H dense; needs W_dev and
   workspace_dev of tdnnf_ng_stats_pass_workspace_bytes()). */
size_t tdnnf_ng_stats_pass_workspace_bytes(int rank, int Di, int num_taps, int N);
int tdnnf_ng_stats_pass(const tdnnf_tdnn_indexes *ix, const tdnnf_mat *X, int Di, const float *eff_dev, const float *WT_dev,
                        const float *W_dev, int ldw, const float *bias_dev, tdnnf_mat *H, double *sumsq_dev, int sumsq_cap, int form,
                        void *workspace_dev, size_t workspace_bytes, tdnnf_stream);
/* device float holding the scale of the object's last tdnnf_ng_precondition call (NULL before the first call) */
const float *tdnnf_ng_scale_dev(const tdnnf_ng *);

/* ========================================================================== A9
 * src/nnet3/nnet-utils.cc */
/* ConstrainOrthonormalInternal :914-1032 on M (rows <= cols; pass the transpose otherwise, :1068-1075).
   workspace: (rows*rows + rows*cols + 8) floats. */
size_t tdnnf_constrain_orthonormal_workspace_bytes(int rows, int cols);
int tdnnf_constrain_orthonormal(float scale, float *M_dev, int rows, int cols, int ld, void *workspace_dev,
                                size_t workspace_bytes, tdnnf_stream);
/* ApplyL2Regularization :2223-2245 : delta += scale * params */
int tdnnf_axpy(const float *x_dev, float a, float *y_dev, size_t n, tdnnf_stream);
/* UpdatableComponent::DotProduct (nnet-tdnn-component.cc:949-958): <x, y> accumulated in double, result on the HOST -- synchronises the
   stream (model averaging / diagnostics, not the training step) */
int tdnnf_dot(const float *x_dev, const float *y_dev, size_t n, double *result_host, tdnnf_stream);
/* UpdateNnetWithMaxChange :2085-2175 on a flat parameter vector partitioned into num_comp components
   (comp_begin_host[num_comp+1] element offsets).  params += factor_i * delta_i with the per-component and
   global max-change factors computed ON DEVICE (no D2H of the dot products).  delta is zeroed afterwards
   when zero_delta != 0 (momentum 0).  info_dev (may be NULL): [num_comp] factors then [1] ok flag. */
size_t tdnnf_max_change_workspace_bytes(int num_comp);
int tdnnf_update_with_max_change(float *params_dev, float *delta_dev, int num_comp, const long long *comp_begin_host,
                                 const float *max_change_host, float max_param_change, float max_change_scale,
                                 float scale, int zero_delta, void *workspace_dev, size_t workspace_bytes,
                                 float *info_dev, tdnnf_stream);

/* ====================================================================== descriptors
 * Row plumbing the nnet3 compiler does with kCopyRows commands for the graphs of SURVEY.md 3.4. */
/* lda input Append(-1,0,1,ReplaceIndex(ivector,t,0)) (run_tdnn_fbk_40_iv_sp_7q.sh:164): out row (k,b) =
   [feats(k + j, b) for j in 0..num_splice-1, ivector(b)]; feats is t-major with num_seq sequences and
   out->rows/num_seq + num_splice - 1 time steps. */
int tdnnf_splice_input(const tdnnf_mat *feats, const tdnnf_mat *ivectors, int num_seq, int num_splice,
                       tdnnf_mat *out, tdnnf_stream);
/* Convert between plain t-major rows (row = tau*B + b) and the row order a Tdnn component with
   row_stride rho > 1 expects on its input (row = (tau/rho)*rho*B + b*rho + tau%rho,
   nnet-tdnn-component.cc:897-902).  to_rho != 0: t-major -> rho order; else the inverse. */
int tdnnf_reorder_rows(const tdnnf_mat *in, int num_seq, int rho, int to_rho, tdnnf_mat *out, tdnnf_stream);

/* ===================================================================== chain trainer
 * One minibatch of nnet3-chain-train (UPSTREAM NnetChainTrainer::TrainInternal; the shipped pieces are
 * ApplyL2Regularization, UpdateNnetWithMaxChange, ConstrainOrthonormal in src/nnet3/nnet-utils.cc) for the
 * TDNN-F graphs of local/chain_NAS/run_tdnn_fbk_40_iv_sp_7q.sh:160-186 / run_tdnn_7q_fbk_40_manual.sh:138-151:
 * lda -> tdnn1 -> num_layers x tdnnf-layer -> prefinal-l -> {prefinal-chain -> output, prefinal-xent -> output-xent}.
 * Parameters and raw gradients live in two caller-owned flat device buffers (so a data-parallel caller can
 * all-reduce the gradient buffer between tdnnf_net_forward_backward and tdnnf_net_update). */
#define TDNNF_NET_MAX_LAYERS 32
typedef struct {
  int feat_dim, ivector_dim, num_pdfs;       /* 40, 100, 6034 */
  int hidden_dim, prefinal_small_dim;        /* 1536, 256 */
  int num_layers;                            /* tdnnf layers (14 for 7q) */
  int bottleneck_dim[TDNNF_NET_MAX_LAYERS];  /* 160 */
  int time_stride[TDNNF_NET_MAX_LAYERS];     /* 1,1,1,0,3 x 10 */
  float bypass_scale;                        /* 0.66 */
  int frames_per_chunk, num_sequences;       /* T (multiple of frame_subsampling), B */
  int frame_subsampling;                     /* 3 */
  float leaky_hmm, xent_regularize, chain_l2_regularize; /* 0.1, 0.1, 0.0 */
  float l2_hidden, l2_output;                /* 0.01, 0.002 (per-component l2-regularize) */
  float max_change_hidden, max_change_output, max_param_change; /* 0.75, 1.5, 2.0 */
  float relu_self_repair_scale;              /* 1e-5 */
  float batchnorm_stats_scale;               /* 0.8 (ScaleBatchnormStats, UPSTREAM trainer default) */
  /* DARTS offset-search supernet (run_TDNN_DARTSV3_fbk_stride_pretrain.sh:143-156 + scripts/generate_config.py:8-43):
     darts_num_offsets = K >= 2 turns every tdnnf layer's .linear / .affine into TdnnDARTSV3Components with offsets
     -(K-1)..0 / 0..K-1 (time_stride is then ignored), bias forced on, K architecture logits in front of the bias.
     darts_flags: TDNNF_DARTS_*; the pretrain recipe is TDNNF_DARTS_UNIFORM_SAMPLE (:124). 0 = plain TDNN-F. */
  int darts_num_offsets;
  int darts_flags;
  float darts_temp_proportion;
  /* != 0: weight gradients go through OnlineNaturalGradient exactly as UpdateNaturalGradient does
     (nnet-tdnn-component.cc:592-624, nnet-simple-component.cc:2980-3024): spliced input [c_i X_i ..., 1] and the
     output derivative are preconditioned (rank 20 / 80, alpha 4, history 2000, update period 4), the product of the
     two scale factors multiplies the update.  0: raw gradients (is_gradient_ / UpdateSimple semantics). */
  int use_natural_gradient;
  /* Bottleneck-dimension search supernet (run_TDNNf_DARTS_mod_fbk_bottleneckCBshare_95onehottrain.sh:151-176 +
     scripts/generate_bottleneckCB8share_onehottrain_config.py:8-102; cv-update: scripts/add_flopsconstraint.py:18-30).
     bn_num_choices = C in 2..8 turns every tdnnf layer into: X.linear (-> sum of bn_choice_dims, must equal
     bottleneck_dim[]) split into C column blocks of widths bn_choice_dims[k]; block k is multiplied (ElementwiseProduct)
     by CopyN(Sum(p_k..p_{C-1})) where p (C values, the same for every row) comes from
       bn_mode 0: OnehotFunctionComponent "X.softmax" (one uniform draw per layer and minibatch; its C-vector
                  output_ is updated with lr * colsum(deriv) although nothing reads it, nnet-simple-component.cc:9521-9552)
       bn_mode 1: ConstantFunctionComponent "X.alpha" (C logits, update 5 * lr * colsum, :2636) -> SoftmaxFlopsComponent
       bn_mode 2: the same through GumbelSoftmaxFlopsComponent (C uniform draws, bn_temp_proportion)
     and X.affine reads the masked blocks.  The FLOPs penalty of modes 1/2 adds bn_flops_scale / (rows * C) * flops_k to
     every row of d p with flops_k = -(bn_choice_dims[0] + ... + bn_choice_dims[k]) (the reference hard-codes
     -25 ... -240, :10006-10017).  0 = off.  Not combinable with darts_num_offsets. */
  int bn_num_choices;
  int bn_choice_dims[8];
  int bn_mode;
  float bn_flops_scale;
  float bn_temp_proportion;
  /* != 0: cross-validation architecture update (run_TDNN_DARTSV3_fbk_stride_cvupdate.sh:128-142,
     run_TDNNf_DARTS_mod_fbk_bottleneckCBshare_cvupdate_flopsconstraint.sh:136-139): every BatchNormComponent becomes a
     BatchNormTestComponent (scale / offset from the stored statistics: load them with tdnnf_net_set_stats, nothing is
     accumulated or rescaled), learning-rate factor 0 on every component (no model derivative is computed for them)
     except 1e-4 on the TdnnDARTSV3Components and 1 on the X.alpha vectors of the bottleneck supernet. */
  int cv_update;
  /* Arithmetic of the trainer's GEMMs.  0: exact f32 MFMA (v_mfma_f32_32x32x2_f32), the reference's BaseFloat.
     1: split-bf16: every f32 operand is a_hi + a_lo in bf16 and a b ~ a_hi b_hi + a_hi b_lo + a_lo b_hi on
     v_mfma_f32_32x32x16_bf16 with f32 accumulation (products to ~2^-16 relative; BASELINE configs[4] names
     "fp32 objf / bf16 MFMA GEMM").  The objective, BatchNorm, the optimizer step and all reductions stay f32 / f64.
     2: the same with three bf16 planes per operand and the six products a_i b_j, i + j <= 2 (24 mantissa bits per
     operand, products to ~2^-24 relative: f32-equivalent results from the bf16 matrix cores).  With option "planes" (default) and
     a minibatch large enough to run on one stream, operands are split ONCE into planes in HBM (tdnnf_planes_*) instead of in the kernels.
     3: "f16x3": every GEMM operand is split once into two f16 planes after scaling by the power of two its Frobenius norm allows
     (no element can overflow), a b ~ h h' + h l' + l h' on v_mfma_f32_32x32x16_f16 with f32 accumulation: 22-23 operand bits,
     f32-equivalent results in norm (tests/test_gpu_planes_gemm.py) at 3/16 of the f32 MFMA's cycles and 4 bytes per operand element;
     GEMMs the planes do not cover (tap coefficients, row strides, small minibatches) run exact f32. */
  int gemm_precision;
  /* Derived child networks (local/chain_NAS/scripts/generate_top_list.py:97-141, generate_optimal_stride.py): when
     use_layer_offsets != 0, layer l's X.linear has time-offsets {-offset_left[l], 0} and its X.affine {0, offset_right[l]}
     (a single tap where the offset is 0) instead of the symmetric time_stride[l]; any values in 0..64.  Ignored by the
     offset supernet (darts_num_offsets >= 2). */
  int use_layer_offsets;
  int offset_left[TDNNF_NET_MAX_LAYERS];
  int offset_right[TDNNF_NET_MAX_LAYERS];
  /* GeneralDropoutComponent of tdnn1 and of every tdnnf layer (UPSTREAM; emitted with "continuous=true" and no
     time-period by composite_layers.py:186-199: one mask row per sequence, shared over time, scale uniform on
     [1 - 2p, 1 + 2p]).  The recipes train with --trainer.dropout-schedule '0,0@0.20,0.5@0.50,0'
     (run_tdnn_fbk_40_iv_sp_7q.sh:48,216).  use_dropout != 0 reserves the masks and (num_layers + 1) * num_sequences *
     hidden_dim further random draws per step (after the others); the proportion p of the moment is set with
     tdnnf_net_set_dropout_proportion (0 = identity, the initial value).  Off in cv-update mode (test mode). */
  int use_dropout;
} tdnnf_net_config;
typedef struct tdnnf_net tdnnf_net;

/* ========================================================================== egs
 * Chain examples ("cegs" archives of NnetChainExample) in and out, and their merge into the buffers
 * tdnnf_net_forward_backward / tdnnf_supervision_create take.  Host code, no GPU needed.  The formats are upstream
 * Kaldi / OpenFst (nnet3/nnet-chain-example.cc, nnet-example.cc, chain/chain-supervision.cc, matrix/compressed-matrix.cc,
 * OpenFst compact-fst.h), restated; the reference only passes flags for them (run_TDNN_DARTSV3_fbk_stride_pretrain.sh:192-199,
 * steps/nnet3/chain/train.py:373-406).  Binary archives only. */
typedef struct tdnnf_egs_reader tdnnf_egs_reader;
typedef struct tdnnf_egs_writer tdnnf_egs_writer;
typedef struct tdnnf_eg tdnnf_eg;
int tdnnf_egs_reader_open(const char *path, tdnnf_egs_reader **out);
void tdnnf_egs_reader_close(tdnnf_egs_reader *);
/* *out = the next example, or NULL at the end of the archive (still TDNNF_OK) */
int tdnnf_egs_reader_next(tdnnf_egs_reader *, tdnnf_eg **out);
void tdnnf_eg_destroy(tdnnf_eg *);
const char *tdnnf_eg_key(const tdnnf_eg *);
/* input "input" / "ivector": dimensions and the time of its first row; copy of the (decompressed) rows x cols values */
int tdnnf_eg_input_info(const tdnnf_eg *, const char *name, int *rows, int *cols, int *first_t);
int tdnnf_eg_input_copy(const tdnnf_eg *, const char *name, float *out);
int tdnnf_eg_supervision_info(const tdnnf_eg *, float *weight, int *num_sequences, int *frames_per_seq, int *label_dim, int *num_states,
                              int *num_arcs, int *first_t, int *t_step);
/* nnet3-chain-merge-egs for n single-sequence examples (+ nnet3-chain-copy-egs --frame-shift): features t-major
   (row = (t - first_t) * n + b, t = first_t .. first_t + num_t - 1 as tdnnf_net_input_frames reports), ivectors n x dim
   (NULL if unused), and the arrays of tdnnf_supervision_create (sizes from tdnnf_egs_merge_sizes; labels are pdf-id + 1,
   weights costs: arc_pdf = label - 1, log-probs = -cost). */
int tdnnf_egs_merge_sizes(const tdnnf_eg *const *egs, int n, int *num_states, int *num_arcs, int *frames_per_seq, int *feat_dim, int *ivector_dim);
int tdnnf_egs_merge(const tdnnf_eg *const *egs, int n, int first_t, int num_t, int frame_shift, float *feats, float *ivectors, int *seq_state_begin,
                    int *seq_arc_begin, int *state_time, float *final_logprob, int *arc_src, int *arc_dst, int *arc_pdf, float *arc_logprob,
                    float *weight_out);
int tdnnf_egs_writer_open(const char *path, tdnnf_egs_writer **out);
int tdnnf_egs_writer_close(tdnnf_egs_writer *);
/* one single-sequence example; the supervision as ONE sequence's arrays of tdnnf_supervision_create (state 0 = start);
   compress != 0 writes the features as a 16-bit CompressedMatrix ("CM2"), as nnet3-chain-get-egs does by default */
int tdnnf_egs_writer_write(tdnnf_egs_writer *, const char *key, const float *feats, int rows, int feat_dim, int first_t, const float *ivector,
                           int ivector_dim, int compress, float weight, int frames, int t_step, int label_dim, int num_states, int num_arcs,
                           const float *final_logprob, const int *arc_src, const int *arc_dst, const int *arc_pdf, const float *arc_logprob);

int tdnnf_net_create(const tdnnf_net_config *cfg, tdnnf_net **out);
/* A second net for ANOTHER MINIBATCH SHAPE of the same model (cfg differing from the primary's only in frames_per_chunk /
   num_sequences): the recipes cut examples of several chunk widths (--egs.chunk-width 150,110,100) and merge each width
   into its own minibatches.  It shares the primary's natural-gradient preconditioners and model statistics (BatchNorm /
   ReLU); give it the primary's parameter and gradient buffers with tdnnf_net_set_buffers.  Use the nets one after the
   other on one stream; destroy the primary last. */
int tdnnf_net_create_shared(const tdnnf_net_config *cfg, const tdnnf_net *primary, tdnnf_net **out);
void tdnnf_net_destroy(tdnnf_net *);
long long tdnnf_net_num_params(const tdnnf_net *);
int tdnnf_net_num_components(const tdnnf_net *);
/* name_out: >= 64 bytes.  Weights are rows x cols at [begin, begin + rows*cols), bias (if has_bias) follows. */
int tdnnf_net_component_info(const tdnnf_net *, int index, char *name_out, long long *begin, int *rows, int *cols,
                             int *has_bias, float *lr_factor, float *l2, float *max_change, float *orthonormal);
/* DARTS components: number K of architecture logits stored between the weights and the bias
   (bias_params_[0:K] of the reference, nnet-tdnn-component.cc:172-176); 0 for every other component. */
int tdnnf_net_component_num_alpha(const tdnnf_net *, int index);
/* Uniform(0,1) draws consumed by one forward pass of a DARTS net: (K + 1) per DARTS component, in component
   order (K Gumbel uniforms, then the tap-sample uniform).  The caller fills a device buffer before every step. */
int tdnnf_net_num_random_draws(const tdnnf_net *);
int tdnnf_net_set_random_draws(tdnnf_net *, const float *draws_dev);
/* rows of the t-major feature matrix the net consumes: (frames_per_chunk + left + right context) * B */
int tdnnf_net_input_frames(const tdnnf_net *, int *num_t_in, int *first_t);
int tdnnf_net_set_buffers(tdnnf_net *, float *params_dev, float *grads_dev);
/* forward + chain objective + backward; ACCUMULATES raw gradients (is_gradient_ semantics) into grads.
   results_dev: as tdnnf_chain_objf_and_deriv.  step selects the pseudo-random decisions of this minibatch
   (ReLU stats / self-repair coin flips). */
int tdnnf_net_forward_backward(tdnnf_net *, const tdnnf_mat *feats, const tdnnf_mat *ivectors, const tdnnf_den_graph *,
                               const tdnnf_supervision *, double *results_dev, long long step, tdnnf_stream);
/* The objective of one minibatch without derivatives (nnet3-chain-compute-prob, the evaluations of nnet3-chain-combine): the forward
   pass of tdnnf_net_forward_backward on the same buffers, then tdnnf_chain_objf -- the denominator beside the xent head's forward pass,
   everything joined onto `stream` before the call returns.  Every configuration tdnnf_net_forward_backward accepts; draws from
   tdnnf_net_set_random_draws as there.  Only the parameter buffer is used: the gradient buffer is neither read nor written.  No backward-data GEMM, weight
   gradient, natural-gradient pass or refresh upload, ReLU statistics or self-repair, gradient-scratch fill, W^T transpose; no
   derivative buffer is written.
   flags = 0: the call leaves no trace in the net -- parameters, gradients, BatchNorm and ReLU statistics, preconditioner state and the
   step count are as before, and a training run with such calls between its steps has the bits of the run without them.
   TDNNF_OBJECTIVE_STORE_BATCHNORM_STATS (ignored when cv_update != 0): the BatchNorm statistics accumulate exactly as in the forward
   half of tdnnf_net_forward_backward (RecomputeStats); ReLU statistics stay untouched -- they come from the backward sweep.
   The call marks no phase boundaries: tdnnf_net_phase_times keeps reporting the last training step's times. */
#define TDNNF_OBJECTIVE_STORE_BATCHNORM_STATS 1
int tdnnf_net_objective(tdnnf_net *, const tdnnf_mat *feats, const tdnnf_mat *ivectors, const tdnnf_den_graph *,
                        const tdnnf_supervision *, double *results_dev, int flags, tdnnf_stream);
/* Data-parallel callers may overlap the gradient all-reduce with the backward pass: the flat gradient buffer is final
   bucket by bucket -- contiguous ranges, whole layers, >= 16 MB where the model allows, in the order backward finishes
   them (heads + prefinal-l first, then tdnnf layers from the top down, tdnn1 last; together they cover the buffer).
   tdnnf_net_forward_backward records an event per bucket once grads[begin, end) holds this minibatch's contribution;
   tdnnf_net_wait_grad_bucket makes `stream` wait for it (hipStreamWaitEvent), so a collective enqueued there afterwards
   runs beside the rest of the backward pass.  (forward_backward's own stream is complete, as before, when it returns.) */
int tdnnf_net_num_grad_buckets(const tdnnf_net *);
int tdnnf_net_grad_bucket(const tdnnf_net *, int index, long long *begin, long long *end);
int tdnnf_net_wait_grad_bucket(const tdnnf_net *, int index, tdnnf_stream stream);
/* delta = lr_c*(grad) - 2*l2_scale*lr_c*l2_c*params; max-change; params += delta; grads = 0; orthonormal
   constraint on the scheduled quarter of the constrained matrices; batchnorm stats *= batchnorm_stats_scale. */
int tdnnf_net_update(tdnnf_net *, float learning_rate, float l2_regularize_scale, long long step, tdnnf_stream);
/* The nnet edit "set-temperature-proportion name=* proportion=p" of the temperature schedule
   (steps/libs/nnet3/train/temperature_schedule.py:51-60, applied by train.py:527-531 before every iteration): sets the
   Temp-Proportion of every TdnnDARTSV3Component and GumbelSoftmax(Flops)Component of the net.  p > 0. */
/* "nnet3-copy --edits='set-dropout-proportion name=* proportion=p'" of train.py's dropout schedule */
int tdnnf_net_set_dropout_proportion(tdnnf_net *, float proportion);
int tdnnf_net_set_temperature_proportion(tdnnf_net *, float proportion);
/* ---- f32-equivalent GEMMs on the 16-bit matrix cores from pre-split operands (csrc/abi_planes.hip; the split: csrc/planes_split.hip,
   the GEMM: csrc/planes_gemm.hip).
   An operand is split ONCE into 16-bit planes laid out for the consumer ("P16": [K block of 16][plane][row][16], 32-byte row
   records, zero rows in front of and behind the matrix so that row-shifted tap views and tile overhang read zeros):
     num_planes 3 ("bf16x6", gemm_precision 2): x = p0 + p1 + p2, three bf16 planes, the six products p_i q_j with i + j <= 2;
     num_planes 2 ("f16x3",  gemm_precision 3): x s = h + l, two f16 planes of the operand scaled by the power of two s that its
       Frobenius norm allows (s ||X||_F <= 65504: no element can overflow, whatever the data), the three products h h', h l', l h';
       the split writes the record [s, 1 / s, ||X||_F] (room for 4 floats) to scale_dev and the GEMM multiplies its result by 1 / (s s').
   Both accumulate in f32.  tdnnf_planes_split writes the row-major planes (k = column; `planes`, rows_total = lead_rows + rows +
   zero tail rows) and / or the planes of the TRANSPOSE (k = row; `planes_t`, t_rows_total >= cols), for the products that reduce over
   the matrix's rows.  Sizes: tdnnf_planes_bytes(num_planes, rows_total, k_blocks) with k_blocks = ceil(cols / 16), resp.
   4 ceil(rows / 64) for the transposed planes.  workspace_dev: tdnnf_planes_split_workspace_bytes() (num_planes 2 only).
   tdnnf_planes_gemm: C (rows x cols) (op)= sum over segments s of  A[a_row[s] + m][a_first_col[s] .. + seg_cols[s]) .
   B[b_row[s] + n][b_first_col[s] .. + seg_cols[s])  -- segments = the taps of TdnnComponent::Propagate / Backprop
   (/root/reference/src/nnet3/nnet-tdnn-component.cc:302-324, :378-411): row-shifted views of one activation matrix against column
   blocks of the weight matrix (B: one row per output column, k contiguous).  a_row / b_row count rows of the plane buffers (lead rows
   included; b_row may be NULL = zeros); first columns must be multiples of 16; the A buffer needs zero rows up to the next multiple of
   256 output rows, the B buffer its rows padded to a multiple of 160 (cols nearer a multiple of 160), 256 or 128.
   init_mode 0: C += , 1: C = bias + , 2: C = . */
size_t tdnnf_planes_bytes(int num_planes, long long rows_total, long long k_blocks);
size_t tdnnf_planes_split_workspace_bytes(void);
/* how many GEMMs / weight gradients of the trainer ran on the plane kernels so far in this process (either pointer may be NULL) */
void tdnnf_planes_routed(long long *rows_gemms, long long *weight_gradients);
/* option "planes_check_bound": how many bound-derived scales were compared with the measured Frobenius norm, and how many bounds were too small */
void tdnnf_planes_bound_checks(long long *checks, long long *violations);
int tdnnf_planes_split(int num_planes, const tdnnf_mat *x, int lead_rows, long long rows_total, void *planes, long long t_rows_total, void *planes_t,
                       float *scale_dev, void *workspace_dev, tdnnf_stream);
int tdnnf_planes_gemm(int num_planes, const void *a_planes, long long a_rows_total, const float *a_scale_dev, const void *b_planes, long long b_rows_total,
                      const float *b_scale_dev, int num_segments, const long long *a_row, const long long *b_row, const int *a_first_col,
                      const int *b_first_col, const int *seg_cols, const float *bias, int init_mode, int relu, tdnnf_mat *c, tdnnf_stream);
/* The same product with the trainer's epilogue options: `add` (may be NULL): C[m] += add_scale * add[m - add_first_row] for the output rows the
   addend covers (the bypass term of the TDNN-F layers' Sum(Scale(0.66, .), .), fused into Backprop's data GEMM); `colstats` (may be NULL):
   column sums and sums of squares of the STORED output, one partial row per row tile of the launch -- colstats[t * cols + n] and
   colstats[(*colstats_rows + t) * cols + n], t < *colstats_rows (written by the call: the tile height depends on the shape; at most
   ceil(rows / 128) rows each) -- what BatchNormComponent::Propagate needs of its input (nnet-normalize-component.cc:433-445). */
int tdnnf_planes_gemm_epilogue(int num_planes, const void *a_planes, long long a_rows_total, const float *a_scale_dev, const void *b_planes, long long b_rows_total,
                               const float *b_scale_dev, int num_segments, const long long *a_row, const long long *b_row, const int *a_first_col,
                               const int *b_first_col, const int *seg_cols, const float *bias, int init_mode, int relu, const tdnnf_mat *add, float add_scale,
                               int add_first_row, float *colstats, int *colstats_rows, tdnnf_mat *c, tdnnf_stream stream);
/* Synchronised BatchNorm for a data-parallel caller ("BN [sum x, sum x^2] (2 D floats per BN) for exact single-GPU
   equivalence").  The reference's BatchNormComponent takes its statistics over ALL rows of the minibatch
   (/root/reference/src/nnet3/nnet-normalize-component.cc:433-445); when the minibatch is sharded over world_size ranks, every
   train-mode BatchNorm of the net then all-reduces its column sums -- forward [sum x, sum x^2], backward [sum z dz, sum dz, sum dz^2],
   as doubles -- through `allreduce(ctx, buf, count, stream)`: an in-place SUM over the ranks of `count` doubles at device pointer
   `buf`, enqueued on `stream` (the trainer's compute stream; must not synchronise it), returning 0.  Mean, scale and the backward
   terms are then formed with the global row count: the sharded step equals the unsharded one.  Every rank must run the same net on
   the same number of rows.  allreduce == NULL switches it off (the default: statistics per shard, as Kaldi's per-job statistics).
   The typedef is spelled in capitals on purpose (not an exported symbol). */
typedef int TDNNF_ALLREDUCE_FN(void *ctx, double *buf, long long count, tdnnf_stream stream);
int tdnnf_net_set_batchnorm_sync(tdnnf_net *, TDNNF_ALLREDUCE_FN *allreduce, void *ctx, int world_size);

/* ---- The data-parallel exchanges on RCCL, issued from C++ on the library's streams (csrc/rccl_sync.hip).
   RCCL is resolved on first use (no link-time dependency): the copy ALREADY MAPPED in the process if there is one (a launcher that
   called torch.distributed's "nccl" backend has torch/lib/librccl.so live: a second copy must not be loaded beside it), else the
   global symbol scope, else dlopen by name; tdnnf_rccl_library_path reports "<path> [<how>]".  One process per GPU: rank 0 takes a unique id
   (128 bytes), the launcher's own channel distributes it (e.g. a torch.distributed broadcast), every rank creates its communicator
   on its current device.
   tdnnf_net_set_batchnorm_sync_rccl: the synchronised BatchNorm above with ncclAllReduce (doubles, in place) on the compute stream
     as the collective -- nothing host-side between the two finalize launches; comm NULL switches it off.
   tdnnf_net_allreduce_grads_rccl: the gradient exchange of one minibatch, call right after tdnnf_net_forward_backward: one
     ncclAllReduce (sum, f32) per gradient bucket (tdnnf_net_grad_bucket) on comm_stream, each behind the event recorded when that
     bucket became final, so the upper layers' reductions run under the lower layers' backward pass; `stream` then waits for the last.
   The two run on DIFFERENT streams inside one step, so they must be given DIFFERENT communicators (RCCL serialises the operations of
   one communicator in issue order: the buckets would queue behind every BatchNorm collective of the backward pass). */
int tdnnf_rccl_available(void);
int tdnnf_rccl_library_path(char *out, int out_bytes);
int tdnnf_rccl_unique_id(void *out_128_bytes);
int tdnnf_rccl_comm_create(const void *id_128_bytes, int world_size, int rank, void **comm_out);
void tdnnf_rccl_comm_destroy(void *comm);
int tdnnf_rccl_allreduce_sum(void *comm, void *buf_dev, long long count, int is_double, tdnnf_stream stream);
int tdnnf_net_set_batchnorm_sync_rccl(tdnnf_net *, void *comm, int world_size);
int tdnnf_net_allreduce_grads_rccl(tdnnf_net *, void *comm, tdnnf_stream comm_stream, tdnnf_stream stream);
/* The nnet edit "set-learning-rate-factor name=<pattern> learning-rate-factor=f" (ReadEditConfig,
   /root/reference/src/nnet3/nnet-utils.cc:1232-1256): SetLearningRateFactor(f) on every UPDATABLE component whose name matches
   the pattern ('*' matches any run of characters, as NameMatchesPattern; the fixed lda layer is not updatable).  The cv-update
   recipes freeze the parent model with it (run_TDNN_DARTSV3_fbk_stride_cvupdate.sh:129).  *num_set (optional): how many
   components matched ("Set learning rate factors for N components").  A factor of 0 stops the component's model derivative
   from being formed at all, as UpdatableComponent's "learning_rate_ != 0" guards do. */
int tdnnf_net_set_learning_rate_factor(tdnnf_net *, const char *name_pattern, float factor, int *num_set);
/* Model state outside the parameter vector, as doubles in network order (tdnn1, tdnnf2.., prefinal-chain, prefinal-xent):
   per BatchNorm [count, stats_sum[D], stats_sumsq[D]] (BatchNormComponent::StoreStats, nnet-normalize-component.cc:551-589)
   and per ReLU [count, value_sum[D], deriv_sum[D], oderiv_count, oderiv_sumsq[D]] (NonlinearComponent::StoreStatsInternal and
   StoreBackpropStats, nnet-component-itf.cc:433-480: the latter on three minibatches in four, always on the first);
   block order per unit: batchnorm, relu (heads: batchnorm1, relu, batchnorm2).  Host buffers; both calls synchronise. */
long long tdnnf_net_stats_size(const tdnnf_net *);
int tdnnf_net_get_stats(const tdnnf_net *, double *stats_host, tdnnf_stream);
int tdnnf_net_set_stats(tdnnf_net *, const double *stats_host, tdnnf_stream);
/* nnet3 "raw" model files of the network (what nnet3-copy reads and writes): "<Nnet3>", the config lines of the graph,
   "<NumComponents>" and every component in the token order of the reference's Write() functions (csrc/model_io.hip
   cites each one); binary != 0 writes Kaldi's binary encoding ("\0B" header, "FM"/"FV" blobs).  Parameters come from /
   go to the buffers of tdnnf_net_set_buffers, BatchNorm / ReLU statistics from / to the net (as tdnnf_net_get_stats).
   learning_rate is what the "<LearningRate>" tokens record (times each component's factor).  read_model matches
   components by name, checks dimensions and fails if a parameterised component of the net is missing from the file;
   both text and binary files are accepted.  Both calls synchronise the stream. */
int tdnnf_net_write_model(const tdnnf_net *, const char *path, int binary, float learning_rate, tdnnf_stream);
int tdnnf_net_read_model(tdnnf_net *, const char *path, tdnnf_stream);
/* The trainer configuration for the graph a model file holds (no GPU needed): dimensions from the component blocks,
   time strides / DARTS taps and flags from the Tdnn components, bypass scale and input dimensions from the config
   lines, l2 / max-change / self-repair from the tokens, BatchNormTestComponent => cv_update, the bottleneck supernet's
   blocks from its CopyN components.  What a model file does not record (chunk size, minibatch size, leaky-hmm,
   max-param-change ...) is set to the recipe's values (run_tdnn_fbk_40_iv_sp_7q.sh:149-203).  Fails for graphs other
   than the ones the trainer runs. */
int tdnnf_net_config_from_model(const char *path, int frames_per_chunk, int num_sequences, tdnnf_net_config *out);
/* The graph of a configuration as nnet3 config lines (input-node / component-node / dim-range-node / output-node: the
   part of a final.config that Nnet::Write keeps in a model file), newline-terminated, as tdnnf_net_write_model writes them.
   Mirrors the node lines of steps/libs/nnet3/xconfig/composite_layers.py:135-215,1283-1331 and of
   local/chain_NAS/scripts/generate_bottleneckCB8share_onehottrain_config.py:10-120, add_flopsconstraint.py:18-30.
   No GPU needed.  *needed (optional) receives the size including the terminating 0; out may be null with capacity 0 to
   query it. */
int tdnnf_net_config_text(const tdnnf_net_config *cfg, char *out, size_t capacity, size_t *needed);
/* diagnostics (tdnnf_set_option("phase_events", 1)): the last step's time between phase boundaries on the caller's stream, in ms:
   [0] forward trunk, [1] heads forward + objective issue, [2] heads backward (incl. the wait for the denominator), [3] trunk backward,
   [4] join of the side streams, [5] between forward_backward and update (collectives), [6] update.  *count = 7, or 0 when the option was
   off.  Synchronises the last event. */
int tdnnf_net_phase_times(tdnnf_net *, double *ms_out, int capacity, int *count);
/* debugging / parity: on != 0 makes the following forward_backward calls keep copies of the backward pass's derivative
   matrices (which otherwise live in recycled scratch): "<layer>.noop.deriv" (w.r.t. the layer output), "<layer>.affine.deriv",
   "<layer>.linear.deriv" (w.r.t. those components' outputs), "prefinal-l.deriv", "prefinal-{chain,xent}.{batchnorm2,linear,
   batchnorm1,affine}.deriv", "output-xent.deriv", "tdnn1.batchnorm.deriv", "tdnn1.affine.deriv"; served by tdnnf_net_get_activation.  Costs memory and copies: tests only. */
int tdnnf_net_set_capture(tdnnf_net *, int on);
/* debugging / parity: copy an internal activation by name ("tdnnf2.linear", "output", ...) into out */
int tdnnf_net_get_activation(const tdnnf_net *, const char *name, tdnnf_mat *out, tdnnf_stream);
int tdnnf_net_activation_dims(const tdnnf_net *, const char *name, int *rows, int *cols);

/* ======================================================================== inference (forward only, whole utterances)
 * The model's output for decoding: nnet3's DecodableNnetSimple (UPSTREAM, not shipped) restated -- what steps/nnet3/decode.sh
 * hands to latgen-faster-mapped (run_tdnn_fbk_40_iv_sp_7q.sh:254-258).  Utterances u = 0..U-1 of T_u input frames:
 *  - feats: sum T_u x feat_dim, the utterances stacked row-wise.  ivectors: R_u rows per utterance, stacked, one every
 *    ivector_period input frames; ivector_period <= 0: one per utterance (R_u = 1; ivector_rows_host may be NULL).
 *  - out: O_u = (T_u + fsf - 1) / fsf rows per utterance, stacked (fsf = frame_subsampling); row j of utterance u is the
 *    output at input frame j * fsf.  which_output 0: "output" (the chain head, raw, no log-softmax: what
 *    latgen-faster-mapped --acoustic-scale 1.0 reads); 1: "output-xent" (log-softmax of the xent head).
 *  - Chunks of F = frames_per_chunk input frames (a multiple of fsf): chunk k of utterance u covers input frames
 *    [k F, k F + F) widened by the model's left / right context at this chunk width (tdnnf_net_input_frames of a net with
 *    frames_per_chunk F); frames outside [0, T_u) are clamped to the first / last frame (nnet3's edge padding).  The last
 *    chunk is computed at full width, its rows past O_u are dropped.  With a constant i-vector the output does not depend on F.
 *  - I-vector of chunk k: n_k = its output rows inside O_u; row min(((k F / fsf) + n_k / 2) * fsf / ivector_period, R_u - 1)
 *    (integer arithmetic; the middle of the chunk, as DecodableNnetSimple::GetCurrentIvector does -- restated, not checked
 *    against Kaldi).
 *  - BatchNorm in test mode from the model's stored statistics (BatchNormTestComponent: epsilon 1e-3, target rms 1),
 *    dropout off, no ReLU statistics; nothing in the model is written.
 *  - Models: the 7q graph and derived children (layer offsets, per-layer bottleneck, strided affine rows).  The offset supernet
 *    (darts_num_offsets >= 2) and the bottleneck supernet (bn_num_choices > 0) fail with TDNNF_EINVAL.
 *  - Arithmetic: a property of the inference object, not of the model (whose parameters are f32 either way).
 *    tdnnf_infer_create builds exact f32 and accepts only models whose own gemm_precision is 0 (any other: TDNNF_EINVAL).
 *    tdnnf_infer_create_arith takes the arithmetic as an argument and does not consult the model's: gemm_precision 0 is exactly
 *    the f32 object, 3 is f16x3 -- every GEMM of the forward pass on the 16-bit matrix cores from operands split once into two
 *    scaled f16 planes (three products, f32 accumulation; held to the f32 tolerances), the weights split at the top of every
 *    compute, each activation as it is produced.  1 and 2 (the split-bf16 forms) and bf16x6 are not built for inference:
 *    TDNNF_EINVAL.  Streaming (tdnnf_online_*, below) is exact f32 only: its GEMMs run on a few rows per slot and step, where
 *    a 256-row plane tile is mostly padding. */
typedef struct tdnnf_infer tdnnf_infer;
/* binds the model net's parameter buffer and statistics by reference (read at every compute: an update or set_stats on the
   model is seen by the next call); max_chunks bounds the chunks of one batch (the arena is sized for it) */
int tdnnf_infer_create(const tdnnf_net *model, int frames_per_chunk, int max_chunks, int which_output, tdnnf_infer **out);
/* the same object in the arithmetic gemm_precision (0: f32, what tdnnf_infer_create builds; 3: f16x3; 1, 2, anything else:
   TDNNF_EINVAL); the model is checked as above except for its own cfg.gemm_precision.  The scalar arguments are checked
   first, before the model is looked at and before any device call. */
int tdnnf_infer_create_arith(const tdnnf_net *model, int frames_per_chunk, int max_chunks, int which_output, int gemm_precision,
                             tdnnf_infer **out);
void tdnnf_infer_destroy(tdnnf_infer *);
/* host only, no device call: the chunk plan above -- per chunk 4 ints (utterance, first input frame k F, i-vector row within
   the utterance, valid output rows n_k); *num_chunks = the number of chunks.  More than `capacity` chunks: the first
   `capacity` are written and the call fails (TDNNF_EINVAL) with *num_chunks still set. */
int tdnnf_infer_plan(const tdnnf_infer *, int num_utts, const int *frames_host, const int *ivector_rows_host, int ivector_period,
                     int *chunks_out, int capacity, int *num_chunks);
/* the same plan for a chunk width and frame_subsampling alone (no model, no device): what tdnnf_infer_plan returns for a
   model with that frame_subsampling and frames_per_chunk; frames_per_chunk not a positive multiple of it: TDNNF_EINVAL */
int tdnnf_chunk_plan(int frames_per_chunk, int frame_subsampling, int num_utts, const int *frames_host, const int *ivector_rows_host,
                     int ivector_period, int *chunks_out, int capacity, int *num_chunks);
/* feats / ivectors / out: stacked as above (device); any number of chunks (batches of max_chunks inside).  Does not
   synchronise the stream. */
int tdnnf_infer_compute(tdnnf_infer *, int num_utts, const int *frames_host, const tdnnf_mat *feats, const int *ivector_rows_host,
                        const tdnnf_mat *ivectors, int ivector_period, tdnnf_mat *out, tdnnf_stream);
/* of the last compute: BatchNorm stages (tdnn1, every tdnnf layer, the head's two: num_layers + 3) applied in a GEMM epilogue
   -- with the layer's bypass --, and those applied by a separate elementwise pass (tdnnf layers whose bypass rows are strided
   against their output rows) */
int tdnnf_infer_counts(const tdnnf_infer *, int *fused_layers, int *fallback_passes);
/* of the last compute, summed over its batches: GEMM launches of the forward pass that ran from f16 planes, and those that
   ran on the f32 kernels -- all of them in an f32 object; in an f16x3 object the ones whose operands did not fit the plane
   kernels.  The splits of the weights and activations are not counted.  A forward pass is 2 num_layers + 6 GEMMs per batch:
   lda, tdnn1, every layer's .linear and .affine, prefinal-l, the head's affine and linear, the output. */
int tdnnf_infer_gemm_counts(const tdnnf_infer *, long long *plane_gemms, long long *f32_gemms);

/* CHUNK INPUTS: the input of tdnnf_net_forward_backward for a minibatch of chunks, gathered on the device from whole utterances -- the
   features of the chunks whose supervisions "ALIGNMENT CHUNKS" compiles, so that a training pass over aligned utterances needs no archive
   and no host-built array of features.
   Utterances u = 0..U-1 have frames[u] input frames; their features are stacked row-wise in one device matrix exactly as
   tdnnf_infer_compute takes them, their i-vectors the same way: R_u rows each, one every ivector_period input frames, or
   ivector_period <= 0 for one per utterance (R_u = 1; ivector_rows_host is then not read).  fsf = frame_subsampling,
   O_u = (frames[u] + fsf - 1) / fsf.  Sequence b of a minibatch of B is the output frames [begin_b, begin_b + T) of utterance seq_utt[b],
   T = frames_per_sequence; first_t and num_t are what tdnnf_net_input_frames reports.
     feats_out     (num_t * B) x feat_dim, t-major: row (t - first_t) * B + b, t = first_t .. first_t + num_t - 1, is feature row
                   clamp(begin_b * fsf + t - frame_shift, 0, frames[u] - 1) of utterance u.  frame_shift has the sign of tdnnf_egs_merge
                   (example times += frame_shift); clamping is nnet3's edge padding, as in "inference".
     ivectors_out  B x ivector_dim: row b is i-vector row min(((begin_b + T / 2) * fsf) / ivector_period, R_u - 1) of utterance u, or row 0
                   for ivector_period <= 0 (integer divisions: the rule of tdnnf_infer_plan with k F / fsf -> begin_b, n_k -> T).  With
                   ivector_dim == 0 (ivectors NULL or of no columns) no i-vector argument is read or written.
   Refused with TDNNF_EINVAL, by name, before any device call and leaving the handle as it was: begin_b < 0, begin_b + T > O_u, seq_utt[b]
   outside [0, U) (each naming the sequence); frames[u] < 1, R_u < 1 where i-vectors are used (naming the utterance);
   |frame_shift| >= fsf; feats, ivectors, feats_out or ivectors_out of another shape than the above; more sequences than max_sequences
   (named with the excess, as the assigns name a capacity).
   tdnnf_chunk_input_create makes every allocation: the device table and two pinned staging buffers that take turns (the ring of the
   reserved-handle assigns: turn k waits only for the copies of turn k - 2).  tdnnf_chunk_input_plan is host only, no device, no handle: the
   table of a minibatch, 4 ints a sequence -- the first stacked feature row of its utterance, the utterance's frames[u], the window start
   begin_b * fsf - frame_shift, the stacked i-vector row (0 when ivector_period > 0 comes without ivector_rows_host: no i-vectors) -- after
   the same checks.  tdnnf_chunk_input_gather validates, stages those 16 bytes a sequence and enqueues one copy and ONE kernel on `stream`
   (csrc/chunk_input_kernels.h: a grid-stride copy through the table, consecutive lanes on consecutive columns of one output row; 16-byte
   loads and stores where feat_dim, ivector_dim, every stride and every base pointer allow, else a float at a time; the i-vector rows in
   the same launch).  No allocation, no free, no stream or device synchronise; work enqueued on `stream` before a gather still reads the
   outputs of the previous one if they are other buffers.  It takes first_t / num_t / frame_subsampling as integers, not a net.
   tdnnf_chunk_input_info: allocations made since create (0), successful gathers, and the form of the last (4: 16-byte, 1: scalar, 0: none
   yet); any out-pointer may be NULL.
   Stored (8- and 16-bit) features: "FEATURE STORES" below, tdnnf_chunk_input_gather_stored.
   Not built: chunks shorter than T at an utterance's end, frame-rate (not output-rate) alignments, device-side validation, capture into
   a HIP graph. */
typedef struct tdnnf_chunk_input tdnnf_chunk_input;
int tdnnf_chunk_input_create(int max_sequences, tdnnf_chunk_input **out);
void tdnnf_chunk_input_destroy(tdnnf_chunk_input *);
int tdnnf_chunk_input_plan(int frame_subsampling, int frames_per_sequence, int num_sequences, const int *seq_utt_host, const int *chunk_begin_host,
                           int frame_shift, int num_utts, const int *frames_host, const int *ivector_rows_host, int ivector_period, int *table_out);
int tdnnf_chunk_input_gather(tdnnf_chunk_input *, int first_t, int num_t, int frame_subsampling, int frames_per_sequence, int num_sequences,
                             const int *seq_utt_host, const int *chunk_begin_host, int frame_shift, int num_utts, const int *frames_host,
                             const tdnnf_mat *feats, const int *ivector_rows_host, const tdnnf_mat *ivectors, int ivector_period, tdnnf_mat *feats_out,
                             tdnnf_mat *ivectors_out, tdnnf_stream stream);
int tdnnf_chunk_input_info(const tdnnf_chunk_input *, int *max_sequences, long long *allocations, long long *gathers, int *last_form);

/* FEATURE STORES: the utterances' features kept on the device as Kaldi stores them, CompressedMatrix codes, and decoded where they are
   read -- in the gather of a chunk minibatch and in an expand for the whole-utterance passes.  A resident training set then costs what its
   archive does: 1 byte a value ("CM", what copy-feats --compress=true writes, and "CM3") or 2 ("CM2", what the recipes' egs hold), not 4.
   VALUE OF A CODE, float32, one rounding an operation, in this order, never contracted into an FMA (csrc/feature_code_value.h, which the egs
   reader's read_general_matrix uses too: the two agree bit for bit).  k16 = 1.0f / 65535.0f; (min, range) the matrix's global header:
     format 2 "CM2", code w (uint16):  min + range * k16 * w
     format 3 "CM3", code b (uint8):   min + range * (1.0f / 255.0f) * b
     format 1 "CM",  code b (uint8) of column j with percentiles h0..h3 (uint16), p_i = min + range * k16 * h_i:
                     b <= 64: p0 + (p1 - p0) * b * (1.0f / 64.0f);  b <= 192: p1 + (p2 - p1) * (b - 64) * (1.0f / 128.0f);
                     else: p2 + (p3 - p2) * (b - 192) * (1.0f / 63.0f)
   A STORE holds one format (1, 2 or 3) and one feat_dim, and up to max_utterances utterances of max_frames frames in all (< 2^31), all
   fixed at create, which makes every allocation.  BYTE LAYOUT, w = 2 bytes a code in format 2, else 1: utterance u's codes are row-major
   (Kaldi's format 1 is column-major: transposed on the host at append, so that lanes on consecutive columns read consecutive bytes) at
   byte offset[u] of the code buffer, offset[0] = 0, offset[u + 1] = offset[u] + round_up(frames[u] * feat_dim * w, 16): every utterance
   begins at a 16-byte boundary; offsets are 64-bit.  Beside the codes an utterance takes a 32-byte table entry (offset, frames, header row,
   min, range) and, in format 1, its p0..p3 as four floats a column, computed on the host by the expression above.  So
     device_bytes = sum_u round_up(frames[u] * feat_dim * w, 16) + U * (32 + (format == 1 ? 16 * feat_dim : 0)),
   which tdnnf_feature_store_layout computes on the host (no device, no handle; offsets_out: num_utts + 1 entries, or NULL) and
   tdnnf_feature_store_info reports of a store; reserved_bytes is the arena create allocated for the capacities.
   APPEND takes payloads in Kaldi's order, exactly as an archive holds them behind the token (format 1: percentiles cols x 4 uint16, codes
   cols x rows bytes column-major; format 2: rows x cols uint16; format 3: rows x cols bytes), validates, packs and copies them behind the
   store's last utterance; or (append_float) compresses float matrices -- rows_host[i] rows each, feat_dim columns, stacked contiguously
   -- on the host by write_matrix's rule, bit for bit: [min, max] of the matrix, max = min + 1 where not max > min, code
   (uint16) min(65535, max(0, (x - min) / range * 65535 + 0.499)) in format 2, the same with 255 and uint8 in format 3; format 1 from floats
   is refused by name (Kaldi's percentile selection is not built).  An append is a load-time call: it waits for its copies, makes no device
   or pinned allocation, and writes only bytes no earlier call reads.  Utterances are numbered in append order.
   Refused with TDNNF_EINVAL, by name, before any device call and leaving the store as it was: more utterances or frames than reserved
   (naming the excess, as the assigns name a capacity), cols != feat_dim, rows < 1, a non-finite min or range (of a payload, or of a float
   matrix), a payload of another format than the store's.
   USE.  tdnnf_feature_store_expand writes the decoded rows of the listed utterances, stacked in list order, any order, repeats allowed:
   the matrix tdnnf_infer_compute and tdnnf_chunk_input_gather take.  It stages 8 bytes a list entry through the store's own ring (two
   pinned buffers of 8 KB that take turns, whatever the capacities) and enqueues one copy and one kernel a piece of 1024 entries.
   tdnnf_chunk_input_gather_stored is tdnnf_chunk_input_gather, "CHUNK INPUTS" word for word, with "feature row r of utterance u" read as
   the decoded row r of the store's utterance u: seq_utt indexes the store, frames[u] is the store's, ivector_rows_host has one entry an
   utterance of the store; the clamp, the frame shift, the i-vector row and the refusals are the same (named chunk_input_gather_stored);
   i-vectors stay float.  It stages the same 16 bytes a sequence through the chunk-input handle's ring -- the table's first entry the
   utterance's index -- and enqueues one copy and ONE kernel; the per-utterance facts come from the table the store built at append.
   Neither call allocates, frees or synchronises a stream or the device; work enqueued on `stream` before it still reads the outputs of
   the previous call if they are other buffers.  Kernels (csrc/feature_store_kernels.h): the grid-stride walk of chunk_input_gather_kernel;
   form 4, where feat_dim is a multiple of 4 and the outputs' (and i-vectors') strides and base pointers allow 16 bytes: a lane takes 4
   columns, its codes in one 4- or 8-byte load, one 16-byte store; else form 1, a code at a time.
   tdnnf_feature_store_info: the store's format, feat_dim, utterances, frames, device_bytes (the closed form), reserved_bytes, device and
   pinned allocations since create (0), successful gathers and expands, the form of the last of either (4, 1; 0: none yet); any
   out-pointer may be NULL.  tdnnf_chunk_input_info keeps counting the float gathers alone.  tdnnf_feature_store_frames: frames[first ..
   first + count) of the store.
   Host only, no device, no handle, the functions the appends use (csrc/feature_store_plan.h): tdnnf_feature_store_layout (above);
   tdnnf_feature_store_pack: one payload's header floats (format 1: 4 * feat_dim, p0..p3 a column; else header_out is not written and may
   be NULL) and its rows * feat_dim codes row-major, after the payload's checks; tdnnf_feature_store_compress: (min, range) and the codes
   of a float matrix in format 2 or 3.
   Not built: format-1 compression of float input, removing or replacing utterances, mixed formats in one store, compressed i-vectors,
   decoding inside tdnnf_infer_compute's own gather (an expand costs one float copy of a batch), streaming input from a store, device-side
   validation, capture into a HIP graph. */
typedef struct tdnnf_feature_store tdnnf_feature_store;
typedef struct {
  int format; /* 1 "CM", 2 "CM2", 3 "CM3" */
  float min_value, range;
  int rows, cols;
  const void *percentiles; /* format 1: cols x 4 uint16; else not read */
  const void *codes;
} tdnnf_feature_payload;
int tdnnf_feature_store_create(int format, int feat_dim, int max_utterances, long long max_frames, tdnnf_feature_store **out);
void tdnnf_feature_store_destroy(tdnnf_feature_store *);
int tdnnf_feature_store_layout(int format, int feat_dim, int num_utts, const int *frames_host, long long *offsets_out, long long *device_bytes_out);
int tdnnf_feature_store_pack(int feat_dim, const tdnnf_feature_payload *item, float *header_out, void *codes_out);
int tdnnf_feature_store_compress(int format, int rows, int cols, const float *matrix_host, float *min_out, float *range_out, void *codes_out);
int tdnnf_feature_store_append(tdnnf_feature_store *, int num_items, const tdnnf_feature_payload *items);
int tdnnf_feature_store_append_float(tdnnf_feature_store *, int num_items, const int *rows_host, const float *matrices_host);
int tdnnf_feature_store_expand(tdnnf_feature_store *, int num_utts, const int *utt_host, tdnnf_mat *out, tdnnf_stream stream);
int tdnnf_chunk_input_gather_stored(tdnnf_chunk_input *, int first_t, int num_t, int frame_subsampling, int frames_per_sequence, int num_sequences,
                                    const int *seq_utt_host, const int *chunk_begin_host, int frame_shift, tdnnf_feature_store *store,
                                    const int *ivector_rows_host, const tdnnf_mat *ivectors, int ivector_period, tdnnf_mat *feats_out,
                                    tdnnf_mat *ivectors_out, tdnnf_stream stream);
int tdnnf_feature_store_info(const tdnnf_feature_store *, int *format, int *feat_dim, int *utterances, long long *frames, long long *device_bytes,
                             long long *reserved_bytes, long long *allocations, long long *gathers, long long *expands, int *last_form);
int tdnnf_feature_store_frames(const tdnnf_feature_store *, int first, int count, int *frames_out);

/* ======================================================================== inference (forward only, streaming)
 * The same output for streams whose features arrive a few frames at a time: nnet3's looped computation
 * (DecodableNnetLoopedOnline, UPSTREAM, not shipped) restated.  Same models, outputs and BatchNorm as "inference" above, and the
 * same rejections.  fsf = frame_subsampling.
 *  - Slots: num_slots streams, each with its own clock (an input frame index) and its own carried state on the device.
 *    Parameters and BatchNorm statistics are bound by reference (read at every step).
 *  - Context: left / right = the model's true context in input frames, from the taps (lda splice 1 + every layer's left /
 *    right tap), not from a chunk's rho-padded grids.  Latency D = right rounded up to a multiple of fsf.
 *  - Reset starts a new utterance in a slot: its carried state is zeroed (no value of an earlier utterance can be read
 *    again) and its clock set to -W, W = left rounded up to a multiple of F = frames_per_step.
 *  - Step: a list of active slots, each at most once, in any order; per slot a row count n_b, a `final` flag and one i-vector
 *    row; feats = the passed rows of the active slots stacked in list order (sum n_b x feat_dim); out = num_active * F / fsf
 *    rows.  Every active slot advances by one window of F input frames [clock, clock + F); the others keep state and clock.
 *     . The rows passed for a slot are the real frames of its window, in order.  A window position before the first passed row
 *       takes the first passed row, one after the last passed row takes the last (nnet3's edge padding).  So: the W warm-up
 *       frames (clock < 0) pass frame 0 alone, not final; a window at clock >= 0 that is not final passes exactly F rows; the
 *       window in which the utterance ends passes its remaining 1..F rows with `final` set (T = clock + n_b from then on);
 *       every later (flush) window passes the last frame alone with `final` set.  Anything else -- also a slot out of range
 *       or listed twice, or matrices of other dimensions -- fails with TDNNF_EINVAL before any launch and leaves every slot
 *       as it was.
 *     . The library keeps on the device whatever earlier frames and activations it still needs: a frame is never sent
 *       again, except as a clamp source.
 *     . Outputs: the step computes the head's outputs at input frames [clock - D, clock - D + F), stepping fsf; rows at
 *       frames below 0, or at or past T once `final` has been seen, are dropped.  Slot i's kept rows are written at
 *       out[i * F / fsf ...] (the rest of its F / fsf rows is not written); out_first_host[i] = the output index of the first
 *       one (row j of an utterance = input frame j * fsf), out_count_host[i] their number.  A slot is done once
 *       clock - D >= T; stepping it further emits nothing.
 *     . I-vector: the input-layer rows first computed in a step (frames clock - (D - right) - 1 onwards) use the i-vector
 *       passed in that step -- the online i-vector of the looped decodable.  With a constant i-vector the output equals the
 *       whole-utterance output of tdnnf_infer_compute.
 *     . Everything runs on the caller's stream; nothing synchronises (the step's table has a fixed size).
 *  - Schedule (host only, like tdnnf_chunk_plan): the steps of one utterance of T frames, 5 ints each: clock, first passed
 *    frame, passed rows, first output row, kept output rows; from clock -W while clock - D < T.  tdnnf_online_step follows
 *    exactly this arithmetic (one function serves both).
 *  - Counts of the last step: gemm_rows = output rows of all GEMM launches (each computes only the new rows);
 *    carried_rows = time rows x streams moved from the slots' state into the step's buffers (as many go back);
 *    fused / fallback = the BatchNorm stages as in tdnnf_infer_counts. */
typedef struct tdnnf_online tdnnf_online;
int tdnnf_online_create(const tdnnf_net *model, int frames_per_step, int num_slots, int which_output, tdnnf_online **out);
void tdnnf_online_destroy(tdnnf_online *);
int tdnnf_online_context(const tdnnf_online *, int *left, int *right, int *latency);
int tdnnf_online_reset(tdnnf_online *, int slot, tdnnf_stream);
/* a slot's clock and its utterance's length T (-1: `final` not seen yet) */
int tdnnf_online_slot(const tdnnf_online *, int slot, int *clock, int *frames);
/* more than `capacity` steps: the first `capacity` are written and the call fails (TDNNF_EINVAL) with *num_steps still set */
int tdnnf_online_schedule(int frames_per_step, int frame_subsampling, int left, int right, int frames, int *steps_out, int capacity,
                          int *num_steps);
int tdnnf_online_step(tdnnf_online *, int num_active, const int *slots_host, const int *rows_host, const int *final_host,
                      const tdnnf_mat *feats, const tdnnf_mat *ivectors, tdnnf_mat *out, int *out_first_host, int *out_count_host,
                      tdnnf_stream);
int tdnnf_online_counts(const tdnnf_online *, long long *gemm_rows, long long *carried_rows, int *fused, int *fallback);

/* ======================================================================== profiling
 * Optional per-launch timing of the MFMA GEMM kernels with HIP events recorded on the launch stream
 * (bench.py's live roofline measurement).  Classes: 0 = rows_gemm 128x128 tile, 1 = rows_gemm 128x160 tile,
 * 2 = wgrad, 3 = the skinny GEMMs of the natural-gradient statistics.  tdnnf_profile_read synchronises the recorded events and returns totals since enable. */
int tdnnf_profile_enable(int on);
int tdnnf_profile_read(int kernel_class, double *launches, double *total_ms, double *total_flops);
/* Algorithmic HBM bytes of the class's launches since enable, computed from the launch shapes: every operand element
   touched once -- 4 (distinct input rows x K-length + weight block + output rows x N [x 2 when added to]) per GEMM
   (e (N_in Di + K Di Do + N Do)); measured PMC traffic divided by this is the wasted-re-read ratio. */
int tdnnf_profile_read_bytes(int kernel_class, double *algorithmic_bytes);
const char *tdnnf_profile_class_name(int kernel_class);

#ifdef __cplusplus
}
#endif
#endif /* TDNNF_HIP_H_ */
