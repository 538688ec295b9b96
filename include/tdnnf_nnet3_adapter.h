// tdnnf_nnet3_adapter.h -- the Kaldi-side binding a maintainer adds to kaldi/src/nnet3 to route the
// hot-path components of skhu101/TDNN-F_NAS through libtdnnf_hip.so (C-ABI: tdnnf_hip.h).
//
// It is written against the only three things it needs from Kaldi's CuMatrixBase<float> -- Data(),
// NumRows()/NumCols(), Stride() (usage in the reference: src/nnet3/nnet-tdnn-component.cc:815-819) -- so it
// compiles stand-alone (tests/test_adapter_compile.py builds it against a 10-line stub) and inside a Kaldi
// tree unchanged.  Each function body is what replaces the body of the reference method cited above it;
// the surrounding class (config parsing, Read/Write, parameter storage) stays Kaldi's.
//
// Error behaviour: the C-ABI never throws; Check() turns a non-zero status into the exception/abort the
// reference uses (KALDI_ERR throws std::runtime_error; define TDNNF_ADAPTER_FAIL to KALDI_ERR inside Kaldi).
#ifndef TDNNF_NNET3_ADAPTER_H_
#define TDNNF_NNET3_ADAPTER_H_

#include <stdexcept>
#include <string>
#include <vector>

#include "tdnnf_hip.h"

#ifndef TDNNF_ADAPTER_FAIL
#define TDNNF_ADAPTER_FAIL(msg) throw std::runtime_error(msg)
#endif

namespace tdnnf_adapter {

inline void Check(int status) {
  if (status != TDNNF_OK) TDNNF_ADAPTER_FAIL(std::string("tdnnf: ") + tdnnf_last_error());
}

// CuMatrixBase<float> (or CuSubMatrix) -> tdnnf_mat.  Data() is the device pointer when Kaldi runs with a GPU.
template <class CuMat>
inline tdnnf_mat View(const CuMat &m) {
  tdnnf_mat v;
  v.data = const_cast<float *>(m.Data());
  v.rows = m.NumRows();
  v.cols = m.NumCols();
  v.stride = m.Stride();
  return v;
}

// TdnnDARTSV3Component::PrecomputedIndexes (nnet-convolutional-component.h:208-218) -> tdnnf_tdnn_indexes
inline tdnnf_tdnn_indexes Indexes(int row_stride, const std::vector<int> &row_offsets) {
  if (row_offsets.empty() || row_offsets.size() > TDNNF_MAX_OFFSETS) TDNNF_ADAPTER_FAIL("tdnnf: bad number of time offsets");
  tdnnf_tdnn_indexes ix;
  ix.row_stride = row_stride;
  ix.num_offsets = static_cast<int>(row_offsets.size());
  for (int i = 0; i < ix.num_offsets; i++) ix.row_offsets[i] = row_offsets[i];
  return ix;
}

// ---------------------------------------------------------------------------------------------------
// TdnnDARTSV3Component (src/nnet3/nnet-tdnn-component.cc).  State the Kaldi class already owns:
//   linear_params_ (Do x K*Di), bias_params_ (K + Do: first K = log-alpha), time_offsets_, the mode flags.
// The memo is a device buffer of 2K floats [coef | effective coef] instead of a heap CuVector (:330-332).
struct TdnnDartsState {
  int K, Di, Do, ldw;
  const float *linear_params;   // device
  const float *bias_params;     // device, K + Do (or null when use-bias=false)
  int flags;                    // TDNNF_DARTS_* from use_gumbel_/free_select_/uniform_sample_/use_entropy_/update_alpha_
  float temp_proportion;
  int share_index;              // (time_offsets_[1] > 0 ? 0 : K-1), :232-240
  bool offsets1_positive;       // time_offsets_[1] > 0
};

// Propagate :214-333.  uniform_draws_dev: K Gumbel uniforms then 1 sample uniform (the reference draws them
// with SetRandUniform(); pass a freshly filled CuVector<float>(K+1)).  memo_dev: 2K floats.
template <class CuMat>
inline void TdnnDartsPropagate(const TdnnDartsState &c, const tdnnf_tdnn_indexes &ix, const CuMat &in, CuMat *out,
                               const float *uniform_draws_dev, float *memo_dev, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_tdnn_darts_coef(c.bias_params, c.K, c.flags, c.temp_proportion, uniform_draws_dev, uniform_draws_dev + c.K,
                              c.share_index, memo_dev, memo_dev + c.K, stream));
  // :230-241: bias rows only when offsets[1] > 0, zero otherwise (quirk q1); no bias at all -> kPropagateAdds
  const int init_mode = c.bias_params == nullptr ? 0 : (c.offsets1_positive ? 1 : 2);
  const float *bias = c.bias_params ? c.bias_params + c.K : nullptr;
  Check(tdnnf_tdnn_propagate(&ix, &vin, c.linear_params, c.ldw, c.Do, c.Di, bias, memo_dev + c.K, init_mode, &vout, stream));
}

// The component's two OnlineNaturalGradient objects (preconditioner_in_ / preconditioner_out_ of the Kaldi class become
// two tdnnf_ng handles created once with the component's rank / update-period / history / alpha, nnet-tdnn-component.cc:183-210).
struct NaturalGradient {
  tdnnf_ng *in;
  tdnnf_ng *out;
};

// Backprop :335-431: data part :366-416, then (:418-430) "if (to_update->is_gradient_ || !to_update->use_natural_gradient_)
// UpdateSimple(...) else UpdateNaturalGradient(...)".  ng == nullptr selects UpdateSimple (:433-455); otherwise
// UpdateNaturalGradient :457-626 with the component's preconditioners.  to_update_bias is to_update->bias_params_ (K + Do).
// workspace: tdnnf_tdnn_update_workspace_bytes (simple) / tdnnf_tdnn_update_natural_gradient_workspace_bytes (natural gradient).
template <class CuMat>
inline void TdnnDartsBackprop(const TdnnDartsState &c, const tdnnf_tdnn_indexes &ix, const CuMat &in_value,
                              const CuMat &out_deriv, const float *memo_dev, CuMat *in_deriv /* may be null */,
                              float learning_rate, float *to_update_linear /* null: no update */, float *to_update_bias,
                              void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream, const NaturalGradient *ng = nullptr) {
  tdnnf_mat vdy = View(out_deriv), vx = View(in_value);
  if (in_deriv) {
    tdnnf_mat vdx = View(*in_deriv);
    Check(tdnnf_tdnn_backprop_data(&ix, &vdy, c.linear_params, c.ldw, c.Do, c.Di, memo_dev + c.K, &vdx, stream));
  }
  if (!to_update_linear || learning_rate == 0.0f) return;  // :418-424
  if (ng)
    Check(tdnnf_tdnn_update_natural_gradient(&ix, &vx, &vdy, c.Do, c.Di, c.linear_params, c.ldw, memo_dev, memo_dev + c.K, c.flags,
                                             c.share_index, c.temp_proportion, ng->in, ng->out, learning_rate, to_update_linear, c.ldw,
                                             to_update_bias ? to_update_bias + c.K : nullptr, to_update_bias, workspace_dev,
                                             workspace_bytes, stream));
  else
    Check(tdnnf_tdnn_update_simple(&ix, &vx, &vdy, c.Do, c.Di, memo_dev + c.K, learning_rate, to_update_linear, c.ldw,
                                   to_update_bias ? to_update_bias + c.K : nullptr, workspace_dev, workspace_bytes, stream));
}

// Plain TdnnComponent (UPSTREAM): all coefficients one, bias always added.
template <class CuMat>
inline void TdnnPropagate(const tdnnf_tdnn_indexes &ix, const CuMat &in, const float *linear_params, int ldw, int Do, int Di,
                          const float *bias /* Do or null */, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_tdnn_propagate(&ix, &vin, linear_params, ldw, Do, Di, bias, nullptr, bias ? 1 : 0, &vout, stream));
}
// TdnnComponent::Backprop (UPSTREAM): in_deriv += out_deriv W_i on the tap views, then UpdateSimple or UpdateNaturalGradient
template <class CuMat>
inline void TdnnBackprop(const tdnnf_tdnn_indexes &ix, const CuMat &in_value, const CuMat &out_deriv, const float *linear_params, int ldw,
                         int Do, int Di, CuMat *in_deriv /* may be null */, float learning_rate, float *to_update_linear /* null: no update */,
                         float *to_update_bias /* Do or null */, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream,
                         const NaturalGradient *ng = nullptr) {
  tdnnf_mat vdy = View(out_deriv), vx = View(in_value);
  if (in_deriv) {
    tdnnf_mat vdx = View(*in_deriv);
    Check(tdnnf_tdnn_backprop_data(&ix, &vdy, linear_params, ldw, Do, Di, nullptr, &vdx, stream));
  }
  if (!to_update_linear || learning_rate == 0.0f) return;
  if (ng)
    Check(tdnnf_tdnn_update_natural_gradient(&ix, &vx, &vdy, Do, Di, nullptr, 0, nullptr, nullptr, 0, 0, 1.0f, ng->in, ng->out, learning_rate,
                                             to_update_linear, ldw, to_update_bias, nullptr, workspace_dev, workspace_bytes, stream));
  else
    Check(tdnnf_tdnn_update_simple(&ix, &vx, &vdy, Do, Di, nullptr, learning_rate, to_update_linear, ldw, to_update_bias, workspace_dev,
                                   workspace_bytes, stream));
}

// ---------------------------------------------------------------------------------------------------
// BatchNormComponent (src/nnet3/nnet-normalize-component.cc:401-589).  memo_dev = Memo::mean_uvar_scale (5 x D).
template <class CuMat>
inline void BatchNormPropagate(const CuMat &in, float epsilon, float target_rms, CuMat *out, float *memo_dev, void *ws,
                               size_t ws_bytes, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_batchnorm_propagate(&vin, epsilon, target_rms, &vout, memo_dev, ws, ws_bytes, stream));
}
template <class CuMat>
inline void BatchNormBackprop(const CuMat &out_value, const CuMat &out_deriv, float target_rms, float *memo_dev,
                              CuMat *in_deriv, void *ws, size_t ws_bytes, tdnnf_stream stream) {
  tdnnf_mat vz = View(out_value), vdz = View(out_deriv), vdx = View(*in_deriv);
  Check(tdnnf_batchnorm_backprop(&vz, &vdz, target_rms, memo_dev, &vdx, ws, ws_bytes, stream));
}
// BatchNormTestComponent :843-922 (scale_/offset_ from ComputeDerived :682-715)
template <class CuMat>
inline void BatchNormTestPropagate(const CuMat &in, const float *scale_dev, const float *offset_dev, CuMat *out,
                                   tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_batchnorm_test_propagate(&vin, scale_dev, offset_dev, &vout, stream));
}
template <class CuMat>
inline void BatchNormTestBackprop(const CuMat &out_deriv, const float *scale_dev, CuMat *in_deriv, tdnnf_stream stream) {
  tdnnf_mat vdz = View(out_deriv), vdx = View(*in_deriv);
  Check(tdnnf_batchnorm_test_backprop(&vdz, scale_dev, &vdx, stream));
}

// ---------------------------------------------------------------------------------------------------
// (Gumbel)SoftmaxFlopsComponent (src/nnet3/nnet-simple-component.cc:9968-10020, :10088-10158)
template <class CuMat>
inline void SoftmaxFlopsPropagate(const CuMat &in, const float *gumbel_uniform_dev /* null: plain softmax */,
                                  float temp_proportion, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_softmax_flops_propagate(&vin, gumbel_uniform_dev, temp_proportion, &vout, stream));
}
template <class CuMat>
inline void SoftmaxFlopsBackprop(const CuMat &out_value, CuMat *out_deriv /* mutated, as in the reference */, float scale,
                                 const float *flops_dev, int dim, float temp_proportion, CuMat *in_deriv, tdnnf_stream stream) {
  tdnnf_mat vp = View(out_value), vdp = View(*out_deriv), vdx = View(*in_deriv);
  Check(tdnnf_softmax_flops_backprop(&vp, &vdp, scale, flops_dev, dim, temp_proportion, &vdx, stream));
}

// ---------------------------------------------------------------------------------------------------
// BatchNorm statistics: StoreStats nnet-normalize-component.cc:551-589 (stats_dev = [count, sum[D], sumsq[D]] doubles),
// BatchNormTestComponent::ComputeDerived :682-715
inline void BatchNormStoreStats(const float *memo_dev, int dim, int num_frames, double *stats_dev, tdnnf_stream stream) {
  Check(tdnnf_batchnorm_store_stats(memo_dev, dim, num_frames, stats_dev, stream));
}
inline void BatchNormComputeDerived(const double *stats_dev, int dim, float epsilon, float target_rms, float *scale_dev, float *offset_dev,
                                    tdnnf_stream stream) {
  Check(tdnnf_batchnorm_compute_derived(stats_dev, dim, epsilon, target_rms, scale_dev, offset_dev, stream));
}

// ---------------------------------------------------------------------------------------------------
// OnehotFunctionComponent (nnet-simple-component.cc:9504-9552): Propagate draws ONE uniform and replicates the one-hot row;
// Backprop has no input derivative and (is-updatable=true use-natural-gradient=false) adds lr * colsum(out_deriv) to output_.
template <class CuMat>
inline void OnehotPropagate(const float *uniform_draw_dev, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vout = View(*out);
  Check(tdnnf_onehot_propagate(uniform_draw_dev, &vout, stream));
}
template <class CuMat>
inline void OnehotBackprop(const CuMat &out_deriv, float learning_rate, float *to_update_output, void *ws, size_t ws_bytes, tdnnf_stream stream) {
  tdnnf_mat vd = View(out_deriv);
  Check(tdnnf_onehot_backprop(&vd, learning_rate, to_update_output, ws, ws_bytes, stream));
}
// CopyNComponent :4843-4867 (both directions add)
template <class CuMat>
inline void CopyNPropagate(const CuMat &in, float scale, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_copyn_propagate(&vin, scale, &vout, stream));
}
template <class CuMat>
inline void CopyNBackprop(const CuMat &out_deriv, float scale, CuMat *in_deriv, tdnnf_stream stream) {
  tdnnf_mat vd = View(out_deriv), vdx = View(*in_deriv);
  Check(tdnnf_copyn_backprop(&vd, scale, &vdx, stream));
}
// ConstantFunctionComponent :2602-2642 (the NAS-modified non-natural-gradient branch: output_ += 5 lr colsum(out_deriv))
template <class CuMat>
inline void ConstantFunctionPropagate(const float *output_dev, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vout = View(*out);
  Check(tdnnf_constant_function_propagate(output_dev, &vout, stream));
}
template <class CuMat>
inline void ConstantFunctionBackprop(const CuMat &out_deriv, float learning_rate, float *to_update_output, void *ws, size_t ws_bytes,
                                     tdnnf_stream stream) {
  tdnnf_mat vd = View(out_deriv);
  Check(tdnnf_constant_function_backprop(&vd, learning_rate, to_update_output, ws, ws_bytes, stream));
}
// ElementwiseProductComponent :256-299
template <class CuMat>
inline void ElementwiseProductPropagate(const CuMat &in, int output_dim, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_elementwise_product_propagate(&vin, output_dim, &vout, stream));
}
template <class CuMat>
inline void ElementwiseProductBackprop(const CuMat &in_value, const CuMat &out_deriv, int output_dim, CuMat *in_deriv, tdnnf_stream stream) {
  tdnnf_mat vx = View(in_value), vd = View(out_deriv), vdx = View(*in_deriv);
  Check(tdnnf_elementwise_product_backprop(&vx, &vd, output_dim, &vdx, stream));
}

// ---------------------------------------------------------------------------------------------------
// RectifiedLinearComponent :958-1091.  stats_dev = [count, value_sum[D], deriv_sum[D]] doubles (NonlinearComponent's
// value_sum_ / deriv_sum_ / count_); the caller keeps the reference's coin flips (StoreStats w.p. 1/2 :1084, RepairGradients
// w.p. self_repair probability :1017) and calls Repair / StoreStats accordingly.
template <class CuMat>
inline void ReluPropagate(const CuMat &in, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_relu_propagate(&vin, &vout, stream));
}
template <class CuMat>
inline void ReluBackprop(const CuMat &out_value, const CuMat &out_deriv, CuMat *in_deriv, tdnnf_stream stream) {
  tdnnf_mat vy = View(out_value), vd = View(out_deriv), vdx = View(*in_deriv);
  Check(tdnnf_relu_backprop(&vy, &vd, &vdx, stream));
}
template <class CuMat>
inline void ReluRepairGradients(const double *stats_dev, int dim, float self_repair_scale, float lower, float upper, CuMat *in_deriv,
                                tdnnf_stream stream) {
  tdnnf_mat vdx = View(*in_deriv);
  Check(tdnnf_relu_repair(stats_dev, dim, self_repair_scale, lower, upper, &vdx, stream));
}
template <class CuMat>
inline void ReluStoreStats(const CuMat &out_value, double *stats_dev, void *ws, size_t ws_bytes, tdnnf_stream stream) {
  tdnnf_mat vy = View(out_value);
  Check(tdnnf_relu_store_stats(&vy, stats_dev, ws, ws_bytes, stream));
}

// ---------------------------------------------------------------------------------------------------
// AffineComponent :1235-1279 / NaturalGradientAffineComponent::Update :2980-3024 / LinearComponent :3211-3254 (bias == null)
template <class CuMat>
inline void AffinePropagate(const CuMat &in, const float *linear_params, int ldw, const float *bias /* null: LinearComponent */, int output_dim,
                            CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_affine_propagate(&vin, linear_params, ldw, bias, output_dim, &vout, stream));
}
// Backprop :1253-1279: in_deriv += out_deriv W (kBackpropAdds; may be null), then the update of `to_update` -- UpdateSimple :1246-1251
// when ng == nullptr (is_gradient_ or use-natural-gradient=false), else the natural-gradient Update.
// workspace: tdnnf_tdnn_update_workspace_bytes(Do, Di, 1, rows) / tdnnf_affine_update_natural_gradient_workspace_bytes.
template <class CuMat>
inline void AffineBackprop(const CuMat &in_value, const CuMat &out_deriv, const float *linear_params, int ldw, CuMat *in_deriv,
                           float learning_rate, float *to_update_linear /* null: no update */, float *to_update_bias /* null: Linear */,
                           void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream, const NaturalGradient *ng = nullptr) {
  tdnnf_mat vx = View(in_value), vdy = View(out_deriv);
  if (in_deriv) {  // "add with coefficient 1.0 since property kBackpropAdds is true" (:1264-1269): the one-tap gather form adds
    tdnnf_mat vdx = View(*in_deriv);
    tdnnf_tdnn_indexes ix;
    ix.row_stride = 1;
    ix.num_offsets = 1;
    ix.row_offsets[0] = 0;
    Check(tdnnf_tdnn_backprop_data(&ix, &vdy, linear_params, ldw, vdy.cols, vx.cols, nullptr, &vdx, stream));
  }
  if (!to_update_linear || learning_rate == 0.0f) return;
  if (ng)
    Check(tdnnf_affine_update_natural_gradient(&vx, &vdy, ng->in, ng->out, learning_rate, to_update_linear, ldw, to_update_bias, workspace_dev,
                                               workspace_bytes, stream));
  else
    Check(tdnnf_affine_update_simple(&vx, &vdy, learning_rate, to_update_linear, ldw, to_update_bias, workspace_dev, workspace_bytes, stream));
}

// FixedAffineComponent :3378-3399: out = bias + in W^T; in_deriv += out_deriv W (kBackpropAdds), nothing to update
template <class CuMat>
inline void FixedAffineBackprop(const CuMat &out_deriv, const float *linear_params, int ldw, int input_dim, CuMat *in_deriv, tdnnf_stream stream) {
  if (!in_deriv) return;
  tdnnf_mat vdy = View(out_deriv), vdx = View(*in_deriv);
  tdnnf_tdnn_indexes ix;
  ix.row_stride = 1;
  ix.num_offsets = 1;
  ix.row_offsets[0] = 0;
  Check(tdnnf_tdnn_backprop_data(&ix, &vdy, linear_params, ldw, vdy.cols, input_dim, nullptr, &vdx, stream));
}

// NoOpComponent :437-456: out = in; in_deriv = backprop_scale * out_deriv (in place allowed)
template <class CuMat>
inline void NoOpPropagate(const CuMat &in, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  if (vin.data != vout.data) Check(tdnnf_sum_scaled(&vin, 1.0f, nullptr, 0.f, &vout, stream));
}
template <class CuMat>
inline void NoOpBackprop(const CuMat &out_deriv, float backprop_scale, CuMat *in_deriv, tdnnf_stream stream) {
  tdnnf_mat vd = View(out_deriv), vdx = View(*in_deriv);
  if (vd.data != vdx.data || backprop_scale != 1.0f) Check(tdnnf_sum_scaled(&vd, backprop_scale, nullptr, 0.f, &vdx, stream));
}

// GeneralDropoutComponent (UPSTREAM; factory nnet-component-itf.cc:194, edits nnet-utils.cc:1315): mask_dev = num_seq x dim
// from tdnnf_general_dropout_mask, shared over time (row r uses mask row r % num_seq); Backprop applies the same mask
template <class CuMat>
inline void GeneralDropoutApply(const CuMat &in, const float *mask_dev, int num_seq, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_general_dropout(&vin, mask_dev, num_seq, &vout, stream));
}

// FlopsConstraintComponent :9454-9478: Propagate copies; Backprop: in_deriv = rows of flops * scale / (rows * cols of in_value)
template <class CuMat>
inline void FlopsConstraintBackprop(const float *flops_dev, float scale, const CuMat &in_value, CuMat *in_deriv, tdnnf_stream stream) {
  tdnnf_mat vdx = View(*in_deriv);
  Check(tdnnf_flops_constraint_backprop(flops_dev, scale, in_value.NumRows(), in_value.NumCols(), &vdx, stream));
}

// LogSoftmaxComponent :3607-3632
template <class CuMat>
inline void LogSoftmaxPropagate(const CuMat &in, CuMat *out, tdnnf_stream stream) {
  tdnnf_mat vin = View(in), vout = View(*out);
  Check(tdnnf_log_softmax_propagate(&vin, &vout, stream));
}
template <class CuMat>
inline void LogSoftmaxBackprop(const CuMat &out_value, const CuMat &out_deriv, CuMat *in_deriv, tdnnf_stream stream) {
  tdnnf_mat vy = View(out_value), vd = View(out_deriv), vdx = View(*in_deriv);
  Check(tdnnf_log_softmax_backprop(&vy, &vd, &vdx, stream));
}

// ---------------------------------------------------------------------------------------------------
// chain::ComputeChainObjfAndDeriv (UPSTREAM; what NnetChainTrainer::ProcessOutputs calls).  results_dev: 8 device doubles
// (tdnnf_hip.h); xent_output / xent_deriv may be null.  workspace: tdnnf_chain_workspace_bytes(graph, num_sequences, frames).
template <class CuMat>
inline void ChainObjfAndDeriv(const tdnnf_den_graph *den_graph, const tdnnf_supervision *supervision, const CuMat &nnet_output,
                              const CuMat *xent_output, float leaky_hmm_coefficient, float l2_regularize, float xent_regularize,
                              double *results_dev, CuMat *nnet_output_deriv, CuMat *xent_deriv, void *workspace_dev, size_t workspace_bytes,
                              tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output), vd = View(*nnet_output_deriv), vx, vdx;
  if (xent_output) vx = View(*xent_output);
  if (xent_deriv) vdx = View(*xent_deriv);
  Check(tdnnf_chain_objf_and_deriv(den_graph, supervision, &vy, xent_output ? &vx : nullptr, leaky_hmm_coefficient, l2_regularize,
                                   xent_regularize, results_dev, &vd, xent_deriv ? &vdx : nullptr, workspace_dev, workspace_bytes, stream));
}
// The same call with null derivative pointers (what nnet3-chain-compute-prob and nnet3-chain-combine make): the objective only, nothing
// written but results_dev.  workspace: tdnnf_chain_objf_workspace_bytes(graph, num_sequences, frames) -- no per-frame alpha array.
template <class CuMat>
inline void ChainObjf(const tdnnf_den_graph *den_graph, const tdnnf_supervision *supervision, const CuMat &nnet_output, const CuMat *xent_output,
                      float leaky_hmm_coefficient, float l2_regularize, double *results_dev, void *workspace_dev, size_t workspace_bytes,
                      tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output), vx;
  if (xent_output) vx = View(*xent_output);
  Check(tdnnf_chain_objf(den_graph, supervision, &vy, xent_output ? &vx : nullptr, leaky_hmm_coefficient, l2_regularize, results_dev, workspace_dev,
                         workspace_bytes, stream));
}

// An end-to-end (flat-start) supervision for the two calls above, which take it unchanged: one cyclic, epsilon-free pdf-labelled graph per
// sequence (what Kaldi's Supervision holds as e2e_fsts once its transition-ids are mapped to pdf-ids), host arrays in the numbering of
// tdnnf_supervision_create_e2e (tdnnf_hip.h).  Throws on the argument errors listed there; release with tdnnf_supervision_destroy.
inline tdnnf_supervision *SupervisionCreateE2e(int num_sequences, int frames_per_sequence, int num_pdfs, const int *seq_state_begin,
                                               const int *seq_arc_begin, const int *arc_src, const int *arc_dst, const int *arc_pdf,
                                               const float *arc_logprob, const float *initial_logprob, const float *final_logprob, float weight) {
  tdnnf_supervision *sup = nullptr;
  Check(tdnnf_supervision_create_e2e(num_sequences, frames_per_sequence, num_pdfs, seq_state_begin, seq_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob,
                                     initial_logprob, final_logprob, weight, &sup));
  return sup;
}

// The same supervision, reusable (tdnnf_hip.h, tdnnf_supervision_reserve_e2e): reserved once for the largest minibatch of the run, then
// assigned every minibatch's graphs on the trainer's stream -- no allocation, no device-wide wait per step.  Calls enqueued on `stream`
// before the assign still see the previous minibatch.  Throws on the argument errors and on a minibatch beyond a capacity (the supervision
// then still holds the previous minibatch); release with tdnnf_supervision_destroy.
inline tdnnf_supervision *SupervisionReserveE2e(int max_sequences, int max_frames, int num_pdfs, int max_states, int max_arcs) {
  tdnnf_supervision *sup = nullptr;
  Check(tdnnf_supervision_reserve_e2e(max_sequences, max_frames, num_pdfs, max_states, max_arcs, &sup));
  return sup;
}
inline void SupervisionAssignE2e(tdnnf_supervision *sup, int num_sequences, int frames_per_sequence, const int *seq_state_begin,
                                 const int *seq_arc_begin, const int *arc_src, const int *arc_dst, const int *arc_pdf, const float *arc_logprob,
                                 const float *initial_logprob, const float *final_logprob, float weight, tdnnf_stream stream) {
  Check(tdnnf_supervision_assign_e2e(sup, num_sequences, frames_per_sequence, seq_state_begin, seq_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob,
                                     initial_logprob, final_logprob, weight, stream));
}

// The time-synchronous supervision of regular LF-MMI, reusable (tdnnf_hip.h, tdnnf_supervision_reserve): reserved once for the largest
// minibatch of the run -- max_states and max_arcs are totals over a minibatch -- then assigned every minibatch's arrays (those of
// tdnnf_supervision_create, as the egs readers merge them) on the trainer's stream, where the arc tables are built on the device: no
// allocation, no device-wide wait per step.  Calls enqueued on `stream` before the assign still see the previous minibatch.  Throws on what
// tdnnf_supervision_create refuses and on a minibatch beyond a capacity (the supervision then still holds the previous minibatch); release
// with tdnnf_supervision_destroy.
inline tdnnf_supervision *SupervisionReserve(int max_sequences, int max_frames, int max_states, int max_arcs) {
  tdnnf_supervision *sup = nullptr;
  Check(tdnnf_supervision_reserve(max_sequences, max_frames, max_states, max_arcs, &sup));
  return sup;
}
inline void SupervisionAssign(tdnnf_supervision *sup, int num_sequences, int frames_per_sequence, const int *seq_state_begin, const int *seq_arc_begin,
                              const int *state_time, const float *final_logprob, const int *arc_src, const int *arc_dst, const int *arc_pdf,
                              const float *arc_logprob, float weight, tdnnf_stream stream) {
  Check(tdnnf_supervision_assign(sup, num_sequences, frames_per_sequence, seq_state_begin, seq_arc_begin, state_time, final_logprob, arc_src, arc_dst,
                                 arc_pdf, arc_logprob, weight, stream));
}

// A reusable graph set for the Align* calls below (tdnnf_hip.h, tdnnf_align_graphs_reserve): reserved once for the largest batch -- max_states
// and max_arcs are totals over a batch; num_labels 0: no labels -- then assigned each batch of transcript graphs on `stream`, where the
// tables are built on the device.  arc_label: null exactly for a handle reserved without labels.  Release with tdnnf_align_graphs_destroy.
inline tdnnf_align_graphs *AlignGraphsReserve(int max_graphs, int num_pdfs, int num_labels, int max_states, int max_arcs) {
  tdnnf_align_graphs *graphs = nullptr;
  Check(tdnnf_align_graphs_reserve(max_graphs, num_pdfs, num_labels, max_states, max_arcs, &graphs));
  return graphs;
}
inline void AlignGraphsAssign(tdnnf_align_graphs *graphs, int num_graphs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                              const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob,
                              const float *final_logprob, const int *arc_label, tdnnf_stream stream) {
  Check(tdnnf_align_graphs_assign(graphs, num_graphs, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob, initial_logprob,
                                  final_logprob, arc_label, stream));
}

// Transcript graphs (tdnnf_hip.h, "TRANSCRIPT GRAPHS"): the same two assigns from unit (phone) sequences, the graphs compiled on the
// device.  A unit set is made once from the tree's answers -- per unit, or per (left unit, unit) with context 1, the pdf of the first frame
// and of the later frames, and the transition model's loop and leave log-probabilities; release with tdnnf_unit_set_destroy.  Transcript g
// is the slots [slot_begin[g], slot_begin[g + 1]) of slot_unit / slot_optional (optional: silence that may be skipped).  Throws on a bad
// slot, naming the transcript and the slot, and on a batch beyond a capacity; the handle then still holds its previous batch.
inline tdnnf_unit_set *UnitSetCreate(int num_units, int num_pdfs, int context, const int *entry_pdf, const int *loop_pdf, const float *loop_logprob,
                                     const float *leave_logprob, float take_logprob, float skip_logprob) {
  tdnnf_unit_set *units = nullptr;
  Check(tdnnf_unit_set_create(num_units, num_pdfs, context, entry_pdf, loop_pdf, loop_logprob, leave_logprob, take_logprob, skip_logprob, &units));
  return units;
}
inline void AlignGraphsAssignTranscripts(tdnnf_align_graphs *graphs, const tdnnf_unit_set *units, int num_transcripts, const int *slot_begin,
                                         const int *slot_unit, const int *slot_optional, tdnnf_stream stream) {
  Check(tdnnf_align_graphs_assign_transcripts(graphs, units, num_transcripts, slot_begin, slot_unit, slot_optional, stream));
}
inline void SupervisionAssignE2eTranscripts(tdnnf_supervision *sup, const tdnnf_unit_set *units, int num_sequences, int frames_per_sequence,
                                            const int *slot_begin, const int *slot_unit, const int *slot_optional, float weight,
                                            tdnnf_stream stream) {
  Check(tdnnf_supervision_assign_e2e_transcripts(sup, units, num_sequences, frames_per_sequence, slot_begin, slot_unit, slot_optional, weight, stream));
}

// Pronunciation graphs (tdnnf_hip.h, "PRONUNCIATION GRAPHS"): the same from transcripts whose positions (words) have several
// pronunciations -- the lexicon's alternatives, each a unit sequence with a log-probability.  Transcript g is the positions
// [pos_begin[g], pos_begin[g + 1]) of pos_optional, position P the alternatives [pos_alt_begin[P], pos_alt_begin[P + 1]) of alt_logprob,
// alternative Q the units [alt_unit_begin[Q], alt_unit_begin[Q + 1]) of alt_units.  PronunciationGraphSizes (host only) sizes a reserve;
// either out-pointer may be null.  All three throw on a bad batch, naming the transcript, the position and the alternative, and the two
// assigns on a batch beyond a capacity; the handle then still holds its previous batch.
inline void PronunciationGraphSizes(const tdnnf_unit_set *units, int num_transcripts, const int *pos_begin, const int *pos_optional,
                                    const int *pos_alt_begin, const float *alt_logprob, const int *alt_unit_begin, const int *alt_units,
                                    int *states_out, int *arcs_out) {
  Check(tdnnf_pronunciation_graph_sizes(units, num_transcripts, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units, states_out,
                                        arcs_out));
}
inline void AlignGraphsAssignPronunciations(tdnnf_align_graphs *graphs, const tdnnf_unit_set *units, int num_transcripts, const int *pos_begin,
                                            const int *pos_optional, const int *pos_alt_begin, const float *alt_logprob, const int *alt_unit_begin,
                                            const int *alt_units, tdnnf_stream stream) {
  Check(tdnnf_align_graphs_assign_pronunciations(graphs, units, num_transcripts, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units,
                                                 stream));
}
inline void SupervisionAssignE2ePronunciations(tdnnf_supervision *sup, const tdnnf_unit_set *units, int num_sequences, int frames_per_sequence,
                                               const int *pos_begin, const int *pos_optional, const int *pos_alt_begin, const float *alt_logprob,
                                               const int *alt_unit_begin, const int *alt_units, float weight, tdnnf_stream stream) {
  Check(tdnnf_supervision_assign_e2e_pronunciations(sup, units, num_sequences, frames_per_sequence, pos_begin, pos_optional, pos_alt_begin, alt_logprob,
                                                    alt_unit_begin, alt_units, weight, stream));
}

// Alignment supervisions (tdnnf_hip.h, "ALIGNMENT SUPERVISIONS"): SupervisionAssign from alignments, the lattices of regular LF-MMI -- every
// unit boundary free to move by +-tolerance output frames -- compiled on the device into a supervision of SupervisionReserve.  Sequence s is
// the entries [unit_begin[s], unit_begin[s + 1]) of units / starts: its units (phones, of the unit set) and the output frames they start
// at, the first 0 (an alignment at the frame rate is subsampled by the caller).  AlignmentSupervisionSizes: the states and arcs of every
// sequence's lattice on the host, for the reserve (either out-pointer may be null).  Both throw on a bad alignment, naming the sequence and
// the unit's position; the assign also on a minibatch beyond a capacity, and the supervision then still holds its previous minibatch.
inline void AlignmentSupervisionSizes(const tdnnf_unit_set *units, int num_sequences, int frames_per_sequence, const int *unit_begin,
                                      const int *unit, const int *starts, int tolerance, int *states_out, int *arcs_out) {
  Check(tdnnf_alignment_supervision_sizes(units, num_sequences, frames_per_sequence, unit_begin, unit, starts, tolerance, states_out, arcs_out));
}
inline void SupervisionAssignAlignments(tdnnf_supervision *sup, const tdnnf_unit_set *units, int num_sequences, int frames_per_sequence,
                                        const int *unit_begin, const int *unit, const int *starts, int tolerance, float weight,
                                        tdnnf_stream stream) {
  Check(tdnnf_supervision_assign_alignments(sup, units, num_sequences, frames_per_sequence, unit_begin, unit, starts, tolerance, weight, stream));
}

// Alignment chunks (tdnnf_hip.h, "ALIGNMENT CHUNKS"): the supervisions of fixed-length chunks, what nnet3-chain-get-egs cuts out of an
// utterance's supervision (SupervisionSplitter::GetFrameRange, before its determinisation), compiled on the device from the alignment of the
// WHOLE utterance.  Sequence s is the output frames [chunk_begin[s], chunk_begin[s] + frames_per_sequence) of an utterance of utt_frames[s]
// output frames, whose units and starts are the entries [unit_begin[s], unit_begin[s + 1]) of units / starts; two chunks of one utterance
// repeat its alignment.  AlignmentChunkSupervisionSizes: the states and arcs of every chunk's lattice on the host, for the reserve (either
// out-pointer may be null).  Both throw on a bad alignment or chunk, naming the sequence; the assign also on a minibatch beyond a capacity
// or beyond the reserve's staging (many very short chunks: reserve more states), and the supervision then still holds its previous minibatch.
inline void AlignmentChunkSupervisionSizes(const tdnnf_unit_set *units, int num_sequences, int frames_per_sequence, const int *unit_begin,
                                           const int *unit, const int *starts, const int *utt_frames, const int *chunk_begin, int tolerance,
                                           int *states_out, int *arcs_out) {
  Check(tdnnf_alignment_chunk_supervision_sizes(units, num_sequences, frames_per_sequence, unit_begin, unit, starts, utt_frames, chunk_begin, tolerance,
                                                states_out, arcs_out));
}
inline void SupervisionAssignAlignmentChunks(tdnnf_supervision *sup, const tdnnf_unit_set *units, int num_sequences, int frames_per_sequence,
                                             const int *unit_begin, const int *unit, const int *starts, const int *utt_frames,
                                             const int *chunk_begin, int tolerance, float weight, tdnnf_stream stream) {
  Check(tdnnf_supervision_assign_alignment_chunks(sup, units, num_sequences, frames_per_sequence, unit_begin, unit, starts, utt_frames, chunk_begin,
                                                  tolerance, weight, stream));
}

// Chunk inputs (tdnnf_hip.h, "CHUNK INPUTS"): the features and i-vectors of the same chunks, what nnet3-chain-get-egs cuts out of an
// utterance's feature matrix and nnet3-chain-merge-egs interleaves, gathered on the device from the utterances' matrices stacked row-wise
// (as the inference calls take them).  A handle is created once for the largest minibatch; release with tdnnf_chunk_input_destroy.
// Sequence b is the output frames [chunk_begin[b], chunk_begin[b] + frames_per_sequence) of utterance seq_utt[b]; first_t / num_t: the
// net's input window (tdnnf_net_input_frames).  feats_out: (num_t * num_sequences) x feat_dim, t-major; ivectors / ivectors_out may be
// null for a model without i-vectors (ivector_rows is then not read).  Throws on a bad chunk, naming the sequence, on matrices of another
// shape and on a minibatch beyond the capacity -- before anything is enqueued, the outputs as they were.
inline tdnnf_chunk_input *ChunkInputCreate(int max_sequences) {
  tdnnf_chunk_input *input = nullptr;
  Check(tdnnf_chunk_input_create(max_sequences, &input));
  return input;
}
template <class CuMat>
inline void ChunkInputGather(tdnnf_chunk_input *input, int first_t, int num_t, int frame_subsampling, int frames_per_sequence, int num_sequences,
                             const int *seq_utt, const int *chunk_begin, int frame_shift, int num_utts, const int *frames, const CuMat &feats,
                             const int *ivector_rows, const CuMat *ivectors, int ivector_period, CuMat *feats_out, CuMat *ivectors_out,
                             tdnnf_stream stream) {
  if (!feats_out) TDNNF_ADAPTER_FAIL("tdnnf: ChunkInputGather needs feats_out");
  tdnnf_mat vf = View(feats), vo = View(*feats_out), vi, vio;
  if (ivectors) vi = View(*ivectors);
  if (ivectors_out) vio = View(*ivectors_out);
  Check(tdnnf_chunk_input_gather(input, first_t, num_t, frame_subsampling, frames_per_sequence, num_sequences, seq_utt, chunk_begin, frame_shift, num_utts,
                                 frames, &vf, ivector_rows, ivectors ? &vi : nullptr, ivector_period, &vo, ivectors_out ? &vio : nullptr, stream));
}

// Feature stores (tdnnf_hip.h, "FEATURE STORES"): the utterances' features kept on the device as the CompressedMatrix codes a Kaldi data
// directory holds (CM, what copy-feats --compress=true writes; CM2; CM3) and decoded where they are read, so that a resident training set
// costs what its archive does.  A store is created once for one format (1, 2, 3), one feat_dim and its capacities; release with
// tdnnf_feature_store_destroy.  FeatureStoreAppend takes payloads exactly as CompressedMatrix holds them behind its token (global header
// min / range / rows / cols, format 1: per-column percentiles and column-major bytes) and waits for its copies; utterances are numbered in
// append order.  FeatureStoreExpand writes the decoded rows of the listed utterances stacked in list order -- what InferCompute and
// ChunkInputGather take.  ChunkInputGatherStored is ChunkInputGather with the features decoded out of the store: seq_utt indexes the
// store, the frames are the store's; ivector_rows has one entry an utterance of the store, i-vectors stay float.  All throw on what the
// C entries refuse, by name, the store and the outputs as they were.
inline tdnnf_feature_store *FeatureStoreCreate(int format, int feat_dim, int max_utterances, long long max_frames) {
  tdnnf_feature_store *store = nullptr;
  Check(tdnnf_feature_store_create(format, feat_dim, max_utterances, max_frames, &store));
  return store;
}
inline void FeatureStoreAppend(tdnnf_feature_store *store, int num_items, const tdnnf_feature_payload *items) {
  Check(tdnnf_feature_store_append(store, num_items, items));
}
template <class CuMat>
inline void FeatureStoreExpand(tdnnf_feature_store *store, int num_utts, const int *utts, CuMat *out, tdnnf_stream stream) {
  if (!out) TDNNF_ADAPTER_FAIL("tdnnf: FeatureStoreExpand needs out");
  tdnnf_mat vo = View(*out);
  Check(tdnnf_feature_store_expand(store, num_utts, utts, &vo, stream));
}
template <class CuMat>
inline void ChunkInputGatherStored(tdnnf_chunk_input *input, int first_t, int num_t, int frame_subsampling, int frames_per_sequence, int num_sequences,
                                   const int *seq_utt, const int *chunk_begin, int frame_shift, tdnnf_feature_store *store, const int *ivector_rows,
                                   const CuMat *ivectors, int ivector_period, CuMat *feats_out, CuMat *ivectors_out, tdnnf_stream stream) {
  if (!feats_out) TDNNF_ADAPTER_FAIL("tdnnf: ChunkInputGatherStored needs feats_out");
  tdnnf_mat vo = View(*feats_out), vi, vio;
  if (ivectors) vi = View(*ivectors);
  if (ivectors_out) vio = View(*ivectors_out);
  Check(tdnnf_chunk_input_gather_stored(input, first_t, num_t, frame_subsampling, frames_per_sequence, num_sequences, seq_utt, chunk_begin, frame_shift, store,
                                        ivector_rows, ivectors ? &vi : nullptr, ivector_period, &vo, ivectors_out ? &vio : nullptr, stream));
}

// Best-path alignment (tdnnf_hip.h, "best-path alignment"; what nnet3-align-compiled | ali-to-pdf prints, or the free best path through the
// denominator graph): frame t of utterance u is row utt_row_begin[u] + t * row_stride of nnet_output.  The index arrays are host memory;
// pdf_out_dev: sum(utt_frames) ints, state_out_dev (may be null): sum(utt_frames) + num_utts ints, results_dev: 2 doubles per utterance
// (score, ok).  workspace: tdnnf_align_workspace_bytes(graphs, num_utts, utt_graph, utt_frames).  Option "align_path_checkpoint"
// (tdnnf_set_option; back-pointers of C frames at a time, the same path) governs AlignBestPath and AlignBestPathLabels as "align_form" does:
// the workspace question and the call read it alike.
template <class CuMat>
inline void AlignBestPath(const tdnnf_align_graphs *graphs, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                          int row_stride, const CuMat &nnet_output, float acoustic_scale, int *pdf_out_dev, int *state_out_dev, double *results_dev,
                          void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output);
  Check(tdnnf_align_best_path(graphs, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, &vy, acoustic_scale, pdf_out_dev, state_out_dev,
                              results_dev, workspace_dev, workspace_bytes, stream));
}

// Forward-backward on the same graphs (tdnnf_hip.h, "forward-backward"): logprob and ok flag of every utterance into results_dev (2 doubles
// per utterance) and, with post_out, weight x the per-frame pdf posteriors into columns [0, num_pdfs) of post_out's rows utt_row_begin[u] +
// t * row_stride -- soft alignments, or the flat-start numerator's derivative (GenericNumeratorComputation: deriv = weight * posterior).
// post_out null: the forward recursion alone.  workspace: tdnnf_align_posteriors_workspace_bytes(graphs, num_utts, utt_graph, utt_frames,
// post_out != null).  Option "align_checkpoint" (tdnnf_set_option; alpha of every C-th frame only, the same bits) governs AlignPosteriors,
// AlignPosteriorsCompact, AlignPosteriorsSparse and the label forms below as "align_form" does: the workspace question and the call read
// it, so set it before both.
template <class CuMat>
inline void AlignPosteriors(const tdnnf_align_graphs *graphs, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                            int row_stride, const CuMat &nnet_output, float acoustic_scale, float weight, CuMat *post_out, double *results_dev,
                            void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output), vp;
  if (post_out) vp = View(*post_out);
  Check(tdnnf_align_posteriors(graphs, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, &vy, acoustic_scale, weight,
                               post_out ? &vp : nullptr, results_dev, workspace_dev, workspace_bytes, stream));
}

// The same pass writing the compact layout (tdnnf_hip.h, "compact posteriors"): per utterance frames x D floats, D the distinct pdfs of its
// graph (tdnnf_align_graphs_pdfs), at the offsets of tdnnf_align_posteriors_compact_layout -- the (pdf, posterior) pairs of a Posterior
// without a num_pdfs-wide matrix.  post_compact_dev: device memory of post_compact_elems floats.  workspace:
// tdnnf_align_posteriors_workspace_bytes(graphs, num_utts, utt_graph, utt_frames, 1).
template <class CuMat>
inline void AlignPosteriorsCompact(const tdnnf_align_graphs *graphs, int num_utts, const int *utt_graph, const int *utt_frames,
                                   const int *utt_row_begin, int row_stride, const CuMat &nnet_output, float acoustic_scale, float weight,
                                   float *post_compact_dev, size_t post_compact_elems, double *results_dev, void *workspace_dev,
                                   size_t workspace_bytes, tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output);
  Check(tdnnf_align_posteriors_compact(graphs, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, &vy, acoustic_scale, weight,
                                       post_compact_dev, post_compact_elems, results_dev, workspace_dev, workspace_bytes, stream));
}

// The same pass reduced to what a Posterior holds (tdnnf_hip.h, "sparse posteriors"): per frame the at most max_per_frame (pdf, value)
// pairs with value > min_post, ascending by pdf, in slots [f * max_per_frame, ..) of pdf_out_dev / post_out_dev with their number in
// count_out_dev[f]; frames are numbered utterance after utterance.  results_dev: 4 doubles per utterance (logprob, ok, frames that had more
// candidates than slots, the greatest number of candidates).  workspace: tdnnf_align_posteriors_sparse_workspace_bytes(graphs, num_utts,
// utt_graph, utt_frames, max_per_frame).
template <class CuMat>
inline void AlignPosteriorsSparse(const tdnnf_align_graphs *graphs, int num_utts, const int *utt_graph, const int *utt_frames,
                                  const int *utt_row_begin, int row_stride, const CuMat &nnet_output, float acoustic_scale, float weight,
                                  float min_post, int max_per_frame, int *pdf_out_dev, float *post_out_dev, int *count_out_dev, double *results_dev,
                                  void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output);
  Check(tdnnf_align_posteriors_sparse(graphs, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, &vy, acoustic_scale, weight, min_post,
                                      max_per_frame, pdf_out_dev, post_out_dev, count_out_dev, results_dev, workspace_dev, workspace_bytes, stream));
}

// The labelled entries (tdnnf_hip.h, "best-path alignment" and "label posteriors"), for graphs of tdnnf_align_graphs_create_labelled: a
// caller-defined label per arc -- a transition-id, a phone, a word position.
// AlignBestPath plus, per frame, the label of the arc taken (label_out_dev: sum(utt_frames) ints, with transition-ids as labels what
// nnet3-align-compiled writes) and the caller's index of that arc (arc_out_dev, may be null).  Same workspace.
template <class CuMat>
inline void AlignBestPathLabels(const tdnnf_align_graphs *graphs, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                                int row_stride, const CuMat &nnet_output, float acoustic_scale, int *pdf_out_dev, int *state_out_dev, int *label_out_dev,
                                int *arc_out_dev, double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output);
  Check(tdnnf_align_best_path_labels(graphs, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, &vy, acoustic_scale, pdf_out_dev, state_out_dev,
                                     label_out_dev, arc_out_dev, results_dev, workspace_dev, workspace_bytes, stream));
}

// AlignPosteriorsCompact per label: frames x L floats, L the distinct labels of the utterance's graph (tdnnf_align_graphs_labels), at the
// offsets of tdnnf_align_label_posteriors_compact_layout.  Same workspace.
template <class CuMat>
inline void AlignLabelPosteriorsCompact(const tdnnf_align_graphs *graphs, int num_utts, const int *utt_graph, const int *utt_frames,
                                        const int *utt_row_begin, int row_stride, const CuMat &nnet_output, float acoustic_scale, float weight,
                                        float *post_compact_dev, size_t post_compact_elems, double *results_dev, void *workspace_dev,
                                        size_t workspace_bytes, tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output);
  Check(tdnnf_align_label_posteriors_compact(graphs, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, &vy, acoustic_scale, weight,
                                             post_compact_dev, post_compact_elems, results_dev, workspace_dev, workspace_bytes, stream));
}

// AlignPosteriorsSparse per label: (label, value) pairs -- with transition-ids as labels the pairs of the Posterior that ali-to-post writes.
// workspace: tdnnf_align_label_posteriors_sparse_workspace_bytes(graphs, num_utts, utt_graph, utt_frames, max_per_frame).
template <class CuMat>
inline void AlignLabelPosteriorsSparse(const tdnnf_align_graphs *graphs, int num_utts, const int *utt_graph, const int *utt_frames,
                                       const int *utt_row_begin, int row_stride, const CuMat &nnet_output, float acoustic_scale, float weight,
                                       float min_post, int max_per_frame, int *label_out_dev, float *post_out_dev, int *count_out_dev,
                                       double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  tdnnf_mat vy = View(nnet_output);
  Check(tdnnf_align_label_posteriors_sparse(graphs, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, &vy, acoustic_scale, weight, min_post,
                                            max_per_frame, label_out_dev, post_out_dev, count_out_dev, results_dev, workspace_dev, workspace_bytes,
                                            stream));
}

// ConstrainOrthonormalInternal nnet-utils.cc:914-1032 on a CuMatrixBase with rows <= cols (pass the transpose otherwise, :1068-1075)
template <class CuMat>
inline void ConstrainOrthonormal(float scale, CuMat *M, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  tdnnf_mat vm = View(*M);
  Check(tdnnf_constrain_orthonormal(scale, vm.data, vm.rows, vm.cols, vm.stride, workspace_dev, workspace_bytes, stream));
}

}  // namespace tdnnf_adapter
#endif  // TDNNF_NNET3_ADAPTER_H_
