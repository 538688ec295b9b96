// common.h -- shared helpers of libtdnnf_hip (error reporting, matrix views).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "tdnnf_hip.h"

namespace tdnnf {

struct MatView {
  float *data;
  int rows, cols, stride;
};
inline MatView view(const tdnnf_mat *m) { return MatView{m->data, m->rows, m->cols, m->stride}; }

void set_error(const char *fmt, ...);
int hip_status(hipError_t e, const char *what);

inline bool mat_ok(const tdnnf_mat *m) {
  return m && m->rows >= 0 && m->cols >= 0 && m->stride >= m->cols && (m->data || m->rows * m->cols == 0);
}
inline bool same_dim(const tdnnf_mat *a, const tdnnf_mat *b) { return a->rows == b->rows && a->cols == b->cols; }

inline bool vec4_ok(const MatView &m) {
  return (reinterpret_cast<uintptr_t>(m.data) & 15) == 0 && m.stride % 4 == 0 && m.cols % 4 == 0;
}

#define TDNNF_REQUIRE(cond, ...)            \
  do {                                      \
    if (!(cond)) {                          \
      ::tdnnf::set_error(__VA_ARGS__);      \
      return TDNNF_EINVAL;                  \
    }                                       \
  } while (0)

#define TDNNF_HIP(expr)                                         \
  do {                                                          \
    hipError_t e__ = (expr);                                    \
    if (e__ != hipSuccess) return ::tdnnf::hip_status(e__, #expr); \
  } while (0)

#define TDNNF_LAUNCH_CHECK() TDNNF_HIP(hipGetLastError())

// Tuning options (tdnnf_set_option / tdnnf_get_option, include/tdnnf_hip.h): process-wide integers that select between code paths;
// the library reads no environment variable for them.  What is tested: the GEMM planners' options (gemm_ring, splitk_partial_round,
// splitk_per_cu, gemm_alt_taps, ng_bk, wgrad_small) value by value and element by element, with the launch-form counters
// (launch_forms.h) as the witness of the path that ran (tests/test_gpu_gemm_forms.py); ng_fuse, ng_valu, planes, num_form and
// the test hooks by the tests that name them; den_split and xent_behind_den at 0 and 1 by the trainer test that names them
// (tests/test_gpu_net.py: a small net under den_split x xent_behind_den x wgrad_stream), and den_split 0's kernels stand-alone as
// denominator mode 4 (tests/test_gpu_chain_hostile.py, tests/test_gpu_parity.py).  The trainer's other scheduling options (ng_early_fork,
// wgrad_lag, wgrad_on_caller, ng_pform, ng_early_in, ng_grouped) are tested at their defaults only; reverse_passes at 0 and 3, bit for bit
// against each other with the sweeps' own form counters as the witness (tests/test_gpu_backward_layers.py).  The optimizer step
// behind them (tdnnf_net_update: optim_group.hip, net_update.hip) has no option; tests/test_gpu_net_update.py holds it per component and
// per element to float64: max-change regimes, the orthonormal step's regimes and tile / split-K edges, the tall-matrix path.
struct Options {
  int ng_grouped = 1;     // natural gradient: 1 the side chain of a gradient bucket as grouped launches, 0 per object (read by tdnnf_net_create)
  int ng_fuse = 1;        // output-side statistic H = dY Wy^T: 0 by its own GEMM, 1 inside the BatchNorm / ReLU backward sweep when that pays, 2 always
  int ng_early_in = 1;    // input-side statistics ahead of the backward pass: 0 never, 1 for minibatches without the weight-gradient streams, 2 always (a launch per component), 3 always, with the weight-gradient streams as ONE grouped launch (read by tdnnf_net_create)
  int wgrad_stream = -1;  // parameter gradients on a stream of their own: -1 by minibatch size, 0 off, 1 on (read by tdnnf_net_create)
  int gemm_ring = 1;      // the persistent LDS-DMA-ring form of the rows GEMM where it applies
  int planes = 1;         // gemm_precision 2: the pre-split bf16-plane GEMMs where they apply (0: the in-kernel split everywhere)
  int den_mw_test_abort = 0;  // tests: raise the multi-workgroup denominator's abort word before its launch (the one-workgroup kernels must then redo the minibatch)
  int planes_group = 1;   // f16x3 trainer: the plain components' weight matrices split by ONE grouped pair of launches per step (planes_split_group)
  int planes_check_bound = 0;  // tests: after every split that took its scale from a norm bound, measure the norm and count violations (tdnnf_planes_bound_checks)
  int wgrad_lag = 3;      // trainer, weight-gradient stream on: the caller's stream runs 3 (default) or 1 component(s) ahead of the gradients (read by tdnnf_net_create)
  int wgrad_on_caller = 0;  // trainer: the xent head's weight gradients on the caller's stream when the early statistics occupy the gradient stream
  int splitk_partial_round = 1;  // rows GEMM: split K when the tiles fill only part of one round of resident blocks (rows_gemm.hip launch_rows_balanced)
  int reverse_passes = 0;  // HBM-bound passes walk their matrix from the last rows to the first: bit 0 bn_apply_bypass, bit 1 bn_relu_bwd's apply pass
  int gemm_alt_taps = 1;  // rows GEMM with two taps of one matrix: odd row tiles visit the taps in reverse order, so that both readers of a row block fetch it together
  int splitk_per_cu = 2;  // rows GEMM, few tiles and a long reduction: K slices per CU (2: fill every resident slot; 1: half the partial tiles)
  int wgrad_small = 0;    // weight gradients of launches with at most this many rows on 64 x 64 tiles (0: off)
  int ng_bk = 0;          // natural-gradient statistics passes H = X W^T, longer K steps: bit 0 = 64 instead of 32 for rank <= 32, bit 1 = 32 instead of 16 for rank <= 96
  int ng_early_fork = 1;  // trainer, minibatches without weight-gradient streams: the trunk components' early input statistics start where the trunk's forward pass ends (beside the denominator's recursions) instead of behind the xent head's backward pass
  int xent_behind_den = -1;  // trainer: the xent head's forward pass waits for the denominator's two recursions (their 1024-thread workgroups pin half the CUs): -1 minibatches without weight-gradient streams, 0 never, 1 always; only with den_split on (the one-kernel backward pass has no point between its recursions to wait at)
  int ng_pform = 1;       // natural-gradient statistics of a component whose K taps are row shifts of one matrix (the .linear inputs): one pass over the matrix for all taps' products (ng_stats.hip ng_pform_pass) instead of K
  int ng_valu = 0;        // natural-gradient statistics passes H = X W^T on the vector ALUs (ng_valu.hip) where the rank is 20 / 40 / 80 (measured: no gain, docs/experiments.md r5-n); 0: the MFMA rows GEMM
  int ng_diag_skip = 0;   // diagnostics (timing only, results wrong): skip the statistics passes H = X W^T -- bit 0 two-tap inputs >= 1024 wide, bit 1 every other
  int phase_events = 0;   // diagnostics: the trainer records an event on the caller's stream at every phase boundary of a step (tdnnf_net_phase_times)
  int den_split = -1;     // trainer: the denominator's two recursions side by side (then the occupancies of all frames at once): -1 and 1 always, 0 never (forward recursion, then the one-kernel backward pass, beside the xent head; the workspace is shorter by chain_split_region_bytes); latched at the net's first step
  int num_form = 0;       // the chain numerator: 0 by the supervision's width (numerator_kernel up to 4 states per frame on average, num_wide_kernels.h above), 1 / 2 force one; 2 at tdnnf_supervision_create also gives a narrow supervision the wide form's tables
  int gemm_arith_test = 0;   // tests: 1 / 3 = the stand-alone GEMM entries (no GemmPrecisionScope around them) run the in-kernel split-bf16 kernels bf16x3 / bf16x6 where exact f32 is the default; the exact-f32 scopes (natural gradient, orthonormal constraint) keep f32
  int num_frontier_cap = 0;  // tests: the wide numerator keeps its frontier in global memory for supervisions with a frame of more states than this (0: what the LDS holds)
  int align_form = 0;       // best-path alignment (align.hip; the rules: align_tables.h align_form_plan): 0 the two state vectors in LDS where 2 * S doubles fit kLdsBudget, in the workspace otherwise; 1 / 2 force LDS / workspace (tests/test_gpu_align.py runs both); read by tdnnf_align_workspace_bytes and tdnnf_align_best_path, and alike by forward-backward (align_fb.hip; tests/test_gpu_posteriors.py runs both)
  int align_checkpoint = 0;  // forward-backward with posteriors (align_fb.hip; the rules: align_tables.h align_checkpoint_plan): 0 alpha of every frame stays in the workspace; C >= 1 alpha of every C-th frame, the backward pass recomputes each segment's from its checkpoint (the same bits; tests/test_gpu_posteriors_checkpoint.py); -1 C = ceil(sqrt(the call's longest utterance)); read by tdnnf_align_posteriors_workspace_bytes and by every posterior call alike
  int align_path_checkpoint = 0;  // best-path alignment (align.hip; the rules: align_tables.h align_path_checkpoint_plan): 0 one back-pointer per (frame, state) stays in the workspace; C >= 1 the state scores of every C-th frame and the back-pointers of one segment of C frames, the trace-back recomputes each earlier segment's from its checkpoint (the same path; tests/test_gpu_align_checkpoint.py); -1 C = ceil(sqrt(the call's longest utterance)); read by tdnnf_align_workspace_bytes, tdnnf_align_best_path and tdnnf_align_best_path_labels alike
  int den_gamma_pairs = 0;  // the split form's occupancy pass: 1 one (frame, sequence) per workgroup (den_gamma_kernel), 0 two frames per workgroup where their vectors fit the LDS (den_gamma2_kernel)
};
Options &options();

// Named ranges for profilers (rocprofv3 --marker-trace; the reference's NVTX_RANGE at nnet-normalize-component.cc:185,476 is
// the same idea): roctxRangePush / Pop from librocprofiler-sdk-roctx.so (or libroctx64.so), resolved with dlopen on first use so
// that the library has no link-time dependency on a profiler; without the library (or with TDNNF_ROCTX=0) a range is a no-op.
struct TraceRange {
  explicit TraceRange(const char *name);
  ~TraceRange();
  bool on;
};

// CuMatrix::ApplyFloor semantics: `if (x < floor) x = floor`, so a NaN stays a NaN (fmaxf would swallow it and a
// diverged minibatch would no longer be detected by the objective's finiteness check).
__host__ __device__ inline float floor_keep_nan(float x, float f) { return x < f ? f : x; }

inline int grid_for(long long work, int block, int cap = 2048) {
  long long g = (work + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}
#ifdef __HIPCC__
template <class T>
struct as_given { typedef T type; };
// A grid-stride map over a rows x cols matrix, 256 threads a block: `k4` with a float4 per thread where the caller's predicate `vec`
// holds (every view and column vector it touches allows 16-byte accesses), else `k1` with a float per thread.
template <class... P>
__attribute__((visibility("hidden"))) inline hipError_t launch_vec_or_scalar(bool vec, int rows, int cols, void (*k4)(P...), void (*k1)(P...), hipStream_t s, typename as_given<P>::type... args) {
  const long long work = (long long)rows * (vec ? cols / 4 : cols);
  void (*k)(P...) = vec ? k4 : k1;
  hipLaunchKernelGGL(k, dim3(grid_for(work, 256)), dim3(256), 0, s, args...);
  return hipGetLastError();
}
#endif

// Reproducible stand-in for the reference's RandInt()/RandUniform() control decisions (orthonormal
// schedule nnet-utils.cc:1062, ReLU stats / self-repair coin flips nnet-simple-component.cc:1017,1084):
// splitmix64 of (step, k).  Tests restate it in Python.
inline unsigned long long tdnnf_decision(unsigned long long step, unsigned long long k) {
  unsigned long long z = step * 0x9E3779B97F4A7C15ULL + k * 0xBF58476D1CE4E5B9ULL + 0x94D049BB133111EBULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return (z ^ (z >> 31)) >> 8;
}

// LogSoftmax forward that also leaves aux = aux_scale * softmax(in) (log_softmax.hip); false, nothing launched: not a shape of the one-pass kernel
bool log_softmax_propagate_with_aux(const tdnnf_mat *in, tdnnf_mat *out, tdnnf_mat *aux, float aux_scale, hipStream_t s);
// the three separately launchable parts of the chain objective (chain_den.hip, chain_num.hip)
float chain_supervision_weight(const tdnnf_supervision *sp);
// a supervision of tdnnf_supervision_reserve that holds no minibatch yet (chain_sup_build.hip)
bool chain_supervision_needs_assign(const tdnnf_supervision *sp);
// beside_other_work: the caller runs other kernels next to the denominator (the trainer: the xent head), so the persistent form keeps
// its one-kernel backward pass instead of running the two recursions side by side on a further stream
size_t chain_split_region_bytes(const tdnnf_den_graph *g, int B, int T);
// ev_recursions (optional): recorded on s once both recursions of the side-by-side form are done, in front of the occupancies; *ev_recorded says
// whether this call's form did
int chain_den(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, float leaky, tdnnf_mat *deriv, void *ws, hipStream_t s,
              bool beside_other_work = false, hipStream_t caller_aux = nullptr, hipEvent_t ev_recursions = nullptr, bool *ev_recorded = nullptr);
int chain_num_recursion(const tdnnf_supervision *sp, const tdnnf_den_graph *g, const tdnnf_mat *y, void *ws, hipStream_t s);
int chain_num_xent(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, const tdnnf_mat *xent_output, float xent_regularize,
                   tdnnf_mat *xent_deriv, void *ws, hipStream_t s, bool xent_deriv_initialised = false);
int chain_num(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, const tdnnf_mat *xent_output,
              float xent_regularize, tdnnf_mat *xent_deriv, void *ws, hipStream_t s, bool xent_deriv_initialised = false);
int chain_finish(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, float l2_regularize, double *results,
                 tdnnf_mat *deriv, tdnnf_mat *xent_deriv, void *ws, hipStream_t s);
// the parts of tdnnf_chain_objf (objective only, no derivative; workspace of tdnnf_chain_objf_workspace_bytes, or any larger one): the denominator's
// log-probabilities on s alone, the numerator recursion, the xent objective (xent_output null: zero), and the kernels that finish the objective
int chain_objf_den(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, float leaky, void *ws, hipStream_t s);
int chain_objf_num_recursion(const tdnnf_supervision *sp, const tdnnf_den_graph *g, const tdnnf_mat *y, void *ws, hipStream_t s);
int chain_objf_num_xent(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, const tdnnf_mat *xent_output, void *ws, hipStream_t s);
int chain_objf_finish(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, float l2_regularize, double *results, void *ws, hipStream_t s);

// trainer-internal variants of the TDNN entry points (abi_tdnn.hip); tdnn_rows_ok: `in` has the rows the taps read for N output rows
bool tdnn_rows_ok(const tdnnf_tdnn_indexes *ix, int rows_in, int N);
int tdnn_propagate_impl(const tdnnf_tdnn_indexes *ix, const tdnnf_mat *in, const float *W, int ldw, int Do, int Di,
                        const float *bias, const float *eff_coef, int init_mode, int relu, tdnnf_mat *out, tdnnf_stream stream,
                        float *colstats = nullptr, int *colstats_rows = nullptr);
int tdnn_update_simple_impl(const tdnnf_tdnn_indexes *ix, const tdnnf_mat *in_value, const tdnnf_mat *out_deriv, int Do, int Di,
                            const float *eff_coef, float lr, float *W_acc, int ldw, float *bias_acc, void *ws, size_t ws_bytes,
                            const int *active_dev, int max_active, tdnnf_stream stream, bool overwrite = false);
int tdnn_backprop_data_impl(const tdnnf_tdnn_indexes *ix, const tdnnf_mat *out_deriv, const float *W, int ldw, int Do, int Di,
                            const float *eff_coef, int overwrite, const tdnnf_mat *add, float add_scale, int add_lo,
                            tdnnf_mat *in_deriv, tdnnf_stream stream);

}  // namespace tdnnf
