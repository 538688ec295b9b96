// chain_plan.h -- which form of the denominator a (graph, minibatch) gets and where the chain objective's arrays lie in the caller's
// workspace.  One definition (chain_den.hip) for the denominator and for the numerator (chain_num.hip), which share the workspace.
#pragma once
#include "chain_types.h"

namespace tdnnf {

constexpr size_t kLdsBytes = 160 * 1024;  // per CU (gfx950)
// What the planner lets one workgroup's dynamic LDS grow to.  Nobody wrote down what the 10 KiB below kLdsBytes are for; the kernels' static
// arrays (block_sum's sums, den_mw_kernel's slice offsets) take under 1 KiB of them.
constexpr size_t kLdsBudget = 150 * 1024;

// a row of P or H floats, padded to whole float4 (what the kernels compute as P4 / H4 and get as Hs)
inline int pad4(int n) { return (n + 3) & ~3; }

struct ChainPlan {
  int Hs;
  bool lds_state;
  bool split;         // persistent form with the backward recursion beside the forward one (den_beta_kernel + den_gamma_kernel)
  bool wide;          // den_wide_*: one launch per frame over all sequences, sequence-minor arrays
  int wide_blocks;    // partial rows of the widest launch
  int SG, NG;         // wide: sequences per group, groups
  size_t alpha_floats, asum_floats, gstate_floats, la_floats;
  size_t lds_fwd, lds_bwd;
};

struct ChainBufs {
  ChainPlan p;
  double *den_lp, *num_lp, *xent, *l2sum;
  double *l2part = nullptr;  // objective-only layout: kObjfL2Parts partial sums of the l2 term
  float *alpha, *asum, *gstate;
  double *la, *lb;  // numerator log alpha / log beta
};
// (not part of the library's symbol table: chain_den.hip and chain_num.hip only)
__attribute__((visibility("hidden"))) ChainBufs chain_bufs(const tdnnf_den_graph *g, int B, int T, void *ws);
// The objective-only layout (tdnnf_chain_objf): [doubles: den_lp[B], num_lp[B], xent[B], l2sum[2], l2part[kObjfL2Parts]] [la, lb] and what the
// denominator form of the plan needs for TWO state vectors -- nothing (persistent, vectors in LDS), gstate = 2 Hs floats per sequence
// (persistent, vectors in global memory), or alpha = two frames, asum = the (T + 1) x B normalisers, gstate = two partial rows and xT (wide).
// No per-frame alpha array.  *bytes (optional): what a workspace must hold, alignment slack included.
constexpr int kObjfL2Parts = 32;  // (few: with them and the alignment slack the layout still fits every workspace of tdnnf_chain_workspace_bytes)
__attribute__((visibility("hidden"))) ChainBufs chain_objf_bufs(const tdnnf_den_graph *g, int B, int T, void *ws, size_t *bytes = nullptr);

// The numerator of an end-to-end supervision (kind 1; chain_num_e2e.hip), for the host functions of chain_num.hip.  The recursion leaves
// num_lp[B] and, unless forward_only, alpha / beta of every frame in the supervision's scratch; the posterior pass reads those and adds
// weight * gamma into deriv and / or xent_scale times it into xent_deriv (either may be absent), do_xent: the xent objective -> xent_objf[B].
__attribute__((visibility("hidden"))) int num_e2e_recursion(const tdnnf_supervision *sp, const MatView &y, double *num_lp, bool forward_only, hipStream_t s);
__attribute__((visibility("hidden"))) int num_e2e_posteriors(const tdnnf_supervision *sp, const MatView &y, const MatView &xent_out, const double *num_lp,
                                                             double *xent_objf, const MatView &deriv, const MatView &xent_deriv, float xent_scale, bool do_xent,
                                                             hipStream_t s);

}  // namespace tdnnf
