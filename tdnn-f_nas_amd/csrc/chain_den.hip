// chain_den.hip -- host side of the chain objective's denominator: the planner (which form, what workspace), the per-device state of the
// multi-workgroup recursions, the aux stream, and chain_den(), which launches one of three strategies.
// Kernels: den_persistent_kernels.h, den_mw_kernels.h, den_wide_kernels.h.  Graph and supervision: chain_types.h, chain_graph.hip.
#include <algorithm>
#include <initializer_list>

#include "chain_plan.h"
#include "den_mw_kernels.h"
#include "den_persistent_kernels.h"
#include "den_wide_kernels.h"
#include "device.h"
#include "prof.h"

namespace tdnnf {
namespace {

// tdnnf_chain_set_denominator_mode: 0 automatic, 1 persistent, 2 wide, 3 persistent with one workgroup per sequence, 4 persistent with the
// forward recursion, then the one-kernel backward pass on one stream (plan and workspace as mode 1)
int g_den_mode = 0;
// per device (a process may drive several): a time-out on one device says nothing about the others
struct MwDev {
  unsigned *fallbacks = nullptr;  // pinned host memory, written by den_mw_check_kernel
  bool off = false;               // a multi-workgroup launch gave up once on this device: not used again there
};
MwDev g_mw[kMaxDevices];
MwDev *mw_dev() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  return &g_mw[dev];
}
// exchange buffers and counters of the multi-workgroup recursions (den_mw_kernel), behind b_all / S_all in the split region
size_t mw_slots(const tdnnf_den_graph *g) { return (size_t)std::max(g->by_dst.nslices, g->by_src.nslices) * 64; }
size_t mw_extra_floats(const tdnnf_den_graph *g, int B) { return 4 * (size_t)B * mw_slots(g) + 4 * (size_t)B + 64; }

// ---- dynamic LDS, one function per kernel family
// the persistent kernels: the exponentiated output row and `vectors` state vectors (den_forward_kernel 1, FAST 2; den_backward_kernel 3;
// den_beta_kernel 1, FAST 2; den_gamma_kernel 2, den_gamma2_kernel twice that; none with the state vectors in global memory)
size_t den_lds(const tdnnf_den_graph *g, int vectors) { return sizeof(float) * (pad4(g->P) + vectors * pad4(g->H)); }
// den_mw_kernel with G workgroups per sequence: row and one vector, the workgroup's arcs of `tab`, 64 floats of staging per slice it owns
size_t den_mw_lds(const tdnnf_den_graph *g, const tdnnf_den_graph::Sell &tab, int G) {
  const int nsmax = std::max(g->by_dst.nslices, g->by_src.nslices);
  return den_lds(g, 1) + 8 * (size_t)tab.mw_max_arcs[G] + 256 * (size_t)((nsmax + G - 1) / G);
}
template <class Kernel>
hipError_t lds_opt_in(Kernel *kernel, size_t bytes) {  // (on every call, not once per instantiation as opt_in_lds: the sizes depend on the graph)
  return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// FAST kernels (den_forward_kernel) where a thread's rows of every table the launch's FAST kernels walk, and its states, fit its registers
bool den_fast(const tdnnf_den_graph *g, std::initializer_list<const tdnnf_den_graph::Sell *> tables) {
  for (const tdnnf_den_graph::Sell *t : tables)
    if (t->nslices * 64 > kDenFastSlots * kDenThreads) return false;
  return g->H <= kDenFastStates * kDenThreads;
}

ChainPlan chain_plan(const tdnnf_den_graph *g, int B, int T, int num_states_sup) {
  ChainPlan p;
  p.Hs = pad4(g->H);
  p.lds_state = den_lds(g, 3) <= kLdsBudget;
  p.lds_fwd = den_lds(g, p.lds_state ? 1 : 0);
  p.lds_bwd = den_lds(g, p.lds_state ? 3 : 0);
  const int mode = g_den_mode;
  p.wide = mode == 2 || (mode == 0 && !p.lds_state);
  p.split = !p.wide && p.lds_state;
  const int rows = std::max(std::max(g->by_dst.nslices, g->by_src.nslices), g->by_pdf.nslices) * 64;
  p.wide_blocks = (rows / 64 + 3) & ~3;  // partial sums per sequence (at most one per slice), padded to float4
  // 32 sequences per group (a whole 128-byte line per state) unless the minibatch has no more than 16
  p.SG = B > 16 ? 32 : 16;
  p.NG = (B + p.SG - 1) / p.SG;
  const size_t Bw = p.wide ? (size_t)p.NG * p.SG : (size_t)B;  // the wide arrays hold whole groups
  p.alpha_floats = Bw * (T + 1) * p.Hs;
  p.asum_floats = ((size_t)B * (3 * T + 4) + 31) & ~(size_t)31;  // wide: A(0..T), S(0..T) of the backward recursion, Zd(0..T-1)
  // wide: the backward vectors of every frame, two double-buffered sets of partial rows (the recursions run side by side) and x = exp(clamp(y)) /
  // the derivative, sequence-minor (T x P x B)
  p.gstate_floats = p.wide ? Bw * (size_t)(T + 1) * p.Hs + 4 * Bw * p.wide_blocks + (size_t)T * g->P * Bw : (p.lds_state ? (p.split ? (size_t)B * (T + 1) * (p.Hs + 1) + 32 + mw_extra_floats(g, B) : 0) : (size_t)B * 3 * p.Hs);
  p.la_floats = 4 * (size_t)num_states_sup + 2;  // two arrays of DOUBLES (log alpha, log beta of the numerator), 8-byte aligned
  return p;
}

}  // namespace

// workspace layout: [doubles: den_lp[B], num_lp[B], xent[B], l2sum[1]] [alpha] [asum] [la, lb] [gstate]
// (the numerator scratch is sized for up to 4*(T+1) states per sequence on average; a wider supervision brings its own, chain_types.h)
ChainBufs chain_bufs(const tdnnf_den_graph *g, int B, int T, void *ws) {
  ChainBufs b;
  b.p = chain_plan(g, B, T, B * 4 * (T + 1));
  b.den_lp = (double *)ws;
  b.num_lp = b.den_lp + B;
  b.xent = b.num_lp + B;
  b.l2sum = b.xent + B;
  b.alpha = (float *)(((uintptr_t)(b.l2sum + 2) + 127) & ~(uintptr_t)127);  // the wide form gathers 64- / 128-byte runs: keep them in one line
  b.asum = b.alpha + b.p.alpha_floats;
  // the numerator's arrays before the denominator's state region: that one is the workspace's tail, so a caller that never runs the split form
  // (chain_split_region_bytes) can leave it out
  b.la = (double *)(((uintptr_t)(b.asum + b.p.asum_floats) + 7) & ~(uintptr_t)7);
  b.lb = b.la + (b.p.la_floats - 2) / 4;
  b.gstate = (float *)(((uintptr_t)(b.la + b.p.la_floats / 2) + 127) & ~(uintptr_t)127);
  return b;
}

ChainBufs chain_objf_bufs(const tdnnf_den_graph *g, int B, int T, void *ws, size_t *bytes) {
  ChainBufs b;
  b.p = chain_plan(g, B, T, B * 4 * (T + 1));  // (form, Hs, groups and la_floats as the full entry's; the denominator's arrays are this entry's own)
  ChainPlan &p = b.p;
  const size_t Bw = (size_t)p.NG * p.SG;
  p.split = false;
  p.lds_fwd = den_lds(g, p.lds_state ? 2 : 0);
  p.lds_bwd = 0;
  p.alpha_floats = p.wide ? 2 * Bw * p.Hs : 0;
  p.asum_floats = p.wide ? ((size_t)B * (T + 1) + 31) & ~(size_t)31 : 0;
  p.gstate_floats = p.wide ? 2 * Bw * p.wide_blocks + (size_t)T * g->P * Bw : (p.lds_state ? 0 : 2 * (size_t)B * p.Hs);
  uintptr_t at = (uintptr_t)ws;
  auto take = [&at](size_t n, size_t align) {
    at = (at + align - 1) & ~(uintptr_t)(align - 1);
    const uintptr_t r = at;
    at += n;
    return r;
  };
  b.den_lp = (double *)take(sizeof(double) * (3 * (size_t)B + 2 + kObjfL2Parts), 8);
  b.num_lp = b.den_lp + B;
  b.xent = b.num_lp + B;
  b.l2sum = b.xent + B;
  b.l2part = b.l2sum + 2;
  b.la = (double *)take(sizeof(float) * p.la_floats, 8);
  b.lb = b.la + (p.la_floats - 2) / 4;
  b.alpha = (float *)take(sizeof(float) * p.alpha_floats, 128);  // (the wide form gathers 64- / 128-byte runs: whole lines)
  b.asum = (float *)take(sizeof(float) * p.asum_floats, 128);
  b.gstate = (float *)take(sizeof(float) * p.gstate_floats, 128);
  if (bytes) *bytes = (size_t)(at - (uintptr_t)ws) + 3 * 128;  // (three alignments, each may skip up to 127 bytes more under another base address)
  return b;
}

// Bytes at the END of the workspace that only the split persistent form (den_forward beside den_beta, then den_gamma) touches: a caller
// that always passes beside_other_work = true to chain_den may allocate that much less.
size_t chain_split_region_bytes(const tdnnf_den_graph *g, int B, int T) {
  if (!g || B <= 0 || T <= 0) return 0;
  ChainPlan p = chain_plan(g, B, T, B * 4 * (T + 1));
  return p.split ? sizeof(float) * p.gstate_floats : 0;
}

// A second stream for the backward recursion and the fork / join events: one set per DEVICE and calling thread (created on first
// use on that device; a process that drives several devices, or several host threads, gets a set each -- the entry points are
// still not re-entrant for one thread).  They live as long as the process: HIP tears them down with the context.
// The stream is created only when the caller has none to lend (aux == nullptr: events only): a stream holds a share of one of the
// device's four hardware queues for as long as it exists, used or not, and the trainer passes its own.
int den_aux_stream(hipStream_t *aux, hipEvent_t *ev_fork, hipEvent_t *ev_join) {
  struct Set {
    hipStream_t st = nullptr;
    hipEvent_t ef = nullptr, ej = nullptr;
  };
  static thread_local Set sets[kMaxDevices];
  int dev = 0;
  TDNNF_HIP(hipGetDevice(&dev));
  TDNNF_REQUIRE(dev >= 0 && dev < kMaxDevices, "chain: device index %d out of range", dev);
  Set &S = sets[dev];
  if (!S.ef) {
    TDNNF_HIP(hipEventCreateWithFlags(&S.ef, hipEventDisableTiming));
    TDNNF_HIP(hipEventCreateWithFlags(&S.ej, hipEventDisableTiming));
  }
  if (aux && !S.st) TDNNF_HIP(hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking));
  if (aux) *aux = S.st;
  *ev_fork = S.ef;
  *ev_join = S.ej;
  return TDNNF_OK;
}

namespace {

// fork: `to` goes on behind what `from` holds now; the join is the same the other way round, with the other event
int stream_after(hipStream_t to, hipStream_t from, hipEvent_t ev) {
  TDNNF_HIP(hipEventRecord(ev, from));
  TDNNF_HIP(hipStreamWaitEvent(to, ev, 0));
  return TDNNF_OK;
}

// what every strategy of one chain_den() call launches with
struct DenCall {
  const tdnnf_den_graph *g;
  DenDev gd;
  MatView y, deriv;
  int B, T;
  float leaky, deriv_weight;  // (-weight of the supervision)
  ChainBufs b;
  hipStream_t s;
};

// the one-workgroup recursions (the sizes come from the caller, who has opted in: the split form does so for both kernels ahead of both launches)
template <bool LDS_STATE, bool FAST>
void launch_forward(const DenCall &c, size_t lds, const unsigned *only_if, int res_cap) {
  hipLaunchKernelGGL((den_forward_kernel<LDS_STATE, FAST>), dim3(c.B), dim3(kDenThreads), lds, c.s, c.gd, c.y, c.B, c.T, c.leaky, c.b.alpha, c.b.asum, c.b.p.Hs,
                     c.b.den_lp, c.b.gstate, only_if, res_cap);
}
template <bool LDS_STATE>
void launch_backward(const DenCall &c) {
  hipLaunchKernelGGL(den_backward_kernel<LDS_STATE>, dim3(c.B), dim3(kDenThreads), c.b.p.lds_bwd, c.s, c.gd, c.y, c.B, c.T, c.leaky, c.b.alpha, c.b.asum, c.b.p.Hs,
                     c.deriv_weight, c.deriv, c.b.gstate);
}
// the split form's arrays in the workspace tail, and the stream of its backward recursion
struct SplitBufs {
  float *b_all, *S_all;
  hipStream_t aux;
};
template <bool FAST>
void launch_beta(const DenCall &c, const SplitBufs &sb, size_t lds, const unsigned *only_if, int res_cap) {
  hipLaunchKernelGGL(den_beta_kernel<FAST>, dim3(c.B), dim3(kDenThreads), lds, sb.aux, c.gd, c.y, c.B, c.T, c.leaky, sb.b_all, sb.S_all, c.b.p.Hs, only_if, res_cap);
}

// ---------------------------------------------------------------------------------------------- wide
int den_wide(const DenCall &c) {
  const tdnnf_den_graph *g = c.g;
  const ChainBufs &b = c.b;
  const DenDev &gd = c.gd;
  const int B = c.B, T = c.T, Hs = b.p.Hs, P = g->P;
  const float leaky = c.leaky;
  hipStream_t s = c.s;
  const WideDims d{B, b.p.NG, b.p.SG};
  const size_t Bw = (size_t)d.NG * d.SG, frame = Bw * Hs, prow = Bw * b.p.wide_blocks;
  const int nsl = kWideSlices;
  auto blocks = [&](const tdnnf_den_graph::Sell &t) { return (t.nslices + nsl - 1) / nsl; };
  const int nb_dst = blocks(g->by_dst), nb_src = blocks(g->by_src);
  float *alphaT = b.alpha, *asum = b.asum, *S = asum + (size_t)(T + 1) * B, *Zd = S + (size_t)(T + 1) * B;
  float *bT = b.gstate, *part = bT + frame * (T + 1), *part2 = part + 2 * prow, *xT = part2 + 2 * prow;
  const dim3 blk(256), tr((P + 63) / 64, (B + 63) / 64, T), ini(grid_for((long long)frame, 256));
  hipStream_t aux;
  hipEvent_t ev_fork, ev_join;
  int rc = den_aux_stream(&aux, &ev_fork, &ev_join);
  if (rc) return rc;
  hipLaunchKernelGGL(den_wide_prep_kernel, tr, blk, 0, s, c.y, d, P, xT);
  if ((rc = stream_after(aux, s, ev_fork))) return rc;
  // (a template cannot be handed to a function as a kernel name can to a macro: the dispatch on SG written as a function needs a functor
  // per kernel and comes out longer)
#define WIDE_LAUNCH(kernel, ...)                                      \
  do {                                                                \
    if (d.SG == 16) hipLaunchKernelGGL(kernel<16>, __VA_ARGS__);      \
    else hipLaunchKernelGGL(kernel<32>, __VA_ARGS__);                 \
  } while (0)
  // forward recursion (this stream): launch t sums launch t-1's partial rows itself
  hipLaunchKernelGGL(den_wide_init_kernel, ini, blk, 0, s, gd, d, Hs, false, alphaT, asum);
  for (int t = 1; t <= T; t++)
    WIDE_LAUNCH(den_wide_fwd_kernel, dim3(nb_dst * d.NG), blk, 0, s, gd, d, t, leaky, xT, alphaT, asum, Hs,
                t > 1 ? part + (size_t)((t - 1) & 1) * prow : (const float *)nullptr, nb_dst, nsl, part + (size_t)(t & 1) * prow);
  WIDE_LAUNCH(den_wide_sum_kernel, dim3(d.NG), blk, 0, s, part + (size_t)(T & 1) * prow, nb_dst, d, asum + (size_t)T * B);
  hipLaunchKernelGGL(den_wide_total_kernel, dim3((B + 255) / 256), blk, 0, s, gd, B, T, leaky, asum, b.den_lp);
  // backward recursion, self-normalised (the other stream)
  hipLaunchKernelGGL(den_wide_init_kernel, ini, blk, 0, aux, gd, d, Hs, true, bT + (size_t)T * frame, S + (size_t)T * B);
  for (int t = T - 1; t >= 0; t--)
    WIDE_LAUNCH(den_wide_beta_kernel, dim3(nb_src * d.NG), blk, 0, aux, gd, d, t, leaky, xT, bT + (size_t)(t + 1) * frame, S, Hs, bT + (size_t)t * frame,
                t < T - 1 ? part2 + (size_t)((t + 1) & 1) * prow : (const float *)nullptr, nb_src, nsl, part2 + (size_t)(t & 1) * prow);
  WIDE_LAUNCH(den_wide_sum_kernel, dim3(d.NG), blk, 0, aux, part2, nb_src, d, S);
  if ((rc = stream_after(s, aux, ev_join))) return rc;
  // occupancies of every frame at once
  WIDE_LAUNCH(den_wide_dot_kernel, dim3(T, d.NG), blk, 0, s, gd, d, leaky, alphaT, asum, Hs, bT, Zd);
  WIDE_LAUNCH(den_wide_gamma_kernel, dim3(g->by_pdf.nslices * d.NG, T), blk, 0, s, gd, d, leaky, xT, alphaT, asum, Hs, bT, S, Zd, c.deriv_weight);
#undef WIDE_LAUNCH
  hipLaunchKernelGGL(den_wide_unprep_kernel, tr, blk, 0, s, xT, d, P, c.deriv);
  return TDNNF_OK;
}

// ---------------------------------------------------------------------------------------------- split
// Both recursions with several workgroups per sequence, when everything they need holds; *launched says whether (if not, nothing was enqueued).
// Both recursions at once must fit the chip at one workgroup per CU, every workgroup's arcs and state vectors its LDS, and a workgroup owns at
// most 64 slices.
// Four per sequence.  Measured in the step at 1500 x 16 (ms): one 27.3, two 27.5, four 23.8, eight 25.2 -- eight are faster alone (5.0 against
// 5.6 ms for both recursions) but their 256 workgroups hold every CU while the xent head's backward pass wants them; two cost what they gain.
int den_split_mw(const DenCall &c, const SplitBufs &sb, hipEvent_t ev_fork, bool *launched) {
  *launched = false;
  const tdnnf_den_graph *g = c.g;
  const int B = c.B, T = c.T, G = 4;
  MwDev *md = mw_dev();
  if (g_den_mode == 3 || !md || md->off || T < 8) return TDNNF_OK;
  (void)hipGetLastError();
  const int cus = device_cus_known();  // (-1: unknown, the one-workgroup kernels)
  if (cus <= 0 || 2 * B * G > cus) return TDNNF_OK;
  const int ns = std::min(g->by_dst.nslices, g->by_src.nslices), nsmax = std::max(g->by_dst.nslices, g->by_src.nslices);
  if (ns < G || (nsmax + G - 1) / G > 64) return TDNNF_OK;
  const size_t lds_f = den_mw_lds(g, g->by_dst, G), lds_b = den_mw_lds(g, g->by_src, G);
  if (std::max(lds_f, lds_b) > kLdsBudget || g->P > 8 * 960) return TDNNF_OK;  // (den_mw_kernel's row registers: waves 1-15, eight pdfs each)
  if (!md->fallbacks) {  // (first use on this device: the host-visible fallback counter)
    if (hipHostMalloc((void **)&md->fallbacks, sizeof(unsigned), hipHostMallocMapped) != hipSuccess) {
      (void)hipGetLastError();
      md->fallbacks = nullptr;
      return TDNNF_OK;
    }
    *md->fallbacks = 0;
  }
  if (*(volatile unsigned *)md->fallbacks != 0) {
    fprintf(stderr, "tdnnf: the multi-workgroup denominator recursion timed out (its workgroups were not co-resident); the one-workgroup kernels redid the "
                    "minibatch and are used from here on (this device)\n");
    md->off = true;
    return TDNNF_OK;
  }
  // Every workgroup of a recursion polls for its G - 1 partners: the two launches must be resident together.  HIP gives no such guarantee
  // (a CU mask, another process), so ask the occupancy calculator with the actual LDS sizes, and keep the bounded poll as the last resort.
  TDNNF_HIP(lds_opt_in(den_mw_kernel<0>, lds_f));
  TDNNF_HIP(lds_opt_in(den_mw_kernel<1>, lds_b));
  int occ_f = 0, occ_b = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_f, den_mw_kernel<0>, kDenThreads, lds_f) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_b, den_mw_kernel<1>, kDenThreads, lds_b) != hipSuccess || occ_f < 1 || occ_b < 1) {
    (void)hipGetLastError();
    return TDNNF_OK;
  }
  float *mw = sb.S_all + (size_t)B * (T + 1) + 32;
  MwCtl ctl;
  ctl.NSp = (int)mw_slots(g);
  ctl.ctr = reinterpret_cast<unsigned long long *>((reinterpret_cast<uintptr_t>(mw) + 15) & ~(uintptr_t)15);
  ctl.abort_flag = reinterpret_cast<unsigned *>(ctl.ctr + 2 * B);
  ctl.xf = reinterpret_cast<float *>(ctl.ctr + 2 * B + 2);
  ctl.xb = ctl.xf + (size_t)B * 2 * ctl.NSp;
  TDNNF_HIP(hipMemsetAsync(ctl.ctr, 0, sizeof(unsigned long long) * (2 * B + 2), c.s));  // (in front of the fork: both streams see it)
  if (options().den_mw_test_abort) TDNNF_HIP(hipMemsetAsync(ctl.abort_flag, 1, 1, c.s));  // (tests: the recursions give up at their first poll)
  int rc = stream_after(sb.aux, c.s, ev_fork);
  if (rc) return rc;
  hipLaunchKernelGGL(den_mw_kernel<0>, dim3(B * G), dim3(kDenThreads), lds_f, c.s, c.gd, ctl, G, c.y, B, T, c.leaky, c.b.alpha, c.b.asum, c.b.p.Hs, c.b.den_lp);
  hipLaunchKernelGGL(den_mw_kernel<1>, dim3(B * G), dim3(kDenThreads), lds_b, sb.aux, c.gd, ctl, G, c.y, B, T, c.leaky, sb.b_all, sb.S_all, c.b.p.Hs, (double *)nullptr);
  // behind them, the one-workgroup kernels: they return at once unless the abort word is set (then they redo the recursion, so that
  // the occupancy pass never reads half-written vectors and the minibatch is not lost)
  launch_forward<true, false>(c, c.b.p.lds_fwd, (const unsigned *)ctl.abort_flag, 0);
  launch_beta<false>(c, sb, den_lds(g, 1), (const unsigned *)ctl.abort_flag, 0);
  hipLaunchKernelGGL(den_mw_check_kernel, dim3(1), dim3(64), 0, c.s, (const unsigned *)ctl.abort_flag, md->fallbacks);
  *launched = true;
  return TDNNF_OK;
}

// both recursions with one workgroup per sequence; res_f / res_b: arcs of each table that stay in LDS
template <bool FAST>
int den_split_one(const DenCall &c, const SplitBufs &sb, size_t lds_f, size_t lds_b, int res_f, int res_b) {
  TDNNF_HIP(lds_opt_in(den_forward_kernel<true, FAST>, lds_f));
  TDNNF_HIP(lds_opt_in(den_beta_kernel<FAST>, lds_b));
  launch_forward<true, FAST>(c, lds_f, nullptr, res_f);
  launch_beta<FAST>(c, sb, lds_b, nullptr, res_b);
  return TDNNF_OK;
}

// The recursions side by side (the backward one on `aux`), then the occupancies of all frames in one launch
int den_split(const DenCall &c, hipStream_t caller_aux, hipEvent_t ev_recursions, bool *ev_recorded) {
  const tdnnf_den_graph *g = c.g;
  const int B = c.B, T = c.T;
  const size_t lds_beta = den_lds(g, 1), lds_gamma = den_lds(g, 2);
  SplitBufs sb;
  sb.b_all = c.b.gstate;
  sb.S_all = sb.b_all + (size_t)B * (T + 1) * c.b.p.Hs;
  sb.aux = caller_aux;  // a stream the caller has idle (beyond four streams in flight they share hardware queues)
  hipEvent_t ev_fork, ev_join;
  int rc = den_aux_stream(caller_aux ? nullptr : &sb.aux, &ev_fork, &ev_join);
  if (rc) return rc;
  TDNNF_HIP(lds_opt_in(den_forward_kernel<true>, c.b.p.lds_fwd));
  TDNNF_HIP(lds_opt_in(den_beta_kernel<false>, lds_beta));
  if ((rc = stream_after(sb.aux, c.s, ev_fork))) return rc;
  bool mw = false;
  if ((rc = den_split_mw(c, sb, ev_fork, &mw))) return rc;
  if (!mw) {
    // FAST kernels where they apply; and when the two launches hold every CU (one 1024-thread workgroup each), the LDS nothing else can use
    // keeps the tables' widest slices
    const bool fast = den_fast(g, {&g->by_dst, &g->by_src});
    const size_t lf = den_lds(g, fast ? 2 : 1), lb = den_lds(g, fast ? 2 : 1);
    int res_f = 0, res_b = 0;
    const int cus = device_cus_known();  // (-1: unknown)
    if (mw_dev() && cus > 0 && 2 * B >= cus) {
      if (lf < kLdsBudget) res_f = (int)std::min<long long>(g->by_dst.entries, (long long)((kLdsBudget - lf) / 8)) & ~63;
      if (lb < kLdsBudget) res_b = (int)std::min<long long>(g->by_src.entries, (long long)((kLdsBudget - lb) / 8)) & ~63;
    }
    (void)hipGetLastError();
    const size_t lds_f = lf + 8 * (size_t)res_f, lds_b = lb + 8 * (size_t)res_b;
    if ((rc = fast ? den_split_one<true>(c, sb, lds_f, lds_b, res_f, res_b) : den_split_one<false>(c, sb, lds_f, lds_b, res_f, res_b))) return rc;
  }
  if ((rc = stream_after(c.s, sb.aux, ev_join))) return rc;
  if (ev_recursions) {  // both recursions are done here, the occupancies (a launch that fills the chip) come next
    TDNNF_HIP(hipEventRecord(ev_recursions, c.s));
    if (ev_recorded) *ev_recorded = true;
  }
  if (options().den_gamma_pairs != 1 && 2 * lds_gamma + sizeof(float) * kGamma2Threads / 64 <= kLdsBytes) {  // two frames per workgroup
    TDNNF_HIP(lds_opt_in(den_gamma2_kernel, 2 * lds_gamma));
    hipLaunchKernelGGL(den_gamma2_kernel, dim3((T + 1) / 2, B), dim3(kGamma2Threads), 2 * lds_gamma, c.s, c.gd, c.y, B, T, c.leaky, c.b.alpha, sb.b_all, sb.S_all,
                       c.b.p.Hs, c.deriv_weight, c.deriv);
  } else {
    TDNNF_HIP(lds_opt_in(den_gamma_kernel, lds_gamma));
    hipLaunchKernelGGL(den_gamma_kernel, dim3(T, B), dim3(kGammaThreads), lds_gamma, c.s, c.gd, c.y, B, T, c.leaky, c.b.alpha, sb.b_all, sb.S_all, c.b.p.Hs,
                       c.deriv_weight, c.deriv);
  }
  return TDNNF_OK;
}

// ---------------------------------------------------------------------------------------------- objective only
template <bool LDS_STATE, bool FAST>
int den_logprob(const DenCall &c) {
  TDNNF_HIP(lds_opt_in(den_logprob_kernel<LDS_STATE, FAST>, c.b.p.lds_fwd));
  hipLaunchKernelGGL((den_logprob_kernel<LDS_STATE, FAST>), dim3(c.B), dim3(kDenThreads), c.b.p.lds_fwd, c.s, c.gd, c.y, c.B, c.T, c.leaky, c.b.p.Hs, c.b.den_lp,
                     c.b.gstate);
  return TDNNF_OK;
}
// den_wide's forward recursion on two alpha frames, on one stream
int den_wide_logprob(const DenCall &c) {
  const tdnnf_den_graph *g = c.g;
  const ChainBufs &b = c.b;
  const int B = c.B, T = c.T, Hs = b.p.Hs, P = g->P, nsl = kWideSlices;
  const WideDims d{B, b.p.NG, b.p.SG};
  const size_t Bw = (size_t)d.NG * d.SG, frame = Bw * Hs, prow = Bw * b.p.wide_blocks;
  const int nb_dst = (g->by_dst.nslices + nsl - 1) / nsl;
  float *part = b.gstate, *xT = part + 2 * prow;
  const dim3 blk(256), tr((P + 63) / 64, (B + 63) / 64, T), ini(grid_for((long long)frame, 256));
  hipLaunchKernelGGL(den_wide_prep_kernel, tr, blk, 0, c.s, c.y, d, P, xT);
  hipLaunchKernelGGL(den_wide_init_kernel, ini, blk, 0, c.s, c.gd, d, Hs, false, b.alpha, b.asum);
  for (int t = 1; t <= T; t++) {
    const float *part_prev = t > 1 ? part + (size_t)((t - 1) & 1) * prow : nullptr;
    float *part_cur = part + (size_t)(t & 1) * prow;
    if (d.SG == 16) hipLaunchKernelGGL((den_wide_fwd_kernel<16, true>), dim3(nb_dst * d.NG), blk, 0, c.s, c.gd, d, t, c.leaky, xT, b.alpha, b.asum, Hs, part_prev, nb_dst, nsl, part_cur);
    else hipLaunchKernelGGL((den_wide_fwd_kernel<32, true>), dim3(nb_dst * d.NG), blk, 0, c.s, c.gd, d, t, c.leaky, xT, b.alpha, b.asum, Hs, part_prev, nb_dst, nsl, part_cur);
  }
  if (d.SG == 16) hipLaunchKernelGGL(den_wide_sum_kernel<16>, dim3(d.NG), blk, 0, c.s, part + (size_t)(T & 1) * prow, nb_dst, d, b.asum + (size_t)T * B);
  else hipLaunchKernelGGL(den_wide_sum_kernel<32>, dim3(d.NG), blk, 0, c.s, part + (size_t)(T & 1) * prow, nb_dst, d, b.asum + (size_t)T * B);
  hipLaunchKernelGGL(den_wide_total_kernel, dim3((B + 255) / 256), blk, 0, c.s, c.gd, B, T, c.leaky, b.asum, b.den_lp);
  return TDNNF_OK;
}

// ---------------------------------------------------------------------------------------------- serial
template <bool FAST>
int den_serial_forward(const DenCall &c, size_t lds) {
  TDNNF_HIP(lds_opt_in(den_forward_kernel<true, FAST>, lds));
  launch_forward<true, FAST>(c, lds, nullptr, 0);
  return TDNNF_OK;
}
// Forward, then backward with the occupancies, on one stream; the state vectors in LDS where they fit (there the forward kernel may be FAST:
// den_backward_kernel has no such variant, so only the forward table counts)
int den_serial(const DenCall &c) {
  if (!c.b.p.lds_state) {
    launch_forward<false, false>(c, c.b.p.lds_fwd, nullptr, 0);
    launch_backward<false>(c);
    return TDNNF_OK;
  }
  TDNNF_HIP(lds_opt_in(den_backward_kernel<true>, c.b.p.lds_bwd));
  int rc = den_fast(c.g, {&c.g->by_dst}) ? den_serial_forward<true>(c, den_lds(c.g, 2)) : den_serial_forward<false>(c, c.b.p.lds_fwd);
  if (rc) return rc;
  launch_backward<true>(c);
  return TDNNF_OK;
}

}  // namespace

// The three parts of ComputeChainObjfAndDeriv, separately launchable so that the trainer can run the
// denominator (one workgroup per sequence: half the CUs at 128 sequences) on a second stream beside the xent head.
// (1) denominator forward + backward: deriv = -weight * gamma_den (whole matrix overwritten), den log-probs -> workspace
int chain_den(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, float leaky, tdnnf_mat *deriv, void *ws,
              hipStream_t s, bool beside_other_work, hipStream_t caller_aux, hipEvent_t ev_recursions, bool *ev_recorded) {
  if (ev_recorded) *ev_recorded = false;
  const int B = sp->B, T = sp->T;
  const DenCall c{g, den_dev(g), view(y), view(deriv), B, T, leaky, -sp->weight, chain_bufs(g, B, T, ws), s};
  // algorithmic bytes per (frame, sequence): the arcs once per recursion (8 bytes each forward, twice that backward: two arrays), the
  // output row read by both recursions and the derivative row written; the range covers both streams (fork .. join)
  ProfHbmRange prof(6, (double)B * T * (24.0 * g->A + 12.0 * g->P), s);
  int rc;
  if (c.b.p.wide) rc = den_wide(c);  // mode 2, or automatic and the state vectors do not fit the LDS
  else if (c.b.p.split && !beside_other_work && g_den_mode != 4) rc = den_split(c, caller_aux, ev_recursions, ev_recorded);
  else rc = den_serial(c);  // the trainer without option den_split, mode 4, or the state vectors in global memory
  if (rc) return rc;
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

// The denominator of tdnnf_chain_objf: den log-probs -> the objective-only workspace (chain_objf_bufs), nothing else written.  The form follows
// the plan (persistent or wide); the persistent form is always ONE workgroup per sequence, on this stream alone.
int chain_objf_den(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, float leaky, void *ws, hipStream_t s) {
  const int B = sp->B, T = sp->T;
  const DenCall c{g, den_dev(g), view(y), MatView{nullptr, 0, 0, 0}, B, T, leaky, 0.f, chain_objf_bufs(g, B, T, ws), s};
  ProfHbmRange prof(6, (double)B * T * (8.0 * g->A + 4.0 * g->P), s);  // (the arcs once and the output row once per (frame, sequence))
  int rc;
  if (c.b.p.wide) rc = den_wide_logprob(c);
  else if (!c.b.p.lds_state) rc = den_logprob<false, false>(c);
  else rc = den_fast(g, {&g->by_dst}) ? den_logprob<true, true>(c) : den_logprob<true, false>(c);
  if (rc) return rc;
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_chain_set_denominator_mode(int mode) {
  TDNNF_REQUIRE(mode >= 0 && mode <= 4, "chain_set_denominator_mode: 0 automatic, 1 persistent, 2 wide, 3 persistent with one workgroup per sequence, "
                                        "4 persistent, forward then one-kernel backward on one stream");
  g_den_mode = mode;
  return TDNNF_OK;
}

// tests / diagnostics: how many minibatches the one-workgroup kernels redid behind a multi-workgroup launch that gave up, and whether that
// form is switched off for the process; reset != 0 clears both
int tdnnf_chain_den_mw_status(int *fallbacks, int *disabled, int reset) {
  (void)hipDeviceSynchronize();
  MwDev *md = mw_dev();  // (the current device's)
  if (fallbacks) *fallbacks = md && md->fallbacks ? (int)*(volatile unsigned *)md->fallbacks : 0;
  if (disabled) *disabled = md && md->off ? 1 : 0;
  if (reset && md) {
    if (md->fallbacks) *md->fallbacks = 0;
    md->off = false;
  }
  return TDNNF_OK;
}

size_t tdnnf_chain_workspace_bytes(const tdnnf_den_graph *g, int B, int T) {
  if (!g || B <= 0 || T <= 0) return 0;
  ChainPlan p = chain_plan(g, B, T, B * 4 * (T + 1));
  return sizeof(double) * (3 * (size_t)B + 2) + sizeof(float) * (p.alpha_floats + p.asum_floats + p.gstate_floats + p.la_floats) + 768;
}

size_t tdnnf_chain_split_region_bytes(const tdnnf_den_graph *g, int B, int T) { return chain_split_region_bytes(g, B, T); }

size_t tdnnf_chain_objf_workspace_bytes(const tdnnf_den_graph *g, int B, int T) {
  if (!g || B <= 0 || T <= 0) return 0;
  size_t bytes = 0;
  chain_objf_bufs(g, B, T, nullptr, &bytes);
  return bytes;
}

}  // extern "C"
