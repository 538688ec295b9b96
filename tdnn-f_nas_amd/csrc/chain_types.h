// chain_types.h -- what the chain objective's files share: the two opaque handle types of the C ABI and the views of them that the
// kernels take by value.  Built by chain_graph.hip, walked by the denominator (chain_den.hip) and the numerator (chain_num.hip).
//
// LF-MMI objective and derivative on gfx950: chain::ComputeChainObjfAndDeriv,
// DenominatorComputation and NumeratorComputation (UPSTREAM Kaldi, not shipped in the reference;
// reached via /root/reference/steps/nnet3/chain/train.py:515; options pinned by
// local/chain_NAS/run_TDNN_DARTSV3_fbk_stride_pretrain.sh:185-195).  SURVEY.md 8(a) row A7.
//
// MI355X design (vs. upstream's 2*T kernel launches with atomics):
//  * ONE persistent workgroup per sequence walks all T frames inside a single launch; the HMM state
//    vectors (alpha/beta) and the exponentiated output row live in LDS, the per-frame renormaliser
//    is a workgroup reduction.  Sequences are independent, so there is no inter-workgroup traffic.
//  * the denominator graph is stored three times in sliced-ELL (SELL-64) form -- by destination
//    (forward), by source (beta) and by pdf (occupancies) -- so every arc gather is a coalesced
//    stream and every sum is a fixed-order per-thread loop: no float atomics, results are bitwise
//    reproducible.  An arc is 8 bytes: (state | pdf << 16, prob).
//  * the numerator runs in the log domain, in doubles.  A supervision of at most 4 states per frame on average (alignments, the
//    synthetic graphs) takes one wave per sequence on scratch in the caller's workspace (numerator_kernel).  A wider one (lattices
//    with a frame tolerance, any width) takes one workgroup per sequence with the frontier in LDS and a posterior pass spread over
//    (sequence, block of frames) (num_wide_kernels.h); it owns its scratch, so the workspace does not grow with the supervision.
#pragma once
#include "align_tables.h"
#include "common.h"

namespace tdnnf {
struct SupReserved;  // chain_sup_build.hip
}
struct tdnnf_supervision;
namespace tdnnf {
// frees what a reserved time-synchronous supervision holds (tdnnf_supervision_destroy, chain_graph.hip)
__attribute__((visibility("hidden"))) void sup_reserved_free(tdnnf_supervision *sp);
// the refusal every entry gives a reserved supervision of either kind that holds no minibatch (none yet, or an assign failed behind its
// first enqueued copy).  who: the prefix of the message, the call's name (chain_num.hip)
__attribute__((visibility("hidden"))) int sup_need_minibatch(const tdnnf_supervision *sp, const char *who);
}

struct tdnnf_den_graph {
  int H, A, P;
  // SELL-64 over rows sorted by descending degree (so a slice's rows have near-equal degree and padding is
  // negligible): slot s = 64*k + lane holds original row row[s] (0xffffffff = padding slot); its j-th arc is
  // arc[base[k] + j*64 + lane] = (packed key, prob bits), j < (base[k+1]-base[k])/64.
  struct Sell {
    int nrows, nslices;
    int *base;       // nslices + 1 (device)
    unsigned *row;   // nslices * 64
    uint2 *arc;      // key: (other-state-or-src | pdf << 16), or (src | dst << 16) for the by-pdf table
    uint4 *arc4;     // the same arcs as (key, prob, prob * init[key & 0xffff] or 0, 0): what the wide form loads
    long long entries;
    int mw_max_arcs[9];  // [G]: most arc entries any of G workgroups owns when slice k belongs to workgroup k % G (den_*_mw_kernel); G = 2, 4, 8
  } by_dst, by_src, by_pdf;
  float *init;  // H
  float init_sum;
};

struct tdnnf_supervision {
  int B, T;
  int num_states, num_arcs;
  float weight;
  int *seq_state_begin;  // B+1
  int *state_time;
  float *final_logprob;
  // arcs grouped by destination state (forward) and by source state (backward), CSR over global state ids
  int *in_begin, *in_src, *in_pdf;
  float *in_lp;
  int *out_begin, *out_dst, *out_pdf;
  float *out_lp;
  // states of a sequence are sorted by time; frame_state_begin[s*(T+2) + t] = first state with time t
  int *frame_state_begin;
  int max_states_per_seq;
  // ---- what a supervision wider than the workspace's numerator scratch (4 * (T + 1) states per sequence on average) carries; all null /
  // zero for a narrow one, unless it was created under option num_form = 2 (then everything but la_own / lb_own)
  int max_states_per_frame, max_arcs_per_frame;  // widest frame of any sequence; most arcs between two consecutive frames
  bool wide;                                     // num_states > B * 4 * (T + 1)
  double *la_own, *lb_own;                       // num_states doubles each: the numerator's log alpha / log beta (wide only)
  // the arcs that leave frame t of sequence s are [out_begin[fsb[t]], out_begin[fsb[t + 1]]) in the by-source lists; the same range of these
  // holds them ordered by pdf (stable): source state, destination state, pdf, frame, log-prob
  int *pf_src, *pf_dst, *pf_pdf, *pf_t;
  float *pf_lp;
  double *xent_part;  // B * ceil(T / kNumWideFrames) partial xent objectives of the posterior pass
  double *l2_part;    // kFinishL2Parts partial sums of squares of nnet_output (chain_finish's l2 term, summed in order); every supervision has it
  // ---- kind 1 (tdnnf_supervision_create_e2e, chain_num_e2e.hip): one cyclic graph per sequence.  Of the members above it sets B, T, weight,
  // num_states, num_arcs, max_states_per_seq, max_states_per_frame (both the largest graph's state count) and xent_part; wide stays false and
  // the time-synchronous tables null.  All null / zero for kind 0.
  int kind;       // 0 time-synchronous, 1 end-to-end
  int num_pdfs;   // kind 1: the graphs' pdfs are in [0, num_pdfs)
  struct tdnnf_align_graphs *e2e_graphs;  // the arcs by destination, by source and by pdf (align_tables.h); graph s is sequence s's
  double *e2e_alpha, *e2e_beta;           // (T + 1) * num_states doubles each: alpha_t / beta_t of every frame, sequence after sequence
  double *e2e_vecs;                       // 2 * num_states doubles where the two state vectors do not live in LDS, else null
  tdnnf::AlignFormPlan e2e_form;          // the recursion's launch form (align_tables.h), fixed at creation (e2e_vecs depends on it) or planned at every assign
  // ---- kind 1, RESERVED (tdnnf_supervision_reserve_e2e): e2e_graphs is a reserved graph set, the scratch above is sized for the capacities
  // (e2e_vecs always: the launch form follows the assigned batch), and tdnnf_supervision_assign_e2e sets B, T, weight, the totals and
  // e2e_form per minibatch.  All zero for a created supervision.
  bool e2e_reserved;
  int e2e_assigns;                        // 0: no minibatch yet, every entry refuses the supervision
  int e2e_max_sequences, e2e_max_frames;  // the capacities beside the graph set's own
  // ---- kind 0, RESERVED (tdnnf_supervision_reserve, chain_sup_build.hip): every array a time-synchronous supervision can carry -- the
  // pf_* tables, xent_part, la_own / lb_own included -- is a piece of ONE allocation sized for the capacities, and tdnnf_supervision_assign
  // sets B, T, weight, the counts, the widths and `wide` per minibatch and has the tables built on the device.  All zero / null for a created one.
  bool ts_reserved;
  int ts_assigns;              // 0: no minibatch yet, every entry refuses the supervision
  tdnnf::SupReserved *ts;      // the capacities, the allocation, the build's scratch, the staging
};

namespace tdnnf {
namespace {

// what the kernels get of a graph / a supervision, by value
struct DenDev {
  int H, P;
  tdnnf_den_graph::Sell by_dst, by_src, by_pdf;
  const float *init;
  float init_sum;
};
inline DenDev den_dev(const tdnnf_den_graph *g) { return DenDev{g->H, g->P, g->by_dst, g->by_src, g->by_pdf, g->init, g->init_sum}; }

struct SupDev {
  int B, T;
  float weight;
  const int *seq_state_begin, *frame_state_begin;
  const float *final_logprob;
  const int *in_begin, *in_src, *in_pdf;
  const float *in_lp;
  const int *out_begin, *out_dst, *out_pdf;
  const float *out_lp;
};
constexpr int kFinishL2Parts = 256;  // workgroups (of 1024 threads) of chain_finish's sum of squares, one partial sum each
// the posterior pass of the wide numerator: frames per workgroup
constexpr int kNumWideFrames = 8;
struct SupWideDev {
  const int *pf_src, *pf_dst, *pf_pdf, *pf_t;
  const float *pf_lp;
  double *xent_part;
};
inline SupWideDev sup_wide_dev(const tdnnf_supervision *sp) {
  return SupWideDev{sp->pf_src, sp->pf_dst, sp->pf_pdf, sp->pf_t, sp->pf_lp, sp->xent_part};
}
inline SupDev sup_dev(const tdnnf_supervision *sp) {
  return SupDev{sp->B, sp->T, sp->weight, sp->seq_state_begin, sp->frame_state_begin, sp->final_logprob, sp->in_begin, sp->in_src,
                sp->in_pdf, sp->in_lp, sp->out_begin, sp->out_dst, sp->out_pdf, sp->out_lp};
}

}  // namespace
}  // namespace tdnnf
