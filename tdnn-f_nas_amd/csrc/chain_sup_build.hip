// chain_sup_build.hip -- the reusable time-synchronous supervision (include/tdnnf_hip.h): tdnnf_supervision_reserve makes every allocation
// once for four capacities, tdnnf_supervision_assign validates a minibatch on the host (chain_sup_tables.h), stages its raw arrays in pinned
// memory and enqueues the copies and the device build (chain_sup_build_kernels.h) on the caller's stream -- nothing allocated, nothing freed,
// no device-wide wait.  tdnnf_supervision_assign_alignments plans the lattices of a minibatch of alignments on the host (chain_sup_alignment.h),
// stages units and windows and has the compile kernel (chain_sup_compile.hip) write the raw arrays in front of the same build;
// tdnnf_supervision_assign_alignment_chunks does so for chunks of whole-utterance alignments, staging the slice of units each chunk needs.
// tdnnf_supervision_capacity and tdnnf_supervision_dump (created supervisions too) are the diagnostics the tests read.
// The numerator's host functions (chain_num.hip) see an assigned supervision as they see a created one.
#include <string.h>

#include <string>

#include "chain_sup_alignment.h"
#include "chain_sup_build_kernels.h"
#include "chain_sup_tables.h"
#include "chain_types.h"

namespace tdnnf {

struct SupReserved {
  int max_sequences, max_frames, max_states, max_arcs;
  SupBuildDev build;
  AssignStage stage;  // the one allocation (every device array of the supervision, the build's scratch), the staging of the assigns (assign_stage.h)
  int allocs_at_reserve;  // device and pinned allocations made for the handle by the end of reserve
};

namespace {

// Every device array of a reserved supervision at the capacities, out of c.  Run once with a null base for the size.
void sup_reserve_layout(tdnnf_supervision *sp, Carve *c) {
  SupReserved *r = sp->ts;
  const size_t Bc = r->max_sequences, Tc = r->max_frames, Sc = r->max_states, Ac = r->max_arcs;
  SupBuildDev &b = r->build;
  sp->seq_state_begin = c->take<int>(Bc + 1);
  sp->state_time = c->take<int>(Sc);
  sp->final_logprob = c->take<float>(Sc);
  sp->frame_state_begin = c->take<int>(Bc * (Tc + 2));
  sp->in_begin = c->take<int>(Sc + 1);
  sp->in_src = c->take<int>(Ac);
  sp->in_pdf = c->take<int>(Ac);
  sp->in_lp = c->take<float>(Ac);
  sp->out_begin = c->take<int>(Sc + 1);
  sp->out_dst = c->take<int>(Ac);
  sp->out_pdf = c->take<int>(Ac);
  sp->out_lp = c->take<float>(Ac);
  sp->pf_src = c->take<int>(Ac);
  sp->pf_dst = c->take<int>(Ac);
  sp->pf_pdf = c->take<int>(Ac);
  sp->pf_t = c->take<int>(Ac);
  sp->pf_lp = c->take<float>(Ac);
  sp->la_own = c->take<double>(Sc);
  sp->lb_own = c->take<double>(Sc);
  sp->xent_part = c->take<double>(Bc * ((Tc + kNumWideFrames - 1) / kNumWideFrames));
  sp->l2_part = c->take<double>(kFinishL2Parts);
  for (int t = 0; t < 2; t++) {
    b.len[t] = c->take<int>(Sc);
    b.arcpos[t] = c->take<int>(Ac);
  }
  b.out_src = c->take<int>(Ac);
  r->stage.dev = c->take<char>(r->stage.bytes);
  b.cap_states = r->max_states;
  b.cap_arcs = r->max_arcs;
  b.seq_state_begin = sp->seq_state_begin;
  b.frame_state_begin = sp->frame_state_begin;
  b.begin[0] = sp->in_begin;
  b.begin[1] = sp->out_begin;
  b.other[0] = sp->in_src;
  b.other[1] = sp->out_dst;
  b.list_pdf[0] = sp->in_pdf;
  b.list_pdf[1] = sp->out_pdf;
  b.list_lp[0] = reinterpret_cast<int *>(sp->in_lp);
  b.list_lp[1] = reinterpret_cast<int *>(sp->out_lp);
  b.pf_src = sp->pf_src;
  b.pf_dst = sp->pf_dst;
  b.pf_pdf = sp->pf_pdf;
  b.pf_t = sp->pf_t;
  b.pf_lp = reinterpret_cast<int *>(sp->pf_lp);
}

// The two launches of chain_sup_build_kernels.h on s.  b: the handle's tables and scratch with this minibatch's staged arrays, B and T filled in.
int sup_build_launch(const SupBuildDev &b, hipStream_t s) {
  hipLaunchKernelGGL(sup_build_lists_kernel, dim3(b.B, 2), dim3(kBuildThreads), 0, s, b);
  TDNNF_LAUNCH_CHECK();
  hipLaunchKernelGGL(sup_build_frames_kernel, dim3(b.B * b.T), dim3(kSupFrameThreads), 0, s, b);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

// The second half of an assign, behind every refusal: the copies, the compile launch (compile non-null: an assign from alignments), the
// build's launches and the record of the minibatch.  From here on the device tables are being overwritten.  A refusal in front of it left
// the previous minibatch; an error of the runtime in it (a copy or a launch that fails) leaves NO minibatch: the handle is refused like a
// fresh one until an assign succeeds (assign_stage.h).
int sup_commit(tdnnf_supervision *sp, const StagePacker &pk, size_t raw_bytes, const SupCompileDev *compile, const SupPlan &p, int B, int T, float weight,
               hipStream_t s) {
  SupReserved *r = sp->ts;
  const int assigns_before = sp->ts_assigns;
  sp->ts_assigns = 0;
  int rc;
  if ((rc = r->stage.submit(pk, raw_bytes, s)) || (compile && (rc = sup_compile_launch(*compile, s))) || (rc = sup_build_launch(r->build, s))) return rc;

  sp->B = B;
  sp->T = T;
  sp->weight = weight;
  sp->num_states = p.num_states;
  sp->num_arcs = p.num_arcs;
  sp->max_states_per_seq = p.max_states_per_seq;
  sp->max_states_per_frame = p.max_states_per_frame;
  sp->max_arcs_per_frame = p.max_arcs_per_frame;
  sp->wide = p.wide;
  sp->ts_assigns = assigns_before + 1;
  return TDNNF_OK;
}

}  // namespace

void sup_reserved_free(tdnnf_supervision *sp) {
  SupReserved *r = sp->ts;
  if (!r) return;
  r->stage.destroy();
  delete r;
  sp->ts = nullptr;
}

}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_supervision_reserve(int max_sequences, int max_frames, int max_states, int max_arcs, tdnnf_supervision **out) {
  const char *who = "supervision_reserve: ";
  TDNNF_REQUIRE(out && max_sequences > 0 && max_frames > 0 && max_states > 0 && max_arcs >= 0,
                "%sbad arguments (max_sequences %d, max_frames %d, max_states %d, max_arcs %d)", who, max_sequences, max_frames, max_states, max_arcs);
  TDNNF_REQUIRE(max_states >= max_sequences, "%smax_states %d is below max_sequences %d: every sequence has a state", who, max_states, max_sequences);
  // (the build's second launch has a wave per (sequence, frame): 64 * sequences * frames threads, below 2^32)
  TDNNF_REQUIRE((long long)max_sequences * ((long long)max_frames + 2) <= 1ll << 25, "%smax_sequences * (max_frames + 2) must not exceed 2^25", who);
  tdnnf_supervision *sp = new tdnnf_supervision();  // (both zeroed)
  SupReserved *r = new SupReserved();
  sp->ts = r;
  sp->ts_reserved = true;
  r->max_sequences = max_sequences;
  r->max_frames = max_frames;
  r->max_states = max_states;
  r->max_arcs = max_arcs;
  if (int rc = r->stage.create("supervision_reserve: allocation", sup_stage_bytes(max_sequences, max_frames, max_states, max_arcs),
                               [sp](Carve *c) { sup_reserve_layout(sp, c); })) {
    tdnnf_supervision_destroy(sp);
    return rc;
  }
  // (a created supervision's l2_part starts at zero; every reader writes it first)
  if (hipError_t e = hipMemset(sp->l2_part, 0, sizeof(double) * kFinishL2Parts)) {
    tdnnf_supervision_destroy(sp);
    return hip_status(e, "supervision_reserve: hipMemset");
  }
  r->allocs_at_reserve = r->stage.device_allocs + r->stage.pinned_allocs;
  *out = sp;
  return TDNNF_OK;
}

int tdnnf_supervision_assign(tdnnf_supervision *sp, int B, int T, const int *seq_state_begin, const int *seq_arc_begin, const int *state_time,
                             const float *final_logprob, const int *arc_src, const int *arc_dst, const int *arc_pdf, const float *arc_logprob,
                             float weight, tdnnf_stream stream) {
  const char *who = "supervision_assign: ";
  TDNNF_REQUIRE(sp, "%snull supervision", who);
  TDNNF_REQUIRE(sp->kind == 0, "%san end-to-end supervision: tdnnf_supervision_assign_e2e assigns those", who);
  TDNNF_REQUIRE(sp->ts_reserved && sp->ts,
                "%sthe supervision was made by tdnnf_supervision_create: only a supervision of tdnnf_supervision_reserve can be assigned", who);
  SupReserved *r = sp->ts;
  SupPlan p;
  std::string err;
  TDNNF_REQUIRE(sup_validate(who, true, B, T, seq_state_begin, seq_arc_begin, state_time, final_logprob, arc_src, arc_dst, arc_pdf, arc_logprob, &p, &err),
                "%s", err.c_str());
  TDNNF_REQUIRE(sup_check_capacity(who, B, T, p, r->max_sequences, r->max_frames, r->max_states, r->max_arcs, &err), "%s", err.c_str());
  sup_widths(B, T, arc_src, &p);
  const size_t NS = p.num_states, NA = p.num_arcs;

  StagePacker pk;
  if (int rc = r->stage.begin(&pk)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  SupBuildDev &b = r->build;
  const auto raw = [&](const void *v, size_t n) { return reinterpret_cast<const int *>(r->stage.dev + pk.put(v, n)); };
  b.B = B;
  b.T = T;
  b.seq_arc_begin = raw(seq_arc_begin, (size_t)B + 1);
  b.src = raw(arc_src, NA);
  b.dst = raw(arc_dst, NA);
  b.pdf = raw(arc_pdf, NA);
  b.lp_bits = raw(arc_logprob, NA);
  const size_t raw_bytes = pk.at;
  // the arrays that go to the supervision's own device arrays as they are
  pk.put_to(sp->seq_state_begin, seq_state_begin, (size_t)B + 1);
  pk.put_to(sp->state_time, state_time, NS);
  pk.put_to(sp->final_logprob, final_logprob, NS);
  pk.put_to(sp->frame_state_begin, p.frame_state_begin.data(), p.frame_state_begin.size());
  TDNNF_REQUIRE(pk.fits(), "%sinternal: the minibatch needs %zu bytes of staging, the supervision has %zu", who, pk.at, pk.size);
  return sup_commit(sp, pk, raw_bytes, nullptr, p, B, T, weight, s);
}

int tdnnf_alignment_supervision_sizes(const tdnnf_unit_set *units, int B, int T, const int *unit_begin, const int *unit, const int *starts, int tolerance,
                                      int *states_out, int *arcs_out) {
  const char *who = "alignment_supervision_sizes: ";
  TDNNF_REQUIRE(units, "%snull unit set", who);
  std::string err;
  TDNNF_REQUIRE(alignment_sizes(who, units->host, B, T, unit_begin, unit, starts, tolerance, states_out, arcs_out, &err), "%s", err.c_str());
  return TDNNF_OK;
}

int tdnnf_supervision_assign_alignments(tdnnf_supervision *sp, const tdnnf_unit_set *units, int B, int T, const int *unit_begin, const int *unit,
                                        const int *starts, int tolerance, float weight, tdnnf_stream stream) {
  const char *who = "supervision_assign_alignments: ";
  TDNNF_REQUIRE(sp && units, "%snull supervision or null unit set", who);
  TDNNF_REQUIRE(sp->kind == 0, "%san end-to-end supervision: tdnnf_supervision_assign_e2e_transcripts assigns those from unit sequences", who);
  TDNNF_REQUIRE(sp->ts_reserved && sp->ts,
                "%sthe supervision was made by tdnnf_supervision_create: only a supervision of tdnnf_supervision_reserve can be assigned", who);
  SupReserved *r = sp->ts;
  std::string err;
  TDNNF_REQUIRE(alignments_validate(who, units->host, B, T, unit_begin, unit, starts, tolerance, &err), "%s", err.c_str());
  AlignmentSupPlan ap;
  TDNNF_REQUIRE(alignments_plan(who, B, T, unit_begin, starts, tolerance, &ap, &err), "%s", err.c_str());
  const SupPlan &p = ap.plan;
  TDNNF_REQUIRE(sup_check_capacity(who, B, T, p, r->max_sequences, r->max_frames, r->max_states, r->max_arcs, &err), "%s", err.c_str());
  const size_t NA = p.num_arcs, N = unit_begin[B];

  StagePacker pk;
  if (int rc = r->stage.begin(&pk)) return rc;
  SupBuildDev &b = r->build;
  SupCompileDev c;
  const auto raw = [&](const void *v, size_t n) { return reinterpret_cast<const int *>(r->stage.dev + pk.put(v, n)); };
  b.B = c.B = B;
  b.T = c.T = T;
  c.cap_states = r->max_states;
  c.cap_arcs = r->max_arcs;
  b.seq_arc_begin = c.seq_arc_begin = raw(ap.seq_arc_begin.data(), (size_t)B + 1);
  c.slice_begin = raw(unit_begin, (size_t)B + 1);  // (a whole alignment's slice is all its units)
  c.units = raw(unit, N);
  c.lo = raw(ap.lo.data(), N);
  c.hi = raw(ap.hi.data(), N);
  c.chunk = nullptr;
  // the staging's two shapes: on the host the begins, three ints a unit, the supervision's begins and frame_state_begin; on the device the
  // begins and the units, behind them the four arc arrays the kernel writes.  Both fit what tdnnf_supervision_reserve sized for 8 bytes a
  // state, 16 an arc and 4 a (sequence, frame + 2): units <= sequences * frames, units < states, frames <= arcs of a sequence
  const size_t raw_bytes = pk.at, dev_bytes = raw_bytes + 4 * sizeof(int) * NA;
  int *arcs = reinterpret_cast<int *>(r->stage.dev + raw_bytes);  // (device only)
  b.src = c.src = arcs;
  b.dst = c.dst = arcs + NA;
  b.pdf = c.pdf = arcs + 2 * NA;
  b.lp_bits = c.lp_bits = arcs + 3 * NA;
  c.seq_state_begin = sp->seq_state_begin;
  c.frame_state_begin = sp->frame_state_begin;
  c.state_time = sp->state_time;
  c.final_logprob = sp->final_logprob;
  c.frame_arc_begin = b.len[0];
  c.units_dev = units->dev;
  pk.put_to(sp->seq_state_begin, ap.seq_state_begin.data(), (size_t)B + 1);
  pk.put_to(sp->frame_state_begin, p.frame_state_begin.data(), p.frame_state_begin.size());
  TDNNF_REQUIRE(pk.fits() && dev_bytes <= pk.size, "%sinternal: the minibatch needs %zu bytes of staging on the host and %zu on the device, the supervision has %zu",
                who, pk.at, dev_bytes, pk.size);
  return sup_commit(sp, pk, raw_bytes, &c, p, B, T, weight, static_cast<hipStream_t>(stream));
}

int tdnnf_alignment_chunk_supervision_sizes(const tdnnf_unit_set *units, int B, int T, const int *unit_begin, const int *unit, const int *starts,
                                            const int *utt_frames, const int *chunk_begin, int tolerance, int *states_out, int *arcs_out) {
  const char *who = "alignment_chunk_supervision_sizes: ";
  TDNNF_REQUIRE(units, "%snull unit set", who);
  std::string err;
  TDNNF_REQUIRE(alignment_sizes(who, units->host, B, T, unit_begin, unit, starts, tolerance, states_out, arcs_out, &err, true, utt_frames, chunk_begin), "%s",
                err.c_str());
  return TDNNF_OK;
}

int tdnnf_supervision_assign_alignment_chunks(tdnnf_supervision *sp, const tdnnf_unit_set *units, int B, int T, const int *unit_begin, const int *unit,
                                              const int *starts, const int *utt_frames, const int *chunk_begin, int tolerance, float weight,
                                              tdnnf_stream stream) {
  const char *who = "supervision_assign_alignment_chunks: ";
  TDNNF_REQUIRE(sp && units, "%snull supervision or null unit set", who);
  TDNNF_REQUIRE(sp->kind == 0, "%san end-to-end supervision: tdnnf_supervision_assign_e2e_transcripts assigns those from unit sequences", who);
  TDNNF_REQUIRE(sp->ts_reserved && sp->ts,
                "%sthe supervision was made by tdnnf_supervision_create: only a supervision of tdnnf_supervision_reserve can be assigned", who);
  SupReserved *r = sp->ts;
  std::string err;
  TDNNF_REQUIRE(alignments_validate(who, units->host, B, T, unit_begin, unit, starts, tolerance, &err, true, utt_frames, chunk_begin), "%s", err.c_str());
  AlignmentSupPlan ap;
  TDNNF_REQUIRE(alignment_chunks_plan(who, B, T, unit_begin, unit, starts, utt_frames, chunk_begin, tolerance, &ap, &err), "%s", err.c_str());
  const SupPlan &p = ap.plan;
  TDNNF_REQUIRE(sup_check_capacity(who, B, T, p, r->max_sequences, r->max_frames, r->max_states, r->max_arcs, &err), "%s", err.c_str());
  // short chunks may need more staging than the reserve sized (chain_sup_alignment.h)
  TDNNF_REQUIRE(alignment_chunks_fit_staging(who, B, ap, r->stage.bytes, &err), "%s", err.c_str());
  const size_t NA = p.num_arcs, N = ap.lo.size(), raw_ints = alignment_chunks_raw_ints(B, ap);

  StagePacker pk;
  if (int rc = r->stage.begin(&pk)) return rc;
  SupBuildDev &b = r->build;
  SupCompileDev c;
  const auto raw = [&](const void *v, size_t n) { return reinterpret_cast<const int *>(r->stage.dev + pk.put(v, n)); };
  b.B = c.B = B;
  b.T = c.T = T;
  c.cap_states = r->max_states;
  c.cap_arcs = r->max_arcs;
  b.seq_arc_begin = c.seq_arc_begin = raw(ap.seq_arc_begin.data(), (size_t)B + 1);
  c.slice_begin = raw(ap.slice_begin.data(), (size_t)B + 1);
  c.units = raw(ap.units.data(), N);
  c.lo = raw(ap.lo.data(), N);
  c.hi = raw(ap.hi.data(), N);
  c.chunk = raw(ap.chunk.data(), 4 * (size_t)B);
  const size_t raw_bytes = pk.at;
  int *arcs = reinterpret_cast<int *>(r->stage.dev + raw_bytes);  // (device only)
  b.src = c.src = arcs;
  b.dst = c.dst = arcs + NA;
  b.pdf = c.pdf = arcs + 2 * NA;
  b.lp_bits = c.lp_bits = arcs + 3 * NA;
  c.seq_state_begin = sp->seq_state_begin;
  c.frame_state_begin = sp->frame_state_begin;
  c.state_time = sp->state_time;
  c.final_logprob = sp->final_logprob;
  c.frame_arc_begin = b.len[0];
  c.units_dev = units->dev;
  pk.put_to(sp->seq_state_begin, ap.seq_state_begin.data(), (size_t)B + 1);
  pk.put_to(sp->frame_state_begin, p.frame_state_begin.data(), p.frame_state_begin.size());
  TDNNF_REQUIRE(pk.fits() && raw_bytes == sizeof(int) * raw_ints, "%sinternal: the minibatch needs %zu bytes of staging on the host, the supervision has %zu", who,
                pk.at, pk.size);
  return sup_commit(sp, pk, raw_bytes, &c, p, B, T, weight, static_cast<hipStream_t>(stream));
}

int tdnnf_supervision_capacity(const tdnnf_supervision *sp, int *max_sequences, int *max_frames, int *max_states, int *max_arcs, int *assigns,
                               int *allocations_since_reserve, long long *device_bytes) {
  TDNNF_REQUIRE(sp && sp->kind == 0 && sp->ts_reserved && sp->ts,
                "supervision_capacity: null supervision, or one that tdnnf_supervision_reserve did not make (it has no capacity)");
  const SupReserved *r = sp->ts;
  if (max_sequences) *max_sequences = r->max_sequences;
  if (max_frames) *max_frames = r->max_frames;
  if (max_states) *max_states = r->max_states;
  if (max_arcs) *max_arcs = r->max_arcs;
  if (assigns) *assigns = sp->ts_assigns;
  if (allocations_since_reserve) *allocations_since_reserve = r->stage.device_allocs + r->stage.pinned_allocs - r->allocs_at_reserve;
  if (device_bytes) *device_bytes = (long long)r->stage.arena_bytes;
  return TDNNF_OK;
}

int tdnnf_supervision_dump(const tdnnf_supervision *sp, const char *table, void *out, long long capacity, long long *count, tdnnf_stream stream) {
  const char *who = "supervision_dump: ";
  TDNNF_REQUIRE(sp && table && count, "%snull supervision, table name or count", who);
  TDNNF_REQUIRE(sp->kind == 0, "%san end-to-end supervision has none of these tables (tdnnf_align_graphs_dump shows a graph set's)", who);
  if (int rc = sup_need_minibatch(sp, who)) return rc;
  const long long NS = sp->num_states, NA = sp->num_arcs, pf = sp->pf_src ? NA : 0;
  const struct {
    const char *name;
    const void *data;
    long long n;
  } tables[] = {{"seq_state_begin", sp->seq_state_begin, sp->B + 1ll},
                {"state_time", sp->state_time, NS},
                {"final_logprob", sp->final_logprob, NS},
                {"frame_state_begin", sp->frame_state_begin, (long long)sp->B * (sp->T + 2)},
                {"in_begin", sp->in_begin, NS + 1},
                {"in_src", sp->in_src, NA},
                {"in_pdf", sp->in_pdf, NA},
                {"in_lp", sp->in_lp, NA},
                {"out_begin", sp->out_begin, NS + 1},
                {"out_dst", sp->out_dst, NA},
                {"out_pdf", sp->out_pdf, NA},
                {"out_lp", sp->out_lp, NA},
                {"pf_src", sp->pf_src, pf},
                {"pf_dst", sp->pf_dst, pf},
                {"pf_pdf", sp->pf_pdf, pf},
                {"pf_t", sp->pf_t, pf},
                {"pf_lp", sp->pf_lp, pf}};
  for (const auto &t : tables) {
    if (strcmp(t.name, table)) continue;
    *count = t.n;
    if (!out) return TDNNF_OK;
    TDNNF_REQUIRE(capacity >= t.n, "%sout holds %lld elements, table %s has %lld", who, capacity, table, t.n);
    TDNNF_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (sp->ts && sp->ts->stage.last_stream != static_cast<hipStream_t>(stream)) TDNNF_HIP(hipStreamSynchronize(sp->ts->stage.last_stream));
    if (t.n) TDNNF_HIP(hipMemcpy(out, t.data, 4 * (size_t)t.n, hipMemcpyDeviceToHost));
    return TDNNF_OK;
  }
  TDNNF_REQUIRE(false, "%sno table \"%s\" (seq_state_begin, state_time, final_logprob, frame_state_begin, in_begin/src/pdf/lp, out_begin/dst/pdf/lp, pf_src/dst/pdf/t/lp)",
                who, table);
}

}  // extern "C"
