// net_step_planes.hip -- the plane operands of a step (Step, net_step.h; planes_gemm.h): every matrix that is a GEMM operand has a slot, keyed by its
// base pointer (tdnnf_net::plane_slots); the step splits an operand where it is produced -- or has the pass that produces it write the planes --
// and hands the description to the GEMM as a hint.  Also the weights' planes and W^T of the split-bf16 arithmetic, formed once per step.
#include "net_step.h"

namespace tdnnf {
namespace {
// paramsT[begin_c + col * rows + row] = params[begin_c + row * cols + col] for every component c (blockIdx.y)
struct TransTable {
  long long begin[128];
  int rows[128], cols[128];
};
__global__ __launch_bounds__(256) void transpose_weights_kernel(const float *params, float *paramsT, TransTable tb) {
  const int c = blockIdx.y, rows = tb.rows[c], cols = tb.cols[c];
  const float *W = params + tb.begin[c];
  float *WT = paramsT + tb.begin[c];
  const long long total = (long long)rows * cols;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int col = (int)(e / rows), row = (int)(e % rows);  // consecutive threads: consecutive rows of one column -> coalesced writes
    WT[e] = W[(long long)row * cols + col];
  }
}
}  // namespace

// ---------------------------------------------------------------- plane operands
// the slot of `m` (null: none -- the GEMM runs its own kernels)
tdnnf_net::PlaneSlot *Step::slot_of(const tdnnf_mat &m) const {
  auto it = n->plane_slots.find(m.data);
  return it == n->plane_slots.end() ? nullptr : &it->second;
}
// What every writer of planes into a slot opens with.  `lead` zero rows in front of the matrix go up to a multiple of 16 (a weight gradient
// reads the row-major planes in K steps of 16 rows: the matrix starts on one).  The slot was allocated (net_arena.hip, by planes_gemm.h's
// planes_slot_* sizes) for planes of `m` with R rows, and transposed planes with Rt rows (0: none are written): anything larger would be
// written past its end.  *same: whether `ps` last held exactly this split -- (rows, cols, lead, R, layouts): the same again leaves the zero rows
// as they are -- and the record of it.  *o: the row-major planes of `m` in the slot, as a GEMM hint.
int Step::slot_use(tdnnf_net::PlaneSlot &ps, const tdnnf_mat &m, int lead, long long Rt, int layouts, PlanesOperand *o, bool *same) const {
  lead = (lead + 15) & ~15;
  const long long R = planes_slot_rows(m.rows, lead), kb_alloc = planes_slot_kblocks(m.cols);
  TDNNF_REQUIRE(planes_bytes(np, R, kb_alloc) <= ps.bytesP && planes_bytes(np, Rt, planes_t_kblocks(m.rows)) <= ps.bytesPT,
                "net_forward_backward: plane slot too small for a %d x %d matrix", m.rows, m.cols);
  const long long cfg5[5] = {m.rows, m.cols, lead, R, layouts};
  *same = memcmp(cfg5, ps.last, sizeof(cfg5)) == 0;
  memcpy(ps.last, cfg5, sizeof(cfg5));
  *o = PlanesOperand();
  o->base = m.data; o->rows = m.rows; o->cols = m.cols; o->ld = m.stride; o->np = np;
  o->P = ps.P; o->R = R; o->lead = lead; o->kb_alloc = kb_alloc; o->scale = np == 2 ? ps.scale : nullptr;
  return TDNNF_OK;
}
int Step::split(const tdnnf_mat &m, int lead, int want, PlanesOperand *o, hipStream_t st, const FroBound &fb) {
  *o = PlanesOperand();
  if (!pl_on) return TDNNF_OK;
  tdnnf_net::PlaneSlot *ps = slot_of(m);
  if (!ps || m.rows <= 0) return TDNNF_OK;
  // a wide matrix (the 1536- / 6034-column activations and derivatives) is the tile-row operand of its weight gradient, which reads
  // the ROW-MAJOR planes through transposing LDS loads: no planes of the transpose for those
  if (m.cols >= 1024) want = kP;
  PlanesSplitArgs a;
  a.np = np; a.x = view(&m); a.scale = ps->scale; a.sumsq_ws = n->planes_ws;
  if (np == 2 && fb.blocks > 0 && (fb.add_coef == 0.f || fb.add_rec)) {
    a.fro2_bound = n->fro_buf; a.fro2_blocks = fb.blocks; a.fro_mul = fb.mul; a.add_coef = fb.add_coef; a.add_rec = fb.add_rec;
  }
  a.Rt = planes_slot_t_rows(m.cols);
  CK(slot_use(*ps, m, lead, a.Rt, want, o, &a.pads_done));
  a.lead = o->lead;
  a.R = o->R;
  a.P = (want & kP) ? ps->P : nullptr;
  a.PT = (want & kT) ? ps->PT : nullptr;
  TDNNF_HIP(planes_split(a, st));
  o->P = a.P; o->PT = a.PT; o->Rt = a.Rt;
  return TDNNF_OK;
}
// the planes of `m`, the matrix the last bn_apply_planes wrote: its own (po_next), or a split with the norm bound it left (fb_next)
int Step::next_input_planes(const tdnnf_mat &m, PlanesOperand *o) {
  if (po_next.base != m.data || po_next.rows != m.rows) return split(m, 0, kP | kT, o, s, fb_next);
  *o = po_next;
  return TDNNF_OK;
}
// a component's weight matrix as planes (row-major: forward; transposed: backward-data); coef: a TdnnDARTSV3Component's effective tap
// coefficients (device, one per `period` columns), folded into the planes so that its GEMMs need none
// (`group`: collect the split instead of launching it -- the plain components' weights of a step go as ONE grouped pair of launches)
int Step::split_weights(int comp, const float *coef, int period, bool group) {
  PlanesOperand &o = n->pw[comp];
  if (!o.P) return TDNNF_OK;
  o.base = net_W(n, comp);
  o.coef = coef;
  o.coef_period = period;
  PlanesSplitArgs a;
  a.np = np; a.x = MatView{net_W(n, comp), o.rows, o.cols, o.cols}; a.lead = 0; a.R = o.R; a.P = const_cast<void *>(o.P); a.Rt = o.Rt;
  a.PT = const_cast<void *>(o.PT); a.scale = n->pw_scale[comp]; a.sumsq_ws = n->planes_ws;
  a.col_coef = coef; a.col_coef_period = period;
  o.scale = np == 2 ? n->pw_scale[comp] : nullptr;
  a.pads_done = n->fb_count > 1;  // (fixed shapes: the zero rows written by the first step stay)
  if (group && options().planes_group && planes_split_group_ok(a)) wsplits.push_back(a);
  else TDNNF_HIP(planes_split(a, s));
  return TDNNF_OK;
}
// where the fused BatchNorm / ReLU backward sweep may write the f16 planes of the derivative matrix `d` it produces (f16x3, 1536-wide
// matrices with a slot): fills *bp for bn_relu_bwd and *po for the GEMMs that read `d` next; bp->P == null: not fused, split afterwards
int Step::bwd_planes(const tdnnf_mat &d, int lead, BwdPlanes *bp, PlanesOperand *po) {
  *bp = BwdPlanes{nullptr, 0, 0, nullptr};
  *po = PlanesOperand();
  if (!(pl_on && np == 2 && d.cols % 16 == 0 && d.cols >= 1024)) return TDNNF_OK;
  tdnnf_net::PlaneSlot *ps = slot_of(d);
  if (!ps) return TDNNF_OK;
  bool same = false;
  CK(slot_use(*ps, d, lead, 0, kP, po, &same));
  if (!same) TDNNF_HIP(planes_pad(np, ps->P, planes_kblocks(d.cols), po->R, po->lead, d.rows, s));
  *bp = BwdPlanes{ps->P, po->R, po->lead, ps->scale};
  return TDNNF_OK;
}
// bn_apply_bypass that ALSO writes its output as f16 planes when the BatchNorm finalize left a norm bound (f16x3, plain views): the
// scale record first (from the bound), then one pass writes the f32 matrix and its row-major planes -- the GEMM that reads `out`
// next needs no split pass.  *po describes the planes (empty: not fused, the consumer splits).
int Step::bn_apply_planes(const tdnnf_mat &x, const float *memo, const MatView &byp, float bypass, const tdnnf_mat &out, const float *mask, const FroBound &fb,
                          PlanesOperand *po) {
  *po = PlanesOperand();
  const bool fused = pl_on && np == 2 && fb.blocks > 0 && (fb.add_coef == 0.f || fb.add_rec) && out.cols == Hd && out.stride == ldpad(Hd);
  tdnnf_net::PlaneSlot *ps = fused ? slot_of(out) : nullptr;
  if (!ps) {
    TDNNF_HIP(bn_apply_bypass(view(&x), memo, Hd, ldpad(Hd), byp, bypass, view(&out), s, mask, B));
    return TDNNF_OK;
  }
  const bool held = ps->last[0] >= 0;
  bool same = false;
  CK(slot_use(*ps, out, 0, 0, kP, po, &same));
  TDNNF_HIP(planes_scale_bound(n->fro_buf, fb.blocks, (double)out.rows * out.cols, fb.mul, fb.add_coef, fb.add_rec, ps->scale, s));
  if (!same && held) {  // (the slot last held another shape: zero rows behind the matrix again)
    TDNNF_HIP(planes_pad(np, ps->P, planes_kblocks(out.cols), po->R, 0, out.rows, s));
  }
  const PlanesSink sink{ps->P, po->R, ps->scale};
  TDNNF_HIP(bn_apply_bypass(view(&x), memo, Hd, ldpad(Hd), byp, bypass, view(&out), s, mask, B, &sink));
  if (options().planes_check_bound) TDNNF_HIP(planes_check_bound(view(&out), ps->scale, n->planes_ws, s));
  return TDNNF_OK;
}
// this step's weights as planes (the DARTS components' again in the layer loop, once their coefficients are formed)
int Step::weight_planes() {
  if (!pl_on) return TDNNF_OK;
  // 36 components x (norm pass + split) were 72 launches of 6 - 12 us, serial on the caller's stream with nothing else in flight: two launches now
  for (size_t i = 0; i < n->comps.size(); i++)
    if (n->comps[i].num_alpha == 0 || n->comps[i].plain) CK(split_weights((int)i, nullptr, 0, true));
  // the TdnnDARTSV3Components' too: their tap coefficients depend on the architecture logits and this step's draws only, so they are formed
  // here, ahead of the layer loop, and the coefficient-folded weight planes join the same two launches
  if (options().planes_group && n->draws) {
    for (auto &L : n->layers) {
      if (!L.lin.darts) continue;
      CK(darts_coef(n, L, s));
      CK(split_weights(L.lin.comp, darts_eff(L.lin), c.hidden_dim, true));
      CK(split_weights(L.aff.comp, darts_eff(L.aff), L.bn, true));
    }
    darts_coef_done = true;
  }
  TDNNF_HIP(planes_split_group(wsplits, &n->wsplit_group, s));
  return TDNNF_OK;
}
int Step::transpose_weights() {
  if (n->paramsT) {  // split-bf16 backward-data GEMMs read W^T (k-contiguous B operand)
    TransTable tb;
    memset(&tb, 0, sizeof(tb));
    const int nc = (int)n->comps.size();
    for (int i = 0; i < nc; i++) {
      tb.begin[i] = n->comps[i].begin;
      tb.rows[i] = n->comps[i].rows;
      tb.cols[i] = n->comps[i].cols;
    }
    hipLaunchKernelGGL(transpose_weights_kernel, dim3(256, nc), dim3(256), 0, s, n->params, n->paramsT, tb);
  }
  return TDNNF_OK;
}

}  // namespace tdnnf
