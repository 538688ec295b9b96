// ng_group.hip -- the latency-bound half of OnlineNaturalGradient for MANY components at once (ng.h, "Grouped side chain"): the host
// code of NgGroup (the chain) and NgFin (the grouped finalize); their kernels and descriptors are in ng_group_kernels.h.
//
// Per component and side the reference's PreconditionDirections (UPSTREAM Kaldi nnet3/natural-gradient-online.cc; call sites
// /root/reference/src/nnet3/nnet-tdnn-component.cc:598-599, nnet-simple-component.cc:3001-3002) needs, after the N-sized pass
// H = X W^T:  L = H^T H, tr(X^ X^^T) = tr(XX^T) - 2 tr(L) + <L, W W^T> and the scale; on a refresh K = J J^T and the R x R
// eigen-problem (host, host_linalg.h).  The trainer then projects the raw gradient, T <- (I - Wy^T Wy) T (I - Wx^T Wx), and adds
// a b T to the minibatch's gradient (nnet-tdnn-component.cc:604-624).  Run per component that is ~17 launches of a few
// microseconds of work each, 36 components per step: round 2's step at the recipes' minibatch was a chain of ~1 290 dependent
// launches.  Here every stage is ONE launch over all components of a group (a gradient bucket of the trainer):
//   1  bias columns into T                                   ng_set_columns_kernel
//   2  L partials, slab-parallel over the rows of H          ng_l_partial_kernel      (f32 MFMA, symmetric tiles only)
//   3  L, traces, scale per (component, side)                ng_l_finish_kernel
//   4  Q = T Wx^T      5  T -= Q Wx      6  P = Wy T      7  T -= Wy^T P           ggemm_kernel (+ ggemm_reduce_kernel when K is split)
//   8  gradient += a b T                                     ng_commit_kernel
//   refresh steps:  K = J J^T (ggemm), K / L / tr(XX^T) to pinned host memory (ng_stage_kernel), one event for the pool threads;
//   next step:      W_{t+1} = A_t (J + diag(c) W_t), W^T, last column, W W^T for ALL refreshed objects (ng_group_finalize).
// Results are deterministic: every reduction has a fixed order (no atomics).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gemm_f32.h"
#include "ggemm.h"
#include "ng.h"
#include "ng_group_kernels.h"

namespace tdnnf {

struct NgGroup {
  std::vector<NgGroupComp> comps;
  std::vector<tdnnf_ng *> objs;  // 2 per component: in, out
  char *dev = nullptr;           // one allocation: tables, partial tiles, Q / P
  PairDesc *pairs = nullptr;
  CompDesc *cdesc = nullptr;
  float *lpart = nullptr;
  int npairs = 0, nslabs = 0, commit_blocks = 0;
  size_t l_lds = 0;
  DevList stage[4], kstage;
  hipEvent_t ev_staged = nullptr;
};

int ng_group_create(const std::vector<NgGroupComp> &comps, NgGroup **out) {
  TDNNF_REQUIRE(out && !comps.empty(), "ng_group_create: no components");
  NgGroup *g = new NgGroup();
  g->comps = comps;
  std::vector<PairDesc> pairs;
  std::vector<CompDesc> cdesc;
  GemmList st[4], kst;
  size_t qp_floats = 0;
  std::vector<size_t> q_off, p_off;
  int slab_total = 0, blk = 0;
  for (const NgGroupComp &c : comps) {
    TDNNF_REQUIRE(c.in && c.out && c.in->D == c.Dx && c.in->Dp == c.ldT && c.out->D == c.Do && c.in->rank > 0 && c.out->rank > 0 && c.in->Rp <= 96 &&
                      c.out->Rp <= 96 && c.N > 0,
                  "ng_group_create: a preconditioner is not initialised for its component (or its rank is outside 1..96)");
    q_off.push_back(qp_floats);
    qp_floats += ((size_t)c.Do * c.in->Rp + 63) & ~(size_t)63;
    p_off.push_back(qp_floats);
    qp_floats += ((size_t)c.out->Rp * c.ldT + 63) & ~(size_t)63;
    for (int side = 0; side < 2; side++) {
      tdnnf_ng *ng = side == 0 ? c.in : c.out;
      g->objs.push_back(ng);
      PairDesc p;
      memset(&p, 0, sizeof(p));
      p.H = side == 0 ? c.H_in : c.H_out;
      p.part = side == 0 ? c.part_in : c.part_out;
      p.Ld = ng->Ld;
      p.WWT = ng->WWT;
      p.scal = ng->scal;
      p.scale_f = ng->scale_f;
      p.Kd = ng->Kd;
      TDNNF_HIP(hipHostGetDevicePointer((void **)&p.hK, ng->h_K, 0));
      TDNNF_HIP(hipHostGetDevicePointer((void **)&p.hL, ng->h_L, 0));
      TDNNF_HIP(hipHostGetDevicePointer((void **)&p.h_tr0, ng->h_tr0, 0));
      p.ones_term = (side == 0 && c.bsum) ? (double)c.N : 0.0;
      p.N = c.N;
      p.Rp = ng->Rp;
      p.nt = (ng->Rp + 31) / 32;
      p.npart = rows_gemm_sumsq_blocks(c.N);
      // slabs: at least 256 rows, at most 32 per pair (the finish kernel adds them serially)
      int rps = std::max(256, (c.N + 31) / 32);
      rps = (rps + 7) & ~7;
      p.rows_per_slab = rps;
      p.nslab = (c.N + rps - 1) / rps;
      p.slab0 = slab_total;
      slab_total += p.nslab;
      pairs.push_back(p);
      // refresh: K = J J^T
      kst.add(ng->J, ng->Dp, 1, ng->J, 1, ng->Dp, ng->Kd, ng->Rp, ng->Rp, ng->Rp, ng->Dp, 1.0f, 0);
    }
    CompDesc d;
    memset(&d, 0, sizeof(d));
    d.T = c.T;
    d.bsum = c.bsum;
    d.sa = c.in->scale_f;
    d.sb = c.out->scale_f;
    d.W_acc = c.W_acc;
    d.bias_acc = c.bias_acc;
    d.Do = c.Do;
    d.ldT = c.ldT;
    d.ldw = c.ldw;
    d.Dx = c.Dx;
    d.blk0 = blk;
    blk += (int)(((long long)c.Do * c.Dx + 1023) / 1024);
    cdesc.push_back(d);
  }
  g->npairs = (int)pairs.size();
  g->nslabs = slab_total;
  g->commit_blocks = blk;
  // Q and P live behind the tables; the projection stages (ng.h: T <- (I - Wy^T Wy) T (I - Wx^T Wx))
  // are built once their addresses are known
  size_t bytes = 0;
  bytes = carve_room(bytes, sizeof(PairDesc) * pairs.size());
  bytes = carve_room(bytes, sizeof(CompDesc) * cdesc.size());
  bytes = carve_room(bytes, sizeof(float) * (size_t)slab_total * kLSlabFloats);
  bytes = carve_room(bytes, sizeof(float) * qp_floats);
  // (task lists are sized after a dry build with null Q / P: their counts do not depend on the addresses)
  auto build = [&](float *qp) {
    for (auto &l : st) l = GemmList();
    for (size_t i = 0; i < comps.size(); i++) {
      const NgGroupComp &c = comps[i];
      float *Q = qp + q_off[i], *P = qp + p_off[i];
      const int Rx = c.in->Rp, Ry = c.out->Rp;
      st[0].add(c.T, c.ldT, 1, c.in->WT, Rx, 1, Q, Rx, c.Do, Rx, c.Dx, 1.0f, 0);            // Q = T Wx^T   (WT: D x Rp)
      st[1].add(Q, Rx, 1, c.in->W, c.in->Dp, 1, c.T, c.ldT, c.Do, c.ldT, Rx, -1.0f, 1);     // T -= Q Wx
      st[2].add(c.out->W, c.out->Dp, 1, c.T, c.ldT, 1, P, c.ldT, Ry, c.ldT, c.Do, 1.0f, 0);  // P = Wy T
      st[3].add(c.out->WT, Ry, 1, P, c.ldT, 1, c.T, c.ldT, c.Do, c.ldT, Ry, -1.0f, 1);      // T -= Wy^T P
    }
  };
  build(nullptr);
  GemmList *lists[5] = {&st[0], &st[1], &st[2], &st[3], &kst};
  DevList *dls[5] = {&g->stage[0], &g->stage[1], &g->stage[2], &g->stage[3], &g->kstage};
  bytes = devlists_room(bytes, lists, 5) + 1024;  // (the stages run one after the other: one partial buffer)
  if (hipMalloc((void **)&g->dev, bytes) != hipSuccess) {
    set_error("ng_group_create: cannot allocate %zu bytes", bytes);
    delete g;
    return TDNNF_EHIP;
  }
  char *cur = g->dev;
  g->pairs = carve<PairDesc>(cur, pairs.size());
  g->cdesc = carve<CompDesc>(cur, cdesc.size());
  g->lpart = carve<float>(cur, (size_t)slab_total * kLSlabFloats);
  float *qp = carve<float>(cur, qp_floats);
  build(qp);
  int rc = devlists_upload(cur, lists, dls, 5);
  if (rc) return rc;
  TDNNF_HIP(hipMemcpy(g->pairs, pairs.data(), sizeof(PairDesc) * pairs.size(), hipMemcpyHostToDevice));
  TDNNF_HIP(hipMemcpy(g->cdesc, cdesc.data(), sizeof(CompDesc) * cdesc.size(), hipMemcpyHostToDevice));
  TDNNF_HIP(hipEventCreateWithFlags(&g->ev_staged, hipEventDisableTiming | hipEventBlockingSync));
  g->l_lds = sizeof(float) * 2 * kLSlabFloats;  // two accumulator images (l_partial_body)
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void *)ng_l_partial_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g->l_lds);
    attr_done = true;
  }
  *out = g;
  return TDNNF_OK;
}

void ng_group_destroy(NgGroup *g) {
  if (!g) return;
  for (tdnnf_ng *ng : g->objs)
    if (ng->pending && ng->ev_wait == g->ev_staged) ng_pool_wait(ng);  // a pool thread may still be waiting on this group's event
  if (g->ev_staged) (void)hipEventDestroy(g->ev_staged);
  (void)hipFree(g->dev);
  delete g;
}

int ng_group_run(NgGroup *g, hipStream_t s) {
  TDNNF_REQUIRE(g, "ng_group_run: null group");
  const int nc = (int)g->comps.size();
  // every object of the group is in the same place of its refresh schedule (they are used once per minibatch, from the same start)
  const bool upd = g->objs[0]->cur_upd;
  for (tdnnf_ng *ng : g->objs)
    TDNNF_REQUIRE(ng->cur_upd == upd && ng->cur_N > 0 && !ng->pending, "ng_group_run: the group's preconditioners are out of step");
  hipLaunchKernelGGL(ng_set_columns_kernel, dim3(nc), dim3(256), 0, s, g->cdesc);
  hipLaunchKernelGGL(ng_l_partial_kernel, dim3(g->nslabs), dim3(256), g->l_lds, s, g->pairs, g->npairs, g->lpart);
  hipLaunchKernelGGL(ng_l_finish_kernel, dim3(g->npairs), dim3(1024), 0, s, g->pairs, g->lpart);
  if (upd) {
    int rc = launch_list(g->kstage, s);
    if (rc) return rc;
    hipLaunchKernelGGL(ng_stage_kernel, dim3(g->npairs), dim3(256), 0, s, g->pairs);
    TDNNF_HIP(hipEventRecord(g->ev_staged, s));
  }
  for (int i = 0; i < 4; i++) {
    int rc = launch_list(g->stage[i], s);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(ng_commit_group_kernel, dim3(g->commit_blocks), dim3(256), 0, s, g->cdesc, nc);
  TDNNF_LAUNCH_CHECK();
  for (tdnnf_ng *ng : g->objs) {
    if (upd) ng_refresh_submit(ng, ng->cur_N, g->ev_staged);
    ng->cur_N = 0;
    ng->t += 1;
  }
  return TDNNF_OK;
}

struct NgFin {
  std::vector<tdnnf_ng *> objs;
  char *dev = nullptr;
  FinDesc *fd = nullptr;
  int nf = 0, blocks = 0;
  DevList w1, wwt;
};

int ng_fin_create(const std::vector<tdnnf_ng *> &objs_in, NgFin **out) {
  TDNNF_REQUIRE(out, "ng_fin_create: null argument");
  NgFin *f = new NgFin();
  for (tdnnf_ng *ng : objs_in)
    if (ng && ng->rank > 0 && ng->D != 0) f->objs.push_back(ng);
  std::vector<FinDesc> fd;
  GemmList w1, wwt;
  int blk = 0;
  for (tdnnf_ng *ng : f->objs) {
    FinDesc d;
    d.J = ng->J; d.W = ng->W; d.W1 = ng->W1; d.WT = ng->WT; d.wlast = ng->wlast;
    TDNNF_HIP(hipHostGetDevicePointer((void **)&d.h_coeff, ng->h_coeff, 0));
    d.Rp = ng->Rp; d.D = ng->D; d.Dp = ng->Dp;
    d.blk0 = blk;
    blk += (int)(((long long)ng->Rp * ng->Dp + 1023) / 1024);
    fd.push_back(d);
    float *hAt = nullptr;
    TDNNF_HIP(hipHostGetDevicePointer((void **)&hAt, ng->h_At, 0));
    w1.add(hAt, ng->Rp, 1, ng->J, ng->Dp, 1, ng->W1, ng->Dp, ng->Rp, ng->Dp, ng->Rp, 1.0f, 0);      // W1 = A_t (J + diag(c) W)
    wwt.add(ng->W, ng->Dp, 1, ng->W, 1, ng->Dp, ng->WWT, ng->Rp, ng->Rp, ng->Rp, ng->Dp, 1.0f, 0);  // W W^T
  }
  f->nf = (int)fd.size();
  f->blocks = blk;
  if (f->nf == 0) {
    *out = f;
    return TDNNF_OK;
  }
  GemmList *lists[2] = {&w1, &wwt};
  DevList *dls[2] = {&f->w1, &f->wwt};
  const size_t bytes = devlists_room(carve_room(0, sizeof(FinDesc) * fd.size()), lists, 2) + 1024;
  if (hipMalloc((void **)&f->dev, bytes) != hipSuccess) {
    set_error("ng_fin_create: cannot allocate %zu bytes", bytes);
    delete f;
    return TDNNF_EHIP;
  }
  char *cur = f->dev;
  f->fd = carve<FinDesc>(cur, fd.size());
  int rc = devlists_upload(cur, lists, dls, 2);
  if (rc) return rc;
  TDNNF_HIP(hipMemcpy(f->fd, fd.data(), sizeof(FinDesc) * fd.size(), hipMemcpyHostToDevice));
  *out = f;
  return TDNNF_OK;
}

void ng_fin_destroy(NgFin *f) {
  if (!f) return;
  (void)hipFree(f->dev);
  delete f;
}

int ng_fin_run(NgFin *f, hipStream_t s, bool wait, int *did) {
  *did = 0;
  TDNNF_REQUIRE(f, "ng_fin_run: null argument");
  size_t pending = 0;
  for (tdnnf_ng *ng : f->objs) pending += ng->pending ? 1 : 0;
  if (pending == 0) return TDNNF_OK;
  if (!wait)
    for (tdnnf_ng *ng : f->objs)
      if (ng->pending && !ng_pool_done(ng)) return TDNNF_OK;
  bool reorth = false;
  for (tdnnf_ng *ng : f->objs)
    if (ng->pending) {
      ng_pool_wait(ng);
      reorth = reorth || ng->must_reorth;
    }
  *did = 1;
  if (reorth || pending != f->objs.size()) {  // ReorthogonalizeRt1 (rare, synchronous) / objects out of step: one by one
    for (tdnnf_ng *ng : f->objs) {
      int rc = ng_finalize_one(ng, s);
      if (rc) return rc;
    }
    return TDNNF_OK;
  }
  hipLaunchKernelGGL(ng_fin_adddiag_kernel, dim3(f->blocks), dim3(256), 0, s, f->fd, f->nf);
  int rc = launch_list(f->w1, s);
  if (rc) return rc;
  hipLaunchKernelGGL(ng_fin_derive_kernel, dim3(f->blocks), dim3(256), 0, s, f->fd, f->nf);
  rc = launch_list(f->wwt, s);
  if (rc) return rc;
  TDNNF_LAUNCH_CHECK();
  for (tdnnf_ng *ng : f->objs) ng_refresh_installed(ng);
  return TDNNF_OK;
}

}  // namespace tdnnf
