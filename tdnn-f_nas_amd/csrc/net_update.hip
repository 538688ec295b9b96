// net_update.hip -- the optimizer step of the chain trainer (tdnnf_net_update), the part of NnetChainTrainer::TrainInternal (UPSTREAM)
// behind Backprop: the shipped helpers ApplyL2Regularization, UpdateNnetWithMaxChange, ScaleBatchnormStats and ConstrainOrthonormal
// (/root/reference/src/nnet3/nnet-utils.cc:2223-2245, :2085-2175, :1040-1077).  The grouped launches are optim_group.hip; here are the
// per-component table, the BatchNorm statistics' scaling and the per-component orthonormal path for tall matrices.
#include <string.h>

#include <vector>

#include "common.h"
#include "net_model.h"
#include "optim_group.h"

namespace tdnnf {
namespace {

// out (cols x rows) = in (rows x cols)^T, both dense
__global__ void transpose_kernel(const float *in, int rows, int cols, float *out) {
  const long long total = (long long)rows * cols;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / cols), c = (int)(e % cols);
    out[(size_t)c * rows + r] = in[e];
  }
}
// ScaleBatchnormStats: every BatchNorm's [count, sum[D], sumsq[D]] *= s in one launch (block row = one component)
struct ScaleTable {
  double *p[48];
  int n[48];
};
__global__ void scale_doubles_kernel(ScaleTable tb, double s) {
  double *x = tb.p[blockIdx.y];
  const int n = tb.n[blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) x[i] *= s;
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_net_update(tdnnf_net *n, float lr, float l2_scale, long long step, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && n->params && n->grads, "net_update: call net_set_buffers first");
  TDNNF_REQUIRE(lr >= 0.f && l2_scale >= 0.f, "net_update: learning rate and l2 scale must be >= 0 (nnet-utils.cc:2240)");
  TraceRange trace_update("tdnnf_net_update");
  hipStream_t s = (hipStream_t)stream;
  CK(phase_mark(n, 6, s));
  const int nc = (int)n->comps.size();
  std::vector<long long> begin(nc + 1);
  std::vector<float> lrs(nc), l2coef(nc), mc(nc);
  for (int i = 0; i < nc; i++) {
    const CompDesc &c = n->comps[i];
    begin[i] = c.begin;
    lrs[i] = lr * c.lr_factor;
    l2coef[i] = -2.0f * l2_scale * lrs[i] * c.l2;  // ApplyL2Regularization, nnet-utils.cc:2241
    mc[i] = c.max_change;
  }
  begin[nc] = n->num_params;
  // component i owns [begin[i], begin[i+1]) including alignment padding (padding stays zero).  delta = lr g + l2 theta, max-change and the
  // update as three launches over all components (optim_group.hip)
  if (!n->upd || upd_group_params(n->upd) != n->params) {
    upd_group_destroy(n->upd);
    n->upd = nullptr;
    std::vector<UpdComp> uc(nc);
    for (int i = 0; i < nc; i++) {
      const CompDesc &c = n->comps[i];
      uc[i] = UpdComp{begin[i], begin[i + 1], c.rows, c.cols, c.orthonormal};
    }
    CK(upd_group_create(uc, n->params, &n->upd));
  }
  CK(upd_group_step(n->upd, n->params, n->grads, lrs.data(), l2coef.data(), mc.data(), n->cfg.max_param_change, s));
  // ScaleBatchnormStats
  if (n->cfg.batchnorm_stats_scale != 1.0f && !n->cfg.cv_update) {  // (BatchNormTestComponents are not scaled)
    ScaleTable tb;
    memset(&tb, 0, sizeof(tb));
    int nb = 0, maxn = 0;
    for (const StatBlock &b : stat_blocks(n))
      if (!b.relu && nb < 48) {
        tb.p[nb] = b.p();
        tb.n[nb] = b.doubles();
        maxn = std::max(maxn, b.doubles());
        nb++;
      }
    TDNNF_REQUIRE(nb == (int)n->layers.size() + 5, "net_update: too many BatchNorm components for one launch");
    hipLaunchKernelGGL(scale_doubles_kernel, dim3((maxn + 255) / 256, nb), dim3(256), 0, s, tb, (double)n->cfg.batchnorm_stats_scale);
  }
  // ConstrainOrthonormal: each constrained component with probability 1/4 (nnet-utils.cc:1062); the ones chosen this minibatch run
  // together as grouped launches (tall matrices -- none in the recipes' graphs -- keep the per-component path on the transpose)
  std::vector<int> chosen;
  for (int i = 0; i < nc; i++) {
    const CompDesc &c = n->comps[i];
    if (c.orthonormal == 0.f) continue;
    if (::tdnnf::tdnnf_decision((unsigned long long)step, 2 * (unsigned long long)i + 1) % 4 != 0) continue;  // RandInt(0,3) != 0
    if (upd_group_can_ortho(n->upd, i)) {
      chosen.push_back(i);
    } else if (c.rows <= c.cols) {
      CK(tdnnf_constrain_orthonormal(c.orthonormal, n->params + c.begin, c.rows, c.cols, c.cols, n->ws, n->ws_bytes, s));
    } else {  // tall matrix: constrain the transpose (nnet-utils.cc:1068-1075)
      TDNNF_REQUIRE(n->orthoT, "net_update: no transpose buffer for %s", c.name.c_str());
      const long long total = (long long)c.rows * c.cols;
      hipLaunchKernelGGL(transpose_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, n->params + c.begin, c.rows, c.cols, n->orthoT);
      CK(tdnnf_constrain_orthonormal(c.orthonormal, n->orthoT, c.cols, c.rows, c.rows, n->ws, n->ws_bytes, s));
      hipLaunchKernelGGL(transpose_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, n->orthoT, c.cols, c.rows, n->params + c.begin);
    }
  }
  if (!chosen.empty()) CK(upd_group_ortho(n->upd, chosen, s));
  CK(phase_mark(n, 7, s));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // extern "C"
