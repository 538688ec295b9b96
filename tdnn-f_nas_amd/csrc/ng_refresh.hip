// ng_refresh.hip -- everything about W_{t+1} of an OnlineNaturalGradient object (UPSTREAM Kaldi nnet3/natural-gradient-online.{h,cc};
// ng.h has the file map, ng_stats.hip the N-sized passes that feed this).
//
// Fisher model F ~ R^T D R + rho I of rank R; the preconditioned directions are X^ = X - (X W^T) W with W = E^{1/2} R.  On a refresh call
// (first 10 calls, then every update_period-th) the statistics side leaves J = H^T X on the device and K = J J^T, L = H^T H and
// tr(X X^T) in pinned memory.  The R x R symmetric eigen-problem is solved on the host in double, where the reference solves it, but
// off the critical path: an event behind the copies hands them to a worker thread (ng_refresh_submit), and
// W_{t+1} = A_t (J + diag(c) W_t) is formed on the device the next time the object is used (ng_finalize; W_{t+1} is not needed earlier),
// or for all refreshed objects at once by ng_group.hip's NgFin.
#include <math.h>
#include <string.h>

#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "gemm_f32.h"
#include "host_linalg.h"
#include "ng.h"

namespace tdnnf {
namespace {

// ------------------------------------------------------------------ small device kernels
__global__ void add_diag_rows_kernel(float *J, const float *W, const float *coeff, int R, int D) {
  const long long total = (long long)R * D;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) J[e] += coeff[e / D] * W[e];
}
// WT[d][r] = W[r][d];  wlast[r] = W[r][D-1]
__global__ void derive_kernel(const float *W, int Rp, int D, int Dp, float *WT, float *wlast) {
  const long long total = (long long)D * Rp;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int dd = (int)(e / Rp), r = (int)(e % Rp);
    const float v = W[(size_t)r * Dp + dd];
    WT[e] = v;
    if (dd == D - 1) wlast[r] = v;
  }
}

// ------------------------------------------------------------------ worker pool for the host part of a refresh
void host_update(tdnnf_ng *ng);

struct NgPool {
  std::mutex mu;
  std::condition_variable cv_job, cv_done;
  std::deque<tdnnf_ng *> q;
  bool started = false;
  void start() {
    unsigned hw = std::thread::hardware_concurrency();
    int n = hw >= 16 ? 8 : (hw >= 4 ? (int)hw / 2 : 1);
    for (int i = 0; i < n; i++) std::thread([this]() { run(); }).detach();
    started = true;
  }
  void push(tdnnf_ng *ng) {
    std::lock_guard<std::mutex> lk(mu);
    if (!started) start();
    q.push_back(ng);
    cv_job.notify_one();
  }
  void run() {
    for (;;) {
      tdnnf_ng *ng;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_job.wait(lk, [this]() { return !q.empty(); });
        ng = q.front();
        q.pop_front();
      }
      // the job was queued when its copies were enqueued, not when they finished (a stream callback for that stalls the
      // stream for ~0.1 ms per refresh, 72 of them in a refresh step): wait for them here
      (void)hipSetDevice(ng->device);
      (void)hipEventSynchronize(ng->ev_wait ? ng->ev_wait : ng->ev_job);
      host_update(ng);
      {
        std::lock_guard<std::mutex> lk(mu);
        ng->job_done = 1;
      }
      cv_done.notify_all();
    }
  }
  void wait(tdnnf_ng *ng) {
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [ng]() { return ng->job_done != 0; });
  }
  bool done(tdnnf_ng *ng) {
    std::lock_guard<std::mutex> lk(mu);
    return ng->job_done != 0;
  }
};
NgPool &pool() {
  static NgPool *p = new NgPool();  // never destroyed: worker threads outlive static destruction
  return *p;
}

void compute_et(const std::vector<float> &d, double beta, std::vector<double> &sqrt_e, std::vector<double> &inv_sqrt_e) {
  const int R = (int)d.size();
  sqrt_e.resize(R);
  inv_sqrt_e.resize(R);
  for (int i = 0; i < R; i++) {
    const double e = 1.0 / (beta / d[i] + 1.0);
    sqrt_e[i] = sqrt(e);
    inv_sqrt_e[i] = 1.0 / sqrt_e[i];
  }
}

// Z_t, its eigen-decomposition, d_{t+1}, rho_{t+1} and the R x R factor A_t of W_{t+1} = A_t B_t (UPSTREAM
// PreconditionDirectionsInternal, updating branch).  Reads only host memory; runs on a pool thread.
void host_update(tdnnf_ng *ng) {
  const int R = ng->rank, Rp = ng->Rp, D = ng->D, N = ng->job_N;
  const float *Kh = ng->h_K, *Lh = ng->h_L;
  const double tr0 = *ng->h_tr0;
  float eta = 1.0f - expf(-(float)N / ng->num_samples_history);
  if (eta > 0.9f) eta = 0.9f;
  const float rho_t = ng->rho, alpha = ng->alpha;
  double d_sum = 0;
  for (int i = 0; i < R; i++) d_sum += ng->d[i];
  const double beta_t = rho_t * (1.0 + alpha) + alpha * d_sum / D;
  std::vector<double> sqrt_e, inv_sqrt_e;
  compute_et(ng->d, beta_t, sqrt_e, inv_sqrt_e);
  std::vector<double> Z((size_t)R * R), c, U;
  const double eN = (double)eta / N, eN1 = eN * (1.0 - eta);
  for (int i = 0; i < R; i++)
    for (int j = 0; j < R; j++) {
      const double di = ng->d[i] + rho_t, dj = ng->d[j] + rho_t;
      double z = eN * eN * inv_sqrt_e[i] * Kh[i * Rp + j] * inv_sqrt_e[j] + eN1 * inv_sqrt_e[i] * Lh[i * Rp + j] * inv_sqrt_e[j] * (di + dj);
      if (i == j) z += (1.0 - eta) * (1.0 - eta) * di * di;
      Z[(size_t)i * R + j] = z;
    }
  for (int i = 0; i < R; i++)
    for (int j = 0; j < i; j++) Z[(size_t)i * R + j] = Z[(size_t)j * R + i] = 0.5 * (Z[(size_t)i * R + j] + Z[(size_t)j * R + i]);
  hostla::sym_eig(Z, R, c, U);
  const double c_floor = pow(rho_t * (1.0 - eta), 2);
  bool must_reorthogonalize = c[0] > 1.0e+06 * c[R - 1];  // condition_threshold
  std::vector<double> sqrt_c(R);
  double sqrt_c_sum = 0, sqrt_c_max = 0;
  for (int i = 0; i < R; i++) {
    if (c[i] < c_floor) {
      c[i] = c_floor;
      must_reorthogonalize = true;
    }
    sqrt_c[i] = sqrt(c[i]);
    sqrt_c_sum += sqrt_c[i];
    sqrt_c_max = std::max(sqrt_c_max, sqrt_c[i]);
  }
  float rho_t1 = (float)(1.0 / (D - R) * (eta / N * tr0 + (1 - eta) * (D * rho_t + d_sum) - sqrt_c_sum));
  const float floor_val = std::max(ng->epsilon, ng->delta * (float)sqrt_c_max);
  ng->d_next.resize(R);
  for (int i = 0; i < R; i++) ng->d_next[i] = std::max((float)sqrt_c[i] - rho_t1, floor_val);
  if (rho_t1 < floor_val) rho_t1 = floor_val;
  ng->rho_next = rho_t1;
  double d1_sum = 0;
  for (int i = 0; i < R; i++) d1_sum += ng->d_next[i];
  const double beta_t1 = rho_t1 * (1.0 + alpha) + alpha * d1_sum / D;
  compute_et(ng->d_next, beta_t1, ng->sqrt_e1, ng->inv_sqrt_e1);
  memset(ng->h_coeff, 0, sizeof(float) * Rp);
  memset(ng->h_At, 0, sizeof(float) * (size_t)Rp * Rp);
  for (int r = 0; r < R; r++) ng->h_coeff[r] = (float)((1.0 - eta) / (eta / N) * (ng->d[r] + rho_t));
  for (int i = 0; i < R; i++)
    for (int j = 0; j < R; j++)
      ng->h_At[(size_t)i * Rp + j] = (float)(U[(size_t)j * R + i] * (eta / N) * ng->sqrt_e1[i] / sqrt_c[i] * inv_sqrt_e[j]);
  ng->must_reorth = must_reorthogonalize;
}

// ------------------------------------------------------------------ device state
int alloc_state(tdnnf_ng *ng, int D) {
  if (ng->rank >= D) ng->rank = D - 1;
  const int R = ng->rank, Rp = pad4(std::max(R, 1)), Dp = pad4(D);
  ng->D = D;
  ng->Dp = Dp;
  ng->Rp = Rp;
  const size_t fRD = (size_t)Rp * Dp, fRR = (size_t)Rp * Rp;
  // (W^T: kWtPadRows zero rows behind its D -- ng_valu.hip reads whole K steps of up to 64 rows, the tile's columns there are zeros)
  const size_t fWT = pad4z((size_t)(D + kWtPadRows) * Rp);
  const size_t floats = 3 * fRD + fWT + 4 * fRR + 3 * Rp + 8 + 8;
  TDNNF_HIP(hipMalloc((void **)&ng->dev, sizeof(float) * floats));
  TDNNF_HIP(hipMemset(ng->dev, 0, sizeof(float) * floats));
  float *p = ng->dev;
  ng->W = p; p += fRD;
  ng->J = p; p += fRD;
  ng->W1 = p; p += fRD;
  ng->WT = p; p += fWT;
  ng->WWT = p; p += fRR;
  ng->Kd = p; p += fRR;
  ng->Ld = p; p += fRR;
  ng->Ad = p; p += fRR;
  ng->wlast = p; p += Rp;
  ng->coeff = p; p += Rp;
  ng->tmpR = p; p += Rp;
  ng->neg_one = p; p += 4;
  ng->scale_f = p; p += 4;
  ng->scal = (double *)p;
  const size_t pin_floats = 3 * fRR + Rp + 4 + 4;
  TDNNF_HIP(hipHostMalloc((void **)&ng->pin, sizeof(float) * pin_floats, hipHostMallocDefault));
  if (!ng->ev_job) {
    TDNNF_HIP(hipGetDevice(&ng->device));
    TDNNF_HIP(hipEventCreateWithFlags(&ng->ev_job, hipEventDisableTiming | hipEventBlockingSync));
  }
  memset(ng->pin, 0, sizeof(float) * pin_floats);
  float *h = ng->pin;
  ng->h_K = h; h += fRR;
  ng->h_L = h; h += fRR;
  ng->h_At = h; h += fRR;
  ng->h_coeff = h; h += Rp;
  ng->h_scale = h; h += 4;
  ng->h_tr0 = (double *)h;
  const float consts[8] = {-1.0f, 0, 0, 0, 1.0f, 0, 0, 0};  // neg_one, scale_f
  TDNNF_HIP(hipMemcpy(ng->neg_one, consts, sizeof(consts), hipMemcpyHostToDevice));
  return TDNNF_OK;
}

int derive(tdnnf_ng *ng, hipStream_t s) {  // W^T, W W^T and the last column of W after W changed
  const int Rp = ng->Rp, D = ng->D, Dp = ng->Dp;
  hipLaunchKernelGGL(derive_kernel, dim3(grid_for((long long)D * Rp, 256)), dim3(256), 0, s, ng->W, Rp, D, Dp, ng->WT, ng->wlast);
  TDNNF_HIP(rows_gemm_1seg(ng->W, Dp, ng->W, Dp, true, ng->WWT, Rp, Rp, Rp, Dp, 2, nullptr, nullptr, s));  // W W^T
  return TDNNF_OK;
}

// ReorthogonalizeRt1 (UPSTREAM): bring R_{t+1} = E_{t+1}^{-1/2} W_{t+1} back to orthonormal rows.  Rare; synchronous.
int reorthogonalize(tdnnf_ng *ng, hipStream_t s) {
  const int R = ng->rank, Rp = ng->Rp, D = ng->D, Dp = ng->Dp;
  const size_t fRR = (size_t)Rp * Rp, fRD = (size_t)Rp * Dp;
  TDNNF_HIP(rows_gemm_1seg(ng->W1, Dp, ng->W1, Dp, true, ng->Kd, Rp, Rp, Rp, Dp, 2, nullptr, nullptr, s));  // O = W W^T
  std::vector<float> Oh(fRR);
  TDNNF_HIP(hipMemcpyAsync(Oh.data(), ng->Kd, sizeof(float) * fRR, hipMemcpyDeviceToHost, s));
  TDNNF_HIP(hipStreamSynchronize(s));
  std::vector<double> O((size_t)R * R), Cm, Ci;
  bool is_unit = true;
  for (int i = 0; i < R; i++)
    for (int j = 0; j <= i; j++) {
      const double a = (double)Oh[(size_t)i * Rp + j] * ng->inv_sqrt_e1[i] * ng->inv_sqrt_e1[j];
      O[(size_t)i * R + j] = O[(size_t)j * R + i] = a;
      if (fabs(a - (i == j ? 1.0 : 0.0)) > 1.0e-03) is_unit = false;
    }
  if (is_unit) return TDNNF_OK;
  bool ok = hostla::cholesky_inverse(O, R, Cm, Ci);
  if (ok) {
    double cmax = 0;
    for (auto v : Ci) cmax = std::max(cmax, v);
    if (!(cmax < 100.0)) ok = false;
  }
  if (!ok) {  // Gram-Schmidt on the host, then W = E^{1/2} R
    std::vector<float> Wh(fRD);
    TDNNF_HIP(hipMemcpyAsync(Wh.data(), ng->W1, sizeof(float) * fRD, hipMemcpyDeviceToHost, s));
    TDNNF_HIP(hipStreamSynchronize(s));
    hostla::orthogonalize_rows(Wh, R, D, Dp);
    for (int i = 0; i < R; i++)
      for (int k = 0; k < D; k++) Wh[(size_t)i * Dp + k] *= (float)ng->sqrt_e1[i];
    TDNNF_HIP(hipMemcpyAsync(ng->W1, Wh.data(), sizeof(float) * fRD, hipMemcpyHostToDevice, s));
    TDNNF_HIP(hipStreamSynchronize(s));
    return TDNNF_OK;
  }
  std::vector<float> Th(fRR, 0.f);  // W <- (E^{1/2} C^{-1} E^{-1/2}) W
  for (int i = 0; i < R; i++)
    for (int j = 0; j <= i; j++) Th[(size_t)i * Rp + j] = (float)(Ci[(size_t)i * R + j] * ng->sqrt_e1[i] * ng->inv_sqrt_e1[j]);
  TDNNF_HIP(hipMemcpyAsync(ng->Ad, Th.data(), sizeof(float) * fRR, hipMemcpyHostToDevice, s));
  TDNNF_HIP(hipStreamSynchronize(s));
  TDNNF_HIP(rows_gemm_1seg(ng->Ad, Rp, ng->W1, Dp, false, ng->J, Dp, Rp, Dp, Rp, 2, nullptr, nullptr, s));
  TDNNF_HIP(hipMemcpyAsync(ng->W1, ng->J, sizeof(float) * fRD, hipMemcpyDeviceToDevice, s));
  return TDNNF_OK;
}

}  // namespace

void ng_refresh_submit(tdnnf_ng *ng, int N, hipEvent_t wait_event) {
  ng->job_N = N;
  ng->job_done = 0;
  ng->pending = 1;
  ng->ev_wait = wait_event;
  pool().push(ng);
}
void ng_refresh_installed(tdnnf_ng *ng) {
  ng->pending = 0;
  ng->d = ng->d_next;
  ng->rho = ng->rho_next;
}
void ng_pool_wait(tdnnf_ng *ng) { pool().wait(ng); }
bool ng_pool_done(tdnnf_ng *ng) { return pool().done(ng); }

int ng_init_default(tdnnf_ng *ng, int D, hipStream_t s) {  // InitDefault (UPSTREAM)
  int rc = alloc_state(ng, D);
  if (rc) return rc;
  const int R = ng->rank, Dp = ng->Dp;
  ng->d.assign(R, ng->epsilon);
  ng->rho = ng->epsilon;
  ng->t = 0;
  if (R == 0) return TDNNF_OK;
  std::vector<float> W((size_t)ng->Rp * Dp, 0.f);
  const float first_elem = 1.1f;
  const float E_tii = 1.0f / (2.0f + (D + R) * ng->alpha / D);
  for (int r = 0; r < R; r++) {  // InitOrthonormalSpecial
    int ncols = 0;
    for (int c = r; c < D; c += R) ncols++;
    const float normalizer = 1.0f / sqrtf(first_elem * first_elem + ncols - 1);
    int i = 0;
    for (int c = r; c < D; c += R, i++) W[(size_t)r * Dp + c] = normalizer * (i == 0 ? first_elem : 1.0f) * sqrtf(E_tii);
  }
  TDNNF_HIP(hipMemcpyAsync(ng->W, W.data(), sizeof(float) * W.size(), hipMemcpyHostToDevice, s));
  TDNNF_HIP(hipStreamSynchronize(s));
  return derive(ng, s);
}

// Second half of a refresh: wait for the host part, then W_{t+1} = A_t (J + diag(coeff) W_t) on the device.
int ng_finalize(tdnnf_ng *ng, hipStream_t s) {
  if (!ng->pending) return TDNNF_OK;
  pool().wait(ng);
  const int Rp = ng->Rp, Dp = ng->Dp;
  const size_t fRR = (size_t)Rp * Rp, fRD = (size_t)Rp * Dp;
  TDNNF_HIP(hipMemcpyAsync(ng->coeff, ng->h_coeff, sizeof(float) * Rp, hipMemcpyHostToDevice, s));
  TDNNF_HIP(hipMemcpyAsync(ng->Ad, ng->h_At, sizeof(float) * fRR, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(add_diag_rows_kernel, dim3(grid_for((long long)fRD, 256)), dim3(256), 0, s, ng->J, ng->W, ng->coeff, Rp, Dp);
  TDNNF_HIP(rows_gemm_1seg(ng->Ad, Rp, ng->J, Dp, false, ng->W1, Dp, Rp, Dp, Rp, 2, nullptr, nullptr, s));  // W1 = A_t (J + diag(c) W_t)
  if (ng->must_reorth) {
    int rc = reorthogonalize(ng, s);
    if (rc) return rc;
  }
  TDNNF_HIP(hipMemcpyAsync(ng->W, ng->W1, sizeof(float) * fRD, hipMemcpyDeviceToDevice, s));
  ng_refresh_installed(ng);
  return derive(ng, s);
}

int ng_finalize_one(tdnnf_ng *ng, hipStream_t s) {
  NgCallScope scope;
  return ng_finalize(ng, s);
}

int ng_finalize_if_ready(tdnnf_ng *ng, hipStream_t s, int *did) {
  *did = 0;
  if (!ng || ng->rank == 0 || !ng->pending || !pool().done(ng)) return TDNNF_OK;
  NgCallScope scope;
  *did = 1;
  return ng_finalize(ng, s);
}

}  // namespace tdnnf
