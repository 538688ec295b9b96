// online.hip -- streaming forward-only inference: per-stream layer state carried between calls (tdnnf_online_*, include/tdnnf_hip.h
// "inference (forward only, streaming)").
//
// nnet3's looped computation (DecodableNnetLoopedOnline, UPSTREAM, not shipped) restated for the TDNN-F graphs of net_graph.hip.  A step
// advances every active stream by one window of F input frames and computes, per layer, only the F / step time rows that are new; what
// the taps above a buffer still need from earlier steps is kept per slot on the device.  In the t-major row order (row = time * B +
// position in the active list) the time-concatenation [carried tail | new rows] of a layer's input is one contiguous row range, so
// the schedule is the whole-utterance one (infer_forward.hip: BatchNorm and bypass in the GEMM epilogue) on fewer rows, in exact f32.
//
// Windows, relative to the step's first output frame clock - D and derived downwards as net_layer_grids derives a chunk's grids:
// a layer's .linear output (and its input) starts `right tap` later than the layer's output, so at the bottom the input-layer rows
// start at sum(right taps) and the last feature frame they splice is clock + F - 1 - (D - right).  Every buffer is
// [h carried time rows | F / step new ones] x B:
//   X[l]  input of tdnnf layer l (X[0] = tdnn1's output, X[L] = the head's input): h = max(left, right) / step (the .linear's left tap
//         and the bypass rows, which lie `right` before the new rows);
//   Y[l]  output of layer l's .linear: h = right / step, rounded up to whole blocks of rho time steps where the .affine reads it in the
//         rho row order (the new part is whole blocks because F is a multiple of frame_subsampling);
//   the last D - right + 2 feature frames of a slot, for the input layer's splice (two copies: a step reads one and writes the other).
// State storage is indexed by slot, the step's buffers by position in the active list: one launch copies every buffer's tail in
// (state -> head of the buffer) before the layers run and one copies it out (last h time rows -> state) after them.
#include <limits.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "infer_forward.h"
#include "net_model.h"

using namespace tdnnf;

namespace {

constexpr int kTab = 6;  // device table of a step, per active stream: [slot, first passed row in feats, passed rows, which tail copy holds its frames, first computed output index (may be < 0), number of output rows of the utterance (INT_MAX: not known yet)]

// One carried buffer: `h` units before `m` new ones, a unit = one time step (rho > 1: one block of rho time steps) of one stream,
// `unit` floats.  work: [unit k][position i]; state: per slot at state_off, [unit k].
struct CarryDesc {
  float *work;
  long long state_off;
  int h, m, unit, pad;
};

// The [carried frames | clamped window] of every active stream with its i-vector, straight into the spliced lda layout (t-major: row
// k B + i = [frame(k), frame(k + 1), frame(k + 2) ; i-vector], k < F, in positions of the concatenation), and the slot's next carried
// frames (positions F .. F + hf - 1) into the other tail copy.  Position p < hf: carried frame p; else window position p - hf, which
// past the passed rows takes the last one (nnet3's edge padding; a window before the utterance passes its first frame alone).
// VEC 4: 16-byte accesses (feat_dim, ivector_dim, strides and pointers multiples of 4 floats).
template <int VEC>
__global__ __launch_bounds__(256) void online_gather_kernel(MatView feats, MatView iv, const int *tab, int B, int F, int hf, float *state,
                                                            long long slot_floats, long long tail_off, int fdp, MatView out) {
  const int fd = feats.cols, cv = out.cols / VEC, fv = fd / VEC;
  const long long spliced = (long long)out.rows * cv, total = spliced + (long long)B * hf * fv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    int i, p, c;
    float *dst;
    const float *src = nullptr;
    if (e < spliced) {
      const int r = (int)(e / cv), k = r / B;
      c = (int)(e % cv) * VEC;
      i = r % B;
      dst = out.data + (size_t)r * out.stride + c;
      if (c >= 3 * fd) {
        src = iv.data + (size_t)i * iv.stride + (c - 3 * fd);
        p = -1;
      } else {
        p = k + c / fd;
        c = c % fd;
      }
    } else {
      const long long e2 = e - spliced;
      const int r = (int)(e2 / fv), q = r % hf;
      c = (int)(e2 % fv) * VEC;
      i = r / hf;
      p = q + F;
      const int *t = tab + kTab * i;
      dst = state + (size_t)t[0] * slot_floats + tail_off + (size_t)((t[3] ^ 1) * hf + q) * fdp + c;
    }
    if (p >= 0) {
      const int *t = tab + kTab * i;
      if (p < hf) {
        src = state + (size_t)t[0] * slot_floats + tail_off + (size_t)(t[3] * hf + p) * fdp + c;
      } else {
        const int w = min(p - hf, t[2] - 1);
        src = feats.data + (size_t)(t[1] + w) * feats.stride + c;
      }
    }
    if (VEC == 4) *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
    else *dst = *src;
  }
}

// Every buffer's tail in one launch (blockIdx.y = buffer).  OUT false: state -> the h units at the head of the buffer; OUT true: the
// last h units of [carried | new] -> state.  16-byte accesses throughout: units are whole padded rows (ldpad) of arena buffers.
template <bool OUT>
__global__ __launch_bounds__(256) void online_carry_kernel(const CarryDesc *descs, const int *tab, int B, float *state, long long slot_floats) {
  const CarryDesc d = descs[blockIdx.y];
  const int uv = d.unit / 4;
  const long long total = (long long)d.h * B * uv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int v = (int)(e % uv), r = (int)(e / uv), i = r % B, k = r / B;
    float4 *w = reinterpret_cast<float4 *>(d.work + ((size_t)(k + (OUT ? d.m : 0)) * B + i) * d.unit) + v;
    float4 *st = reinterpret_cast<float4 *>(state + (size_t)tab[kTab * i] * slot_floats + d.state_off + (size_t)k * d.unit) + v;
    if (OUT) *st = *w;
    else *w = *st;
  }
}

// Output placement: row_map[j B + i] = i Tout + (its index among the stream's kept rows) for the computed output rows that lie inside
// the utterance, -1 for those in front of it or, once its length is known, past its end.
__global__ void online_row_map_kernel(const int *tab, int B, int Tout, int *row_map) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= B * Tout) return;
  const int jj = m / B, i = m % B, j0 = tab[kTab * i + 4], j = j0 + jj;
  row_map[m] = j >= 0 && j < tab[kTab * i + 5] ? i * Tout + (j - max(j0, 0)) : -1;
}

// The window of one step: v = [clock, first passed frame, passed rows, first output row, kept output rows] of a stream of T frames at
// `clock` (T < 0: the end has not been seen, a window at clock >= 0 is full).  The one place this arithmetic lives: tdnnf_online_schedule
// lists it, tdnnf_online_step checks the caller's rows against it and places the outputs by it.
void online_window(int F, int fsf, int D, int clock, int T, int v[5]) {
  v[0] = clock;
  if (clock < 0) {  // warm-up: frame 0 alone
    v[1] = 0;
    v[2] = 1;
  } else if (T < 0 || clock + F <= T) {
    v[1] = clock;
    v[2] = F;
  } else if (clock < T) {  // the utterance ends here
    v[1] = clock;
    v[2] = T - clock;
  } else {  // flush: the last frame alone
    v[1] = T - 1;
    v[2] = 1;
  }
  const int j0 = (clock - D) / fsf, lo = std::max(j0, 0);  // (clock and D are multiples of fsf)
  const int hi = T < 0 ? j0 + F / fsf : std::min(j0 + F / fsf, (T + fsf - 1) / fsf);
  v[3] = lo;
  v[4] = std::max(0, hi - lo);
}
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

}  // namespace

struct tdnnf_online {
  const tdnnf_net *model;
  int F, fsf, Tout, num_slots, which;
  int left, right, D, W, hf;  // context in input frames, latency, warm-up frames, carried feature frames
  struct Layer {
    int a, b, bn, ls, s_out, rho;  // taps, bottleneck, step of the .linear (= of X[l]), step of the output, s_out / ls
    int hx, mx, hy, my, m_out;     // time rows: carried / new of X[l] and Y[l], new of the output
    float *Y;
  };
  std::vector<Layer> layers;
  std::vector<float *> X;  // L + 1
  int hx_top = 0;
  int nbn;
  BnTable bn;
  char *arena = nullptr;
  float *lda_in, *lda_out, *lin_tmp, *relu_tmp, *state;
  FwdHead head;
  FwdBuffers fwd;  // where a step of fwd_B active streams lives (step_buffers)
  int fwd_B = 0;
  CarryDesc *descs;
  std::vector<CarryDesc> host_descs;
  long long slot_floats = 0, tail_off = 0, carry_max = 0;  // carry_max: the largest h * unit / 4 of a descriptor
  int fdp = 0, carried_per_stream = 0;
  struct Slot {
    int clock, T, parity;
  };
  std::vector<Slot> slots;
  std::vector<int> host_table;
  long long gemm_rows = 0, carried_rows = 0;
  int fused = 0, fallback = 0;
};

namespace {

void layout(tdnnf_online *q, Arena &A) {
  const tdnnf_net_config &c = q->model->cfg;
  const long long B = q->num_slots;
  const int Hd = c.hidden_dim, lda_dim = 3 * c.feat_dim + c.ivector_dim, L = (int)q->layers.size();
  const long long N0 = (long long)q->F * B, No = (long long)q->Tout * B;
  q->host_descs.clear();
  long long so = 0, lin_rows = 0, relu_rows = 0;
  int bn_max = 0;
  auto carried = [&](float *work, int h, int m, int rho, int cols) {
    if (h == 0) return;
    q->host_descs.push_back(CarryDesc{work, so, h / rho, m / rho, rho * ldpad(cols), 0});
    so += (long long)h * ldpad(cols);
  };
  q->lda_in = A.mat(N0, lda_dim);
  q->lda_out = A.mat(N0, lda_dim);
  q->X.resize(L + 1);
  q->carried_per_stream = q->hf;
  for (int l = 0; l <= L; l++) {
    const int h = l < L ? q->layers[l].hx : 0, m = l < L ? q->layers[l].mx : q->Tout;
    q->X[l] = A.mat((h + m) * B, Hd);
    carried(q->X[l], h, m, 1, Hd);
    q->carried_per_stream += h;
  }
  for (auto &Ly : q->layers) {
    Ly.Y = A.mat((Ly.hy + Ly.my) * B, Ly.bn);
    carried(Ly.Y, Ly.hy, Ly.my, Ly.rho, Ly.bn);
    q->carried_per_stream += Ly.hy;
    bn_max = std::max(bn_max, Ly.bn);
    if (Ly.rho > 1) lin_rows = std::max(lin_rows, Ly.my * B);
    if (Ly.s_out != Ly.ls) relu_rows = std::max(relu_rows, Ly.m_out * B);
  }
  q->lin_tmp = lin_rows ? A.mat(lin_rows, bn_max) : nullptr;
  q->relu_tmp = relu_rows ? A.mat(relu_rows, Hd) : nullptr;
  infer_head_layout(c, q->which, q->nbn, No, true, (size_t)kTab * B, A, &q->head);
  q->descs = A.take<CarryDesc>(q->host_descs.size() + 1);
  q->fdp = (c.feat_dim + 3) & ~3;
  q->tail_off = so;
  so += 2LL * q->hf * q->fdp;
  q->slot_floats = (so + 63) & ~63LL;
  q->state = A.take<float>((size_t)(q->slot_floats * B));
  q->carry_max = 0;
  for (auto &d : q->host_descs) q->carry_max = std::max(q->carry_max, (long long)d.h * (d.unit / 4));
}

// the model's true context in input frames: the lda splice and every layer's taps
void model_context(const std::vector<TdnnfLayer> &layers, int *left, int *right) {
  *left = *right = 1;
  for (auto &L : layers) {
    *left += L.left;
    *right += L.right;
  }
}

// Where a step of B active streams lives: [carried | new] rows of X[l] and Y[l], the GEMMs storing the new rows.  The buffers are the
// object's, so the description changes with B alone and is kept from one step to the next.
const FwdBuffers &step_buffers(tdnnf_online *q, int B) {
  FwdBuffers &b = q->fwd;
  if (q->fwd_B == B) return b;
  const tdnnf_net_config &c = q->model->cfg;
  const int Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  const int N0 = q->F * B, No = q->Tout * B, L = (int)q->layers.size(), ldH = ldpad(Hd);
  // the new rows of X[l]
  auto Xnew = [&](int l) {
    const int h = l < L ? q->layers[l].hx : 0, m = l < L ? q->layers[l].mx : q->Tout;
    return M(q->X[l] + (size_t)h * B * ldH, m * B, Hd);
  };
  b.lda_in = M(q->lda_in, N0, lda_dim);
  b.lda_out = M(q->lda_out, N0, lda_dim);
  b.x0 = Xnew(0);
  for (int l = 0; l < L; l++) {
    const tdnnf_online::Layer &Ly = q->layers[l];
    FwdLayer &f = b.layers[l];
    // time 0 = the first new row of X[l] and Y[l]; the layer's new output rows start at -b
    const Grid gx{-Ly.hx * Ly.ls, Ly.ls, Ly.hx + Ly.mx}, gy_new{0, Ly.ls, Ly.my}, gy{-Ly.hy * Ly.ls, Ly.ls, Ly.hy + Ly.my}, go{-Ly.b, Ly.s_out, Ly.m_out};
    layer_tdnns(q->model, l, gx, gy_new, gy, go, B, &f.lin, &f.aff);
    const tdnnf_mat ynew = M(Ly.Y + (size_t)Ly.hy * B * ldpad(Ly.bn), Ly.my * B, Ly.bn);
    f.lin_in = M(q->X[l], gx.n * B, Hd);
    // the .affine reads blocks of rho time steps: the new rows in plain order, then into the rho row order
    f.lin_out = Ly.rho > 1 ? M(q->lin_tmp, Ly.my * B, Ly.bn) : ynew;
    f.perm_out = ynew;
    f.aff_in = M(Ly.Y, gy.n * B, Ly.bn);
    f.byp = sub_grid_view(q->X[l], gx, go, B, Hd);
    f.out = Xnew(l + 1);
    f.relu = Ly.s_out != Ly.ls ? M(q->relu_tmp, f.aff.rows_out, Hd) : tdnnf_mat{nullptr, 0, 0, 0};
    f.out_times = Ly.m_out;
  }
  b.top = Xnew(L);
  b.pl = M(q->head.pl, No, S);
  b.b1 = M(q->head.b1, No, Hd);
  b.b2 = M(q->head.b2, No, S);
  b.y = M(q->head.y, No, P);
  b.lsm = M(q->head.lsm, No, P);
  b.row_map = q->head.row_map;
  q->fwd_B = B;
  return b;
}

int forward_step(tdnnf_online *q, const tdnnf_mat *feats, const tdnnf_mat *iv, int B, tdnnf_mat *out, hipStream_t s) {
  const tdnnf_net_config &c = q->model->cfg;
  const int lda_dim = 3 * c.feat_dim + c.ivector_dim, N0 = q->F * B, No = q->Tout * B;
  const int ndesc = (int)q->host_descs.size();
  const FwdBuffers &b = step_buffers(q, B);
  TDNNF_HIP(infer_bn_coef(q->bn, q->nbn, q->head.coef, s));
  // ---- every buffer's carried tail into its head
  if (ndesc) {
    hipLaunchKernelGGL(online_carry_kernel<false>, dim3(grid_for(q->carry_max * B, 256), ndesc), dim3(256), 0, s, q->descs, q->head.table, B, q->state, q->slot_floats);
    TDNNF_LAUNCH_CHECK();
  }
  // ---- input: carried frames + clamped windows + i-vectors, spliced for the lda layer in one pass (which also carries the frames on)
  {
    const MatView fv = view(feats), ivv = view(iv), ov = view(&b.lda_in);
    const bool v4 = vec4_ok(fv) && vec4_ok(ivv) && vec4_ok(ov);
    const long long work = ((long long)N0 * lda_dim + (long long)B * q->hf * c.feat_dim) / (v4 ? 4 : 1);
    if (v4) hipLaunchKernelGGL(online_gather_kernel<4>, dim3(grid_for(work, 256)), dim3(256), 0, s, fv, ivv, q->head.table, B, q->F, q->hf, q->state, q->slot_floats, q->tail_off, q->fdp, ov);
    else hipLaunchKernelGGL(online_gather_kernel<1>, dim3(grid_for(work, 256)), dim3(256), 0, s, fv, ivv, q->head.table, B, q->F, q->hf, q->state, q->slot_floats, q->tail_off, q->fdp, ov);
    TDNNF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(online_row_map_kernel, dim3((No + 255) / 256), dim3(256), 0, s, q->head.table, B, q->Tout, q->head.row_map);
  TDNNF_LAUNCH_CHECK();
  // ---- the schedule of infer_forward.hip on the new rows, in exact f32 (the kept rows go straight into the caller's output)
  FwdCounts cnt;
  CK(infer_forward(q->model, q->head.coef, q->which, B, b, out, infer_gemm_f32, const_cast<tdnnf_net *>(q->model), s, &cnt));
  // ---- the last h time rows of every buffer back to their slots
  if (ndesc) {
    hipLaunchKernelGGL(online_carry_kernel<true>, dim3(grid_for(q->carry_max * B, 256), ndesc), dim3(256), 0, s, q->descs, q->head.table, B, q->state, q->slot_floats);
    TDNNF_LAUNCH_CHECK();
  }
  q->gemm_rows = cnt.rows;
  q->carried_rows = (long long)q->carried_per_stream * B;
  q->fused = cnt.fused;
  q->fallback = cnt.fallback;
  return TDNNF_OK;
}

}  // namespace

extern "C" {

int tdnnf_online_create(const tdnnf_net *model, int frames_per_step, int num_slots, int which_output, tdnnf_online **out) {
  TDNNF_REQUIRE(model && out, "online_create: null argument");
  const tdnnf_net_config &c = model->cfg;
  CK(infer_check_model(c, frames_per_step, "online_create", "frames_per_step"));
  TDNNF_REQUIRE(num_slots >= 1 && which_output >= 0 && which_output <= 1, "online_create: num_slots must be >= 1, which_output 0 or 1");
  tdnnf_online *q = new tdnnf_online();
  q->model = model;
  q->F = frames_per_step;
  q->fsf = c.frame_subsampling;
  q->Tout = frames_per_step / c.frame_subsampling;
  q->num_slots = num_slots;
  q->which = which_output;
  q->fwd.layers.resize(c.num_layers);
  std::vector<TdnnfLayer> grids;
  Grid g_lda;
  int rc = net_layer_grids(c, q->Tout, grids, &g_lda);  // (for the steps, which do not depend on the width)
  if (rc == TDNNF_OK && g_lda.step != 1) {
    set_error("online_create: the first tdnnf layers must run at the input frame rate");
    rc = TDNNF_EINVAL;
  }
  if (rc != TDNNF_OK) {
    delete q;
    return rc;
  }
  model_context(grids, &q->left, &q->right);
  q->D = round_up(q->right, q->fsf);
  q->W = round_up(q->left, q->F);
  q->hf = q->D - q->right + 2;
  for (auto &G : grids) {
    tdnnf_online::Layer Ly;
    Ly.a = G.left;
    Ly.b = G.right;
    Ly.bn = G.bn;
    Ly.ls = G.glin.step;
    Ly.s_out = G.gout.step;
    Ly.rho = Ly.s_out / Ly.ls;
    Ly.hx = std::max(Ly.a, Ly.b) / Ly.ls;
    Ly.mx = Ly.my = q->F / Ly.ls;
    Ly.hy = round_up(Ly.b / Ly.ls, Ly.rho);
    Ly.m_out = q->F / Ly.s_out;
    Ly.Y = nullptr;
    q->layers.push_back(Ly);
  }
  q->nbn = infer_bn_table(model, which_output, &q->bn);
  Arena sizing;
  layout(q, sizing);
  const size_t bytes = sizing.off + 1024;
  if (hipMalloc((void **)&q->arena, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("online_create: cannot allocate %zu bytes of activations and state", bytes);
    delete q;
    return TDNNF_EHIP;
  }
  Arena real;
  real.base = q->arena;
  layout(q, real);
  hipError_t e = hipMemset(q->arena, 0, bytes);
  if (e == hipSuccess && !q->host_descs.empty())
    e = hipMemcpy(q->descs, q->host_descs.data(), sizeof(CarryDesc) * q->host_descs.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the first step may come on any stream)
  if (e != hipSuccess) {
    hipFree(q->arena);
    delete q;
    return hip_status(e, "online_create: initialising the arena");
  }
  q->slots.assign(num_slots, tdnnf_online::Slot{-q->W, -1, 0});
  *out = q;
  return TDNNF_OK;
}

void tdnnf_online_destroy(tdnnf_online *q) {
  if (!q) return;
  hipFree(q->arena);
  delete q;
}

int tdnnf_online_context(const tdnnf_online *q, int *left, int *right, int *latency) {
  TDNNF_REQUIRE(q, "online_context: null argument");
  if (left) *left = q->left;
  if (right) *right = q->right;
  if (latency) *latency = q->D;
  return TDNNF_OK;
}

int tdnnf_online_reset(tdnnf_online *q, int slot, tdnnf_stream stream) {
  TDNNF_REQUIRE(q && slot >= 0 && slot < q->num_slots, "online_reset: slot %d out of range (num_slots %d)", slot, q ? q->num_slots : 0);
  TDNNF_HIP(hipMemsetAsync(q->state + (size_t)slot * q->slot_floats, 0, sizeof(float) * q->slot_floats, (hipStream_t)stream));
  q->slots[slot] = tdnnf_online::Slot{-q->W, -1, 0};
  return TDNNF_OK;
}

int tdnnf_online_slot(const tdnnf_online *q, int slot, int *clock, int *frames) {
  TDNNF_REQUIRE(q && slot >= 0 && slot < q->num_slots, "online_slot: slot %d out of range (num_slots %d)", slot, q ? q->num_slots : 0);
  if (clock) *clock = q->slots[slot].clock;
  if (frames) *frames = q->slots[slot].T;
  return TDNNF_OK;
}

int tdnnf_online_schedule(int frames_per_step, int frame_subsampling, int left, int right, int frames, int *steps_out, int capacity, int *num_steps) {
  const int F = frames_per_step, fsf = frame_subsampling;
  TDNNF_REQUIRE(num_steps && capacity >= 0 && (steps_out || capacity == 0), "online_schedule: bad arguments");
  TDNNF_REQUIRE(fsf >= 1 && F > 0 && F % fsf == 0, "online_schedule: frames_per_step %d must be a positive multiple of frame_subsampling %d", F, fsf);
  TDNNF_REQUIRE(left >= 0 && right >= 0 && frames >= 1, "online_schedule: left and right context must be >= 0, the utterance at least one frame");
  const int D = round_up(right, fsf), W = round_up(left, F);
  int ns = 0;
  for (long long clock = -W; clock - D < frames; clock += F, ns++) {
    if (ns < capacity) online_window(F, fsf, D, (int)clock, frames, steps_out + 5 * ns);
  }
  *num_steps = ns;
  TDNNF_REQUIRE(ns <= capacity, "online_schedule: %d steps, capacity %d", ns, capacity);
  return TDNNF_OK;
}

int tdnnf_online_step(tdnnf_online *q, int num_active, const int *slots_host, const int *rows_host, const int *final_host, const tdnnf_mat *feats,
                      const tdnnf_mat *ivectors, tdnnf_mat *out, int *out_first_host, int *out_count_host, tdnnf_stream stream) {
  TDNNF_REQUIRE(q && num_active >= 0 && (num_active == 0 || (slots_host && rows_host && final_host && out_first_host && out_count_host)),
                "online_step: bad arguments");
  TDNNF_REQUIRE(mat_ok(feats) && mat_ok(ivectors) && mat_ok(out), "online_step: bad matrices");
  const tdnnf_net *n = q->model;
  TDNNF_REQUIRE(n->params, "online_step: the model net has no parameter buffer (net_set_buffers)");
  const tdnnf_net_config &c = n->cfg;
  const int B = num_active, F = q->F;
  TDNNF_REQUIRE(B <= q->num_slots, "online_step: %d active streams, %d slots", B, q->num_slots);
  // ---- every check before any launch: a failing call leaves every slot as it was
  std::vector<int> newT(B), seen(q->num_slots, 0);
  q->host_table.resize((size_t)kTab * std::max(B, 1));
  long long sum = 0;
  for (int i = 0; i < B; i++) {
    const int sl = slots_host[i], nb = rows_host[i], fin = final_host[i] != 0;
    TDNNF_REQUIRE(sl >= 0 && sl < q->num_slots, "online_step: slot %d out of range (num_slots %d)", sl, q->num_slots);
    TDNNF_REQUIRE(!seen[sl], "online_step: slot %d is listed twice", sl);
    seen[sl] = 1;
    const tdnnf_online::Slot &st = q->slots[sl];
    int T = st.T;
    if (T >= 0) {
      TDNNF_REQUIRE(nb == 1 && fin, "online_step: slot %d has seen its last frame: a flush window passes that frame alone with final set (got %d rows, final %d)", sl, nb, fin);
    } else if (st.clock < 0) {
      TDNNF_REQUIRE(nb == 1 && !fin, "online_step: slot %d is warming up (clock %d): its window passes frame 0 alone, not final (got %d rows, final %d)", sl, st.clock, nb, fin);
    } else if (fin) {
      TDNNF_REQUIRE(nb >= 1 && nb <= F, "online_step: slot %d: the window in which the utterance ends passes 1..%d rows (got %d)", sl, F, nb);
      T = st.clock + nb;
    } else {
      TDNNF_REQUIRE(nb == F, "online_step: slot %d: a window that is not final passes exactly %d rows (got %d)", sl, F, nb);
    }
    int v[5];
    online_window(F, q->fsf, q->D, st.clock, T, v);
    TDNNF_REQUIRE(v[2] == nb, "online_step: slot %d: the window at clock %d passes %d rows (got %d)", sl, st.clock, v[2], nb);
    newT[i] = T;
    out_first_host[i] = v[3];
    out_count_host[i] = v[4];
    int *t = &q->host_table[(size_t)kTab * i];
    t[0] = sl;
    t[1] = (int)sum;
    t[2] = nb;
    t[3] = st.parity;
    t[4] = (st.clock - q->D) / q->fsf;
    t[5] = T < 0 ? INT_MAX : (T + q->fsf - 1) / q->fsf;
    sum += nb;
  }
  TDNNF_REQUIRE(feats->rows == sum && feats->cols == c.feat_dim, "online_step: feats must be %lld x %d (the passed rows of the active streams stacked)", sum, c.feat_dim);
  TDNNF_REQUIRE(ivectors->rows == B && ivectors->cols == c.ivector_dim, "online_step: ivectors must be %d x %d (one row per active stream)", B, c.ivector_dim);
  TDNNF_REQUIRE(out->rows == (long long)B * q->Tout && out->cols == c.num_pdfs, "online_step: out must be %d x %d (%d rows per active stream)", B * q->Tout, c.num_pdfs, q->Tout);
  q->gemm_rows = q->carried_rows = 0;
  q->fused = q->fallback = 0;
  if (B == 0) return TDNNF_OK;
  hipStream_t s = (hipStream_t)stream;
  TDNNF_HIP(hipMemcpyAsync(q->head.table, q->host_table.data(), sizeof(int) * kTab * B, hipMemcpyHostToDevice, s));
  CK(forward_step(q, feats, ivectors, B, out, s));
  for (int i = 0; i < B; i++) {
    tdnnf_online::Slot &st = q->slots[slots_host[i]];
    st.clock += F;
    st.T = newT[i];
    st.parity ^= 1;
  }
  return TDNNF_OK;
}

int tdnnf_online_counts(const tdnnf_online *q, long long *gemm_rows, long long *carried_rows, int *fused, int *fallback) {
  TDNNF_REQUIRE(q, "online_counts: null argument");
  if (gemm_rows) *gemm_rows = q->gemm_rows;
  if (carried_rows) *carried_rows = q->carried_rows;
  if (fused) *fused = q->fused;
  if (fallback) *fallback = q->fallback;
  return TDNNF_OK;
}

}  // extern "C"
