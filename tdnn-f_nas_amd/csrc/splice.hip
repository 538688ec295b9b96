// splice.hip -- two row-gather ops of the input side, stand-alone (no net object): the spliced lda input of the trainer
// (tdnnf_splice_input) and the rho row order a TdnnComponent with row_stride > 1 reads (tdnnf_reorder_rows,
// TdnnComponent::ReorderIndexes).
#include "common.h"

namespace tdnnf {
namespace {

// lda input: [feats(k+j, b), j < S ; ivector(b)]
__global__ void splice_input_kernel(MatView feats, MatView iv, int B, int S, MatView out) {
  const int C = out.cols, fd = feats.cols;
  const long long total = (long long)out.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C), k = r / B, b = r % B;
    float v;
    if (c < S * fd) v = feats.data[(size_t)((k + c / fd) * B + b) * feats.stride + c % fd];
    else v = iv.data[(size_t)b * iv.stride + (c - S * fd)];
    out.data[(size_t)r * out.stride + c] = v;
  }
}
__global__ void reorder_rows_kernel(MatView in, int B, int rho, int to_rho, MatView out) {
  const int C = in.cols;
  const long long total = (long long)in.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C);
    const int tau = r / B, b = r % B;  // plain t-major coordinates
    const int pr = (tau / rho) * rho * B + b * rho + tau % rho;
    if (to_rho) out.data[(size_t)pr * out.stride + c] = in.data[(size_t)r * in.stride + c];
    else out.data[(size_t)r * out.stride + c] = in.data[(size_t)pr * in.stride + c];
  }
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_splice_input(const tdnnf_mat *feats, const tdnnf_mat *iv, int B, int S, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(feats) && mat_ok(iv) && mat_ok(out) && B > 0 && S > 0, "splice_input: bad arguments");
  TDNNF_REQUIRE(out->rows % B == 0 && feats->rows == (out->rows / B + S - 1) * B && iv->rows == B &&
                    out->cols == S * feats->cols + iv->cols,
                "splice_input: feats must have out_frames + num_splice - 1 time steps and out.cols = S*feat_dim + ivector_dim");
  if (out->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(splice_input_kernel, dim3(grid_for((long long)out->rows * out->cols, 256)), dim3(256), 0, (hipStream_t)stream,
                     view(feats), view(iv), B, S, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_reorder_rows(const tdnnf_mat *in, int B, int rho, int to_rho, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && same_dim(in, out) && B > 0 && rho >= 1 && in->rows % (B * rho) == 0 && in->data != out->data,
                "reorder_rows: rows must be a multiple of num_seq*rho and in != out");
  if (in->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(reorder_rows_kernel, dim3(grid_for((long long)in->rows * in->cols, 256)), dim3(256), 0, (hipStream_t)stream,
                     view(in), B, rho, to_rho, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // extern "C"
