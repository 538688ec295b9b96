// align_build.hip -- launches the device build of a reserved tdnnf_align_graphs (align_build_kernels.h) for tdnnf_align_graphs_assign
// (align_graphs.hip): three launches on the caller's stream, nothing allocated, nothing waited for.
#include "align_build_kernels.h"

namespace tdnnf {

// b: the handle's tables and scratch with this batch's staged arrays and G filled in.  max_graph_arcs, max_graph_rows: the largest graph's,
// which size the fill's grid.
int align_build_launch(const AlignBuildDev &b, int max_graph_arcs, int max_graph_rows, hipStream_t s) {
  hipLaunchKernelGGL(align_build_rows_kernel, dim3(b.G, b.num_tables), dim3(kBuildThreads), 0, s, b);
  TDNNF_LAUNCH_CHECK();
  hipLaunchKernelGGL(align_build_offsets_kernel, dim3(b.num_tables), dim3(kBuildThreads), 0, s, b);
  TDNNF_LAUNCH_CHECK();
  const int work = std::max(max_graph_arcs, max_graph_rows + 63);
  const int parts = std::min(std::max((work + 4 * kBuildThreads - 1) / (4 * kBuildThreads), 1), 64);
  hipLaunchKernelGGL(align_build_fill_kernel, dim3(b.G, b.num_tables, parts), dim3(kBuildThreads), 0, s, b);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // namespace tdnnf
