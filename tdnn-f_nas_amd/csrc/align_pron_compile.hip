// align_pron_compile.hip -- launches the pronunciation compile of a reserved tdnnf_align_graphs (align_pron_compile_kernels.h) for
// tdnnf_align_graphs_assign_pronunciations (align_graphs.hip): one launch on the caller's stream in front of the device build, nothing
// allocated, nothing waited for.
#include "align_pron_compile_kernels.h"

namespace tdnnf {

// c: the batch's staged tables and begins, the arrays to write and the unit set's tables.  G: the transcripts.
int align_pron_compile_launch(const AlignPronCompileDev &c, int G, hipStream_t s) {
  hipLaunchKernelGGL(align_pron_compile_kernel, dim3(G), dim3(kBuildThreads), 0, s, c);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // namespace tdnnf
