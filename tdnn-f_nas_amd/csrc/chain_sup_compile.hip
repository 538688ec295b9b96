// chain_sup_compile.hip -- launches the alignment compile of a reserved time-synchronous tdnnf_supervision (chain_sup_compile_kernels.h)
// for tdnnf_supervision_assign_alignments (chain_sup_build.hip): one launch on the caller's stream in front of the device build, nothing
// allocated, nothing waited for.
#include "chain_sup_compile_kernels.h"

namespace tdnnf {

// c: the minibatch's staged units, windows and begins, the arrays to write and the unit set's tables.
int sup_compile_launch(const SupCompileDev &c, hipStream_t s) {
  hipLaunchKernelGGL(sup_compile_kernel, dim3(c.B), dim3(kBuildThreads), 0, s, c);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // namespace tdnnf
