// translation unit: k_particle_grad_edge, the per-particle tail (kernels_tail.h) under the edge-wise graph prior (include/dibs_hip.h,
// dibs_engine_set_edge_prior), and its launcher.  The block is the source text of k_particle_grad compiled a second time with the
// TAIL_TAB_* macros filled in; a unit of its own, so that engine_step.hip and tu_batch.hip compile what they compiled without it.
#define DIBS_TU_TAIL_EDGE
#include "engine_impl.h"

void edge_launch_tail(hipStream_t st, const TailArgs& ta, const float* tab, int blocks, size_t lds) {
  dibs_allow_lds((const void*)k_particle_grad_edge, lds);
  hipLaunchKernelGGL(k_particle_grad_edge, dim3(blocks), dim3(TAIL_NT), lds, st, ta, tab);
}
