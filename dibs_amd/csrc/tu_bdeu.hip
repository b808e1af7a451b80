// translation unit: the BDeu node-score kernel and its launcher (kernels_bdeu.h)
#include "launch.h"

// `a` as the caller filled it (data, tables, masks, output, sizes); the LDS plan's fields (T, waves, *_bytes) are set here from
// bdeu_plan(N, KW), which dibs_engine_create / dibs_engine_set_data / dibs_score_graphs have checked to exist.  Returns 1 without a plan.
int bdeu_launch_nodes(hipStream_t stream, BdeuArgs a) {
  BdeuPlan pl;
  if (!bdeu_plan(a.N, a.KW, &pl)) return 1;
  a.T = pl.T;
  a.waves = pl.waves;
  a.wave_bytes = (uint32_t)pl.wave_bytes;
  a.rows_bytes = (uint32_t)pl.rows_bytes;
  if (a.nprob <= 0) return 0;
  // persistent blocks: what is resident at this LDS size (at most eight waves per SIMD), grid-strided over the problems
  long long per_cu = (long long)(((size_t)160 * 1024) / pl.lds_bytes);
  if (per_cu * pl.waves > 32) per_cu = 32 / pl.waves;
  if (per_cu < 1) per_cu = 1;
  long long blocks = (a.nprob + pl.waves - 1) / pl.waves;
  const long long resident = per_cu * dibs_cu_count();
  if (blocks > resident) blocks = resident;
  if (pl.rows_lds) {
    allow_lds(k_bdeu_nodes<true>, pl.lds_bytes);
    hipLaunchKernelGGL(k_bdeu_nodes<true>, dim3((unsigned)blocks), dim3(64 * pl.waves), pl.lds_bytes, stream, a);
  } else {
    allow_lds(k_bdeu_nodes<false>, pl.lds_bytes);
    hipLaunchKernelGGL(k_bdeu_nodes<false>, dim3((unsigned)blocks), dim3(64 * pl.waves), pl.lds_bytes, stream, a);
  }
  return 0;
}
