// translation unit: the float64 engine's kernels (kernels_f64.h) and their launchers; compiled with -ffp-contract=off (Makefile)
#include "launch.h"
#include "kernels_f64.h"

void f64_launch_edge(hipStream_t st, const F64Args& a) { hipLaunchKernelGGL(k64_edge, dim3(a.M), dim3(256), 0, st, a); }

void f64_launch_bge(hipStream_t st, const F64Args& a) {
  const size_t lds = 4 * f64_bge_wave_bytes(a.d);
  allow_lds(k64_bge, lds);
  hipLaunchKernelGGL(k64_bge, dim3((a.d + 3) / 4, a.M), dim3(256), lds, st, a);
}

void f64_launch_weights(hipStream_t st, const F64Args& a) {
  const size_t lds = (size_t)2 * a.S * 8;
  allow_lds(k64_weights, lds);
  hipLaunchKernelGGL(k64_weights, dim3(a.M), dim3(256), lds, st, a);
}

void f64_launch_acyc(hipStream_t st, const F64Args& a) {
  const size_t lds = f64_acyc_lds_bytes(a.dpad);
  allow_lds(k64_acyc, lds);
  hipLaunchKernelGGL(k64_acyc, dim3(a.Sa, a.M), dim3(256), lds, st, a);
}

void f64_launch_acyc_reduce(hipStream_t st, const F64Args& a) { hipLaunchKernelGGL(k64_acyc_reduce, dim3(a.M), dim3(256), 0, st, a); }

void f64_launch_grad(hipStream_t st, const F64Args& a) {
  const size_t lds = (size_t)(a.d * a.d + a.d) * 8;
  allow_lds(k64_grad, lds);
  hipLaunchKernelGGL(k64_grad, dim3(a.M), dim3(256), lds, st, a);
}

void f64_launch_kmat(hipStream_t st, const F64Args& a) { hipLaunchKernelGGL(k64_kmat, dim3(a.M), dim3(256), 0, st, a); }

void f64_launch_phi(hipStream_t st, const F64Args& a) {
  hipLaunchKernelGGL(k64_phi, dim3((unsigned)((a.D + 255) / 256), a.M), dim3(256), 0, st, a);
}

void f64_launch_update(hipStream_t st, const F64Args& a) {
  const size_t n = (size_t)a.M * a.D;
  hipLaunchKernelGGL(k64_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
}
