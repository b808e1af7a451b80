// What the host's schedule (step_plan.h) shares with the kernel-matrix kernels (kernels_kmat.h): three sizes and the two counting rules of
// the tiled kernel.  Nothing of HIP beyond the function qualifiers, which a host-only program compiles without.
#pragma once
#define KT_CH 256      // tiled kernel: elements of a row per chunk (kmat_nchunk)
#define KT_T 32        // tiled kernel: tile edge (particles)
#define KMAT_CH 32768  // direct kernel: floats of z_a staged in LDS at a time (128 KiB); longer vectors (DenseNN theta at d = 100) go in chunks
#ifdef __HIPCC__
#define KMAT_HD __host__ __device__
#else
#define KMAT_HD
#endif
KMAT_HD inline int kmat_tile_count(int nta, int ntb, int symmetric) { return symmetric ? nta * (nta + 1) / 2 : nta * ntb; }
KMAT_HD inline int kmat_nchunk(int len) { return (len + KT_CH - 1) / KT_CH; }
