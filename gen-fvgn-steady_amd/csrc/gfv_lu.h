// The M x M LU of the WLSQ systems: what csrc/fvm.hip (the reconstruction and its adjoint) and csrc/wallforce.hip (the body
// nodes' gradients, kept in double) share.  Device inline functions only.
#pragma once
#include "gfv_common.h"

// ---- M x M LU with partial pivoting (LAPACK getf2 order), solve and transpose-solve; M = Taylor terms of the WLSQ
// reconstruction order: 2 (1st), 5 (2nd, the default), 9 (3rd), 14 (4th) (FVorder.py:23-72) ------------------------------
//
// The factorisation and the two triangular solves run in DOUBLE.  The moment matrices of stretched cells are badly
// conditioned (boundary-layer nodes of mesh_example/airfoil_L=1: cond(A_n) = 4e5), where ANY fp32 elimination returns
// rounding noise of size cond * 2^-24 - the reference's LAPACK call, an FMA build of the same loop and this kernel's former
// fp32 loop land 0.009, 0.17 and 1.7 away from the exact gradient 1833 at such a node (profiles/r03_wlsq_conditioning.txt).
// Solving the system exactly (right-hand side accumulated in double from the fp32 data, A normalised in double) puts the
// result in the middle of that noise ball: its distance to the reference's value is the reference's own rounding error.
typedef double lu_t;
template <int M>
struct LU {
  lu_t a[M][M];
  int piv[M];
};

template <int M>
__device__ __forceinline__ void lu_factor(LU<M>& m) {
#pragma unroll
  for (int k = 0; k < M; ++k) {
    int p = k;
    lu_t mx = fabs(m.a[k][k]);
#pragma unroll
    for (int r = k + 1; r < M; ++r) {
      const lu_t v = fabs(m.a[r][k]);
      if (v > mx) { mx = v; p = r; }
    }
    m.piv[k] = p;
    // row swap with static register indices (a[p][c] with a run-time p would put the matrix in scratch memory)
#pragma unroll
    for (int r = k + 1; r < M; ++r) {
      const bool sw = (p == r);
#pragma unroll
      for (int c = 0; c < M; ++c) {
        const lu_t tk = m.a[k][c], tr = m.a[r][c];
        m.a[k][c] = sw ? tr : tk;
        m.a[r][c] = sw ? tk : tr;
      }
    }
    const lu_t inv = 1.0 / m.a[k][k];
#pragma unroll
    for (int r = k + 1; r < M; ++r) {
      m.a[r][k] *= inv;
#pragma unroll
      for (int c = k + 1; c < M; ++c) m.a[r][c] -= m.a[r][k] * m.a[k][c];
    }
  }
}

template <int M>
__device__ __forceinline__ void lu_solve(const LU<M>& m, lu_t (&b)[M]) {
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const int p = m.piv[k];
#pragma unroll
    for (int r = k + 1; r < M; ++r) {
      const bool sw = (p == r);
      const lu_t tk = b[k], tr = b[r];
      b[k] = sw ? tr : tk;
      b[r] = sw ? tk : tr;
    }
  }
#pragma unroll
  for (int k = 0; k < M; ++k)
#pragma unroll
    for (int r = k + 1; r < M; ++r) b[r] -= m.a[r][k] * b[k];
#pragma unroll
  for (int k = M - 1; k >= 0; --k) {
    b[k] /= m.a[k][k];
#pragma unroll
    for (int r = 0; r < k; ++r) b[r] -= m.a[r][k] * b[k];
  }
}

// A_n = A / (row norm + 1e-8) (FVgrad.py:335-336), formed in double from the moment matrix as the reference stores it
template <int M>
__device__ __forceinline__ void load_An(const float* A, const float* rn, int i, LU<M>& m) {
  const float* p = A + (size_t)i * (M * M);
#pragma unroll
  for (int r = 0; r < M; ++r) {
    const lu_t inv = 1.0 / (lu_t)rn[(size_t)i * M + r];
#pragma unroll
    for (int c = 0; c < M; ++c) m.a[r][c] = (lu_t)p[M * r + c] * inv;
  }
}
