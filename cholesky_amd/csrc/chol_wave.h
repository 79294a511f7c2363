// Lane-level helpers shared by the factor's kernels (chol_kernels.hip) and the streamed solve (chol_solve.hip): device code,
// included by .hip files only.
#ifndef CHOL_WAVE_H
#define CHOL_WAVE_H
#include <hip/hip_runtime.h>

typedef double d4 __attribute__((ext_vector_type(4)));

// workgroup barrier that orders LDS traffic only (global loads / stores stay in flight across it)
__device__ __forceinline__ void lds_barrier()
{
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}


// Data handed from one workgroup to another INSIDE a launch (fused POTRF+TRSM+update launch) is written with
// agent-scope stores (write-through, device-coherent) and read with agent-scope loads, so that it is seen across
// the XCDs' L2s while the kernel runs; PUB = false is a plain access.
template <bool PUB> __device__ __forceinline__ void gstore(double *p, double v)
{
  if (PUB) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
template <bool PUB> __device__ __forceinline__ double gload(const double *p)
{
  if (PUB) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

#define TS 16

__device__ __forceinline__ double readlane_f64(double v, int l)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// broadcast of quad-lane I inside every quad (4 consecutive lanes), DPP quad_perm
template <int I> __device__ __forceinline__ double quad_bcast(double v)
{
  constexpr int ctrl = I | (I << 2) | (I << 4) | (I << 6);
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// 1/sqrt(d) to fp64 accuracy.  Measured on gfx950: the v_rsq_f64 seed is good to 5.2e-8, one Newton step
// leaves 4e-15 (36 ulp), two reach 1.4e-16.  A lone wave issues one DP instruction per ~11 cycles
// (scripts/dp_lat.hip), so the pivot chain is bound by its DP instruction COUNT: one third-order step
//   e = 1 - d y^2,  y <- y (1 + e/2 + 3 e^2/8)        (error ~ e^3 = 1e-22)
// costs 5 DP instructions against 7 for two Newton steps.
__device__ __forceinline__ double rsqrt_nr(double d)
{
  const double y = __builtin_amdgcn_rsq(d);
  const double e = fma(-(d * y), y, 1.0);
  const double q = e * fma(0.375, e, 0.5);
  return fma(y, q, y);
}

// acc += m[lane K of this lane's 16-lane row] * nt: the multiplier of a column step straight out of the lane that holds it (DPP
// row_newbcast, the one DPP form double-precision instructions take).  hipcc pads no hazards inside an asm statement: a VGPR written
// by the VALU needs two wait states before a DPP instruction reads it as its shuffled operand -- the first use of m in a column step
// carries them (m may have been produced by a compiler-inserted copy just ahead of the statement)
template <int K, bool FIRST> __device__ __forceinline__ void fmac_bcast(double &acc, double m, double nt)
{
  if (FIRST) asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(m), "v"(nt), "n"(K));
  else asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(m), "v"(nt), "n"(K));
}

// Inverses of the four 4x4 diagonal blocks, one block per quad.  Lane r15 = 4 b + i holds
// blk[k] = L(4b+i, 4b+k) and invd = 1 / L(4b+i, 4b+i).  On exit x[m] = Linv_bb(m, i): the lane owns
// column i of its block's inverse.
__device__ __forceinline__ void linv4_quad(const double (&blk)[4], double invd, double (&x)[4], int qi)
{
  const double inv0 = quad_bcast<0>(invd), inv1 = quad_bcast<1>(invd), inv2 = quad_bcast<2>(invd), inv3 = quad_bcast<3>(invd);
  const double l10 = quad_bcast<1>(blk[0]);
  const double l20 = quad_bcast<2>(blk[0]), l21 = quad_bcast<2>(blk[1]);
  const double l30 = quad_bcast<3>(blk[0]), l31 = quad_bcast<3>(blk[1]), l32 = quad_bcast<3>(blk[2]);
  x[0] = (qi == 0) ? inv0 : 0.0;
  x[1] = (qi == 1) ? inv1 : -(l10 * x[0]) * inv1;
  x[2] = (qi == 2) ? inv2 : -fma(l21, x[1], l20 * x[0]) * inv2;
  x[3] = (qi == 3) ? inv3 : -fma(l32, x[2], fma(l31, x[1], l30 * x[0])) * inv3;
}

// X = T L^-T for a 16x16 tile T in accumulator layout.  Lr[b] = L(r15, 4b + g), b = 0..2 (register b
// of the diagonal block in tile layout), yd = Ydiag(c = r15, k = g).
__device__ __forceinline__ d4 tile_solve(d4 t, const double (&Lr)[3], double yd)
{
  const d4 z = { 0.0, 0.0, 0.0, 0.0 };
  d4 x, s, u;
  s = __builtin_amdgcn_mfma_f64_16x16x4f64(yd, t[0], z, 0, 0, 0);
  x[0] = s[0];
  u = __builtin_amdgcn_mfma_f64_16x16x4f64(Lr[0], -x[0], t, 0, 0, 0);
  s = __builtin_amdgcn_mfma_f64_16x16x4f64(yd, u[1], z, 0, 0, 0);
  x[1] = s[1];
  u = __builtin_amdgcn_mfma_f64_16x16x4f64(Lr[1], -x[1], u, 0, 0, 0);
  s = __builtin_amdgcn_mfma_f64_16x16x4f64(yd, u[2], z, 0, 0, 0);
  x[2] = s[2];
  u = __builtin_amdgcn_mfma_f64_16x16x4f64(Lr[2], -x[2], u, 0, 0, 0);
  s = __builtin_amdgcn_mfma_f64_16x16x4f64(yd, u[3], z, 0, 0, 0);
  x[3] = s[3];
  return x;
}

// Linv(k,k) for the TRSM kernels, off every critical path: X = I L^-T = Linv^T by one tile_solve, stored
// as Wb[k * 16 + c] = Linv(c, k) -- the layout solve16() reads as its MFMA Y operand.
__device__ __forceinline__ void store_linv16(double *Wb, const double (&Lr)[3], double yd, int r15, int g)
{
  d4 id;
  int rr = r15;
  asm volatile("" : "+v"(rr)); // built where it is used: a hoisted identity tile costs 8 registers in the callers' loops
#pragma unroll
  for (int q = 0; q < 4; ++q) id[q] = (rr == g + 4 * q) ? 1.0 : 0.0;
  const d4 xi = tile_solve(id, Lr, yd); // xi(r, c) = Linv(c, r)
#pragma unroll
  for (int q = 0; q < 4; ++q) Wb[r15 * TS + g + 4 * q] = xi[q];
}
#endif
