// dx_dls.hip -- object Jacobians and the batched damped-least-squares Cartesian-to-joint
// velocity mapper for CDNA4 (gfx950).
//
// Reference: dexterity/controllers/dls/dls.py:43-77
// (DampedLeastSquaresMapper.compute_joint_velocities), controllers/mapper.py:57-81 (bodies,
// geoms and sites) and utils/mujoco_utils.py:38-73 (compute_object_6d_jacobian =
// mj_jacBody / mj_jacGeom / mj_jacSite [3P]).
//
// The host resolves every controlled object to a point fixed to a body (dx_internal.h
// DlsDev); one 64-lane workgroup serves one environment.  It recomputes kinematics + com
// positions from the env's qpos (the tree passes of the step kernel, dx_device.h), stacks
// the n3 = 3 * npoint translational Jacobian rows J [n3][nv] in LDS (dx_jac.h) and maps
// the stacked target velocities V to
//     qdot = J^T (J J^T + reg I)^-1 V,
// which is dls.py:69-74's (J^T J + reg I) qdot = J^T V by the push-through identity (the
// header of dx_ik.hip), and for reg = 0 and a J of full row rank the minimum-norm solution
// np.linalg.lstsq returns (dls.py:75-77).  H = J J^T + reg I is one 32 x 32 accumulator
// tile of v_mfma_f32_32x32x2_f32 (ceil(nv / 2) k steps, identity padding past n3); the
// solve is mfma_chol_solve32, as in the IK kernel.
//
// Refinement: H and its factor are fp32, so a bare solve is off by about cond(H) * eps_fp32
// (1e-4 at reg = 0 on the shipped hands).  One step of iterative refinement follows, with
// the residual V - J (J^T y) - reg y taken in fp64 from J itself (2 * n3 * nv fp64 FMAs over
// the wave) and solved with the same fp32 factorisation; qdot = J^T (y + dy) is summed in
// fp64 and rounded once.  What is left is the error the fp32 Jacobian itself carries.
//
// Rank guard: the factorisation's pivots are checked first on the tile itself
// (mfma_chol_pivots32).  A pivot <= eps_fp32 * max(n3, nv) * max_i H_ii -- numpy's
// rcond = eps * max(M, N) numerical-rank rule, applied to the Gram matrix's pivots --
// marks the env rank-deficient: status 1 and a zero row, where lstsq would return a
// least-squares solution.
#include "dx_jac.h"

// mapper block in LDS (words), appended after the model's own layout at P.blk
struct DlsLds {
  int J, H, T, y, r, pt, w, total;
};
__host__ __device__ inline DlsLds dls_lds(int blk, int nv) {
  DlsLds k;
  int o = blk;
  k.J = o;  o += 32 * nv;  // stacked Jacobian rows [3 * npoint][nv]; rows up to 32 stay zero
  k.H = o;  o += 528;      // packed lower triangle of J J^T + reg I (ti(32)), kept for both solves
  k.T = o;  o += 528;      // Cholesky scratch
  k.y = o;  o += 32;       // target velocities -> multipliers
  k.r = o;  o += 32;       // fp64 residual, rounded -> the multipliers' correction
  k.pt = o; o += 32;       // point positions at the current qpos
  o = (o + 1) & ~1;
  k.w = o;  o += 2 * DX_MAX_NV;  // J^T y in fp64 (8-byte aligned)
  k.total = o;
  return k;
}
int dx_dls_lds_words(const DevModel& d) { return dls_lds(0, d.nv).total; }

// the launch's points (kernel arguments)
struct ArgPoints {
  const DlsDev& P;
  __device__ __forceinline__ int body(int s) const { return P.body[s]; }
  __device__ __forceinline__ const float* off(int s) const { return P.off + 3 * s; }
};

// H = J J^T + reg I on the matrix cores, as the padded 32 x 32 tile mfma_chol_solve32
// factors (lane l, VGPR v: H[8 (v/4) + 4 (l/32) + v%4][l%32]; rows and columns past n3
// are the identity).  k step s: lane l supplies A[l%32][l/32] = B[l/32][l%32] =
// J[l%32][2 s + l/32] -- B = A^T is the same operand (pgs_gram64's single-tile case).
// J's rows n3..31 are zero in LDS; a column past nv (odd nv) is masked.
__device__ __forceinline__ dx_f16v dls_gram32(const float* J, int n3, int nv, float reg) {
  const int l = LANE;
  const int j = l & 31, hi = l >> 5;
  dx_f16v C;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int i = 8 * (v >> 2) + 4 * hi + (v & 3);
    C[v] = i == j ? (i < n3 ? reg : 1.f) : 0.f;
  }
  const float* row = J + j * nv;
  for (int s = 0; 2 * s < nv; s++) {
    const int col = 2 * s + hi;
    const float e = row[min(col, nv - 1)];
    const float a = col < nv ? e : 0.f;
    C = __builtin_amdgcn_mfma_f32_32x32x2f32(a, a, C, 0, 0, 0);
  }
  return C;
}

// mode 0: the joint velocities of env blockIdx at its current qpos;
// mode 1: the object Jacobians of env blockIdx at its current qpos.
extern "C" __global__ void __launch_bounds__(64) dx_dls_kernel(const DevModel* __restrict__ mp, DevBatch B, Lds L, DlsDev P) {
  extern __shared__ float smem[];
  const DevModel& m = *(const DevModel*)(const DXG DevModel*)mp;
  const int env = (int)blockIdx.x;
  if (env >= B.nenv) return;
  CtxT<SpecRT> c(m, L, smem, nullptr, nullptr);
  c.I = (int*)(smem + L.ints);
  const DlsLds K = dls_lds(P.blk, m.nv);
  // J's rows past n3 feed the Gram tile as zeros, and the Cholesky solve reads padding
  // words of its packed triangles (times exact zeros)
  for (int k = LANE; k < K.total; k += DX_WAVE) smem[k] = 0.f;
  SYNC();
  const int nv = m.nv, n3 = 3 * P.npoint;
  float* qpos = c.f(L.qpos);
  for (int i = LANE; i < m.nq; i += DX_WAVE) qpos[i] = B.qpos[(size_t)env * m.nq + i];
  SYNC();
  kin_com(c);
  float* pt = c.f(K.pt);
  float* J = c.f(K.J);
  const ArgPoints pts{P};
  points_to_lds(c, pts, P.npoint, pt);
  if (P.mode == 1) {
    const size_t base = (size_t)env * n3 * nv;
    if (P.jacp) {
      point_jacobian(c, pts, P.npoint, pt, J, false);
      for (int k = LANE; k < n3 * nv; k += DX_WAVE) P.jacp[base + k] = J[k];
      SYNC();
    }
    if (P.jacr) {
      point_jacobian(c, pts, P.npoint, pt, J, true);
      for (int k = LANE; k < n3 * nv; k += DX_WAVE) P.jacr[base + k] = J[k];
    }
    return;
  }
  float* H = c.f(K.H);
  float* T = c.f(K.T);
  float* y = c.f(K.y);
  float* res = c.f(K.r);
  double* w = (double*)c.f(K.w);
  point_jacobian(c, pts, P.npoint, pt, J, false);
  const float v = LANE < n3 ? P.target[(size_t)env * n3 + LANE] : 0.f;
  if (LANE < n3) y[LANE] = v;
  const dx_f16v C = dls_gram32(J, n3, nv, P.reg);
  // the tile's lower triangle -> H (packed), and the largest diagonal entry
  const int j = LANE & 31, hi = LANE >> 5;
  float dmax = 0.f;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int i = 8 * (v >> 2) + 4 * hi + (v & 3);
    if (j <= i && i < n3) H[ti(i) + j] = C[v];
    if (i == j && i < n3) dmax = fmaxf(dmax, C[v]);
  }
  SYNC();
  dmax = wave_max_f(dmax);
  const float thr = 1.1920929e-07f * (float)max(n3, nv) * dmax;
  const bool ok = mfma_chol_pivots32(C, n3, thr);  // (wave-uniform)
  float qd = 0.f;
  if (ok) {
    mfma_chol_solve32(H, n3, 0.f, y, T);
    // lane d: dof d, (J^T y)_d in fp64.  A dof on no point's chain has a zero column: exactly 0
    double wd = 0.0;
    if (LANE < nv) {
      for (int r = 0; r < n3; r++) wd = fma((double)J[r * nv + LANE], (double)y[r], wd);
      w[LANE] = wd;
    }
    SYNC();
    // lane i: row i of the residual V - J (J^T y) - reg y
    if (LANE < n3) {
      double r = fma(-(double)P.reg, (double)y[LANE], (double)v);
      for (int d = 0; d < nv; d++) r = fma(-(double)J[LANE * nv + d], w[d], r);
      res[LANE] = (float)r;
    }
    SYNC();
    mfma_chol_solve32(H, n3, 0.f, res, T);
    if (LANE < nv) {
      for (int r = 0; r < n3; r++) wd = fma((double)J[r * nv + LANE], (double)res[r], wd);
      qd = (float)wd;
    }
  }
  if (LANE < nv) P.qvel[(size_t)env * nv + LANE] = qd;
  if (P.status && LANE == 0) P.status[env] = ok ? 0 : 1;
}

hipError_t dx_launch_dls(int nenv, size_t lds, hipStream_t stream, const DevModel* m, const DevBatch& B, const Lds& L,
                         const DlsDev& P) {
  hipLaunchKernelGGL(dx_dls_kernel, dim3(nenv), dim3(64), lds, stream, m, B, L, P);
  return hipGetLastError();
}
