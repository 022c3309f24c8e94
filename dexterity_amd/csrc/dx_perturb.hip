// dx_perturb.hip -- random pushes on the task's bodies (include/dx.h
// dx_env_set_perturbation) for CDNA4: one kernel ahead of every control step, beside the
// action filter, that writes the env's own xfrc_applied rows (DevBatch::xfrc in per-env
// mode).  The step kernels know nothing of it: they read the rows it left.
//
// Per env and control step, for each configured body in order, seven random_sample doubles
// of the env's own numpy-compatible RandomState -- u_gate, u_fmag, u_fz, u_fphi, u_tmag,
// u_tz, u_tphi -- are consumed whatever happens next (a numpy replay is then one
// random_sample(7 * nb) per step), and the first rule that matches applies:
//   the step re-initialises the env (it returns FIRST):  remain = 0, wrench = 0;
//   remain > 0:                                          remain -= 1, the wrench stays;
//   else: wrench = 0, and if u_gate < probability: remain = duration - 1 and
//     force  = (force_min + (force_max - force_min) u_fmag) * dir(u_fz, u_fphi),
//     torque likewise, dir(u_z, u_phi) = (s cos phi, s sin phi, z), z = 2 u_z - 1,
//     s = sqrt(1 - z z), phi = 2 pi u_phi: uniform on the sphere.  fp64, each component
//     magnitude * direction rounded to fp32 once.
// Then xfrc[env][body] = base[body] + wrench (one fp32 add per component; base is the
// batch's shared array, the gravity compensation) and DX_OUT_PERTURB holds the wrench.
//
// Layout: one wave per env, DX_PERT_WAVES per workgroup, every wave with LDS of its own
// for the MT19937 block (a wave barrier orders all it shares).  The wave tempers the 14 nb
// outputs in parallel (lane j: double j), lane k then owns body k: at most four lanes do
// the fp64 trigonometry, once per control step -- the stream's 2.5 KB block is the cost.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dx.h"
#include "dx_internal.h"

#define PERT_LAST 2  // dm_env StepType.LAST (dx_task.h TS_LAST)

// From here on no product contracts with a sum: the replay is numpy's fp64 arithmetic,
// which has no fma (dx_task.hip has the measured reason for the mtw_* helpers).
#pragma clang fp contract(off)
__device__ __forceinline__ double dx_dmul_exact(double a, double b) { return a * b; }
__device__ __forceinline__ double dx_dadd_exact(double a, double b) { return a + b; }
#define __dmul_rn dx_dmul_exact
#define __dadd_rn dx_dadd_exact
#define LANE ((int)(threadIdx.x & (DX_WAVE - 1)))
#define SYNC() __builtin_amdgcn_wave_barrier()
#include "dx_mtw.h"

// (magnitude in [lo, hi]) * (a direction uniform on the sphere), fp64 -> fp32
__device__ __forceinline__ void pert_vector(double lo, double hi, double u_mag, double u_z, double u_phi, float* out) {
  const double mag = lo + (hi - lo) * u_mag;
  const double z = 2.0 * u_z - 1.0;
  const double s = sqrt(1.0 - z * z);
  const double phi = 6.283185307179586 * u_phi;
  out[0] = (float)(mag * (s * cos(phi)));
  out[1] = (float)(mag * (s * sin(phi)));
  out[2] = (float)(mag * z);
}

extern "C" __global__ __launch_bounds__(DX_WAVE* DX_PERT_WAVES) void dx_perturb_kernel(Perturb P) {
  __shared__ uint32_t mt_sm[DX_PERT_WAVES][624];
  const int wave = (int)(threadIdx.x >> 6);
  const int env = blockIdx.x * DX_PERT_WAVES + wave;
  if (env >= P.nenv) return;  // (the whole wave)
  // task_pre's own test (dx_task.h), made a moment before it, as the action filter's
  const bool reinit = P.step_type[env] == PERT_LAST || P.episode[env] < 0;
  MtWave w = mtw_begin(P.mt + (size_t)env * DX_MTW_WORDS, mt_sm[wave]);
  const double u = mtw_uniform(w, 7 * P.nb, 0.0, 1.0);  // lane j: the step's j-th double
  double d[7];
#pragma unroll
  for (int i = 0; i < 7; i++) d[i] = __shfl(u, min(7 * LANE + i, DX_WAVE - 1), DX_WAVE);
  const int k = LANE;  // lane = configured body
  if (k >= P.nb) return;
  const size_t at = (size_t)env * P.nb + k;
  int remain = P.remain[at];
  float wr[6];
#pragma unroll
  for (int x = 0; x < 6; x++) wr[x] = P.wrench[6 * at + x];
  if (reinit) {
    remain = 0;
#pragma unroll
    for (int x = 0; x < 6; x++) wr[x] = 0.f;
  } else if (remain > 0) {
    remain -= 1;
  } else {
#pragma unroll
    for (int x = 0; x < 6; x++) wr[x] = 0.f;
    if (d[0] < P.prob) {
      remain = P.duration - 1;
      pert_vector(P.fmin, P.fmax, d[1], d[2], d[3], wr);
      pert_vector(P.tmin, P.tmax, d[4], d[5], d[6], wr + 3);
    }
  }
  P.remain[at] = remain;
  const int body = P.body[k];
  float* row = P.xfrc + ((size_t)env * P.nbody + body) * 6;
#pragma unroll
  for (int x = 0; x < 6; x++) {
    P.wrench[6 * at + x] = wr[x];
    row[x] = P.base[6 * body + x] + wr[x];
  }
}

// Test hook: the next n (<= 64) random_sample doubles of every env's stream (consumed).
extern "C" __global__ __launch_bounds__(DX_WAVE* DX_PERT_WAVES) void dx_perturb_draw_kernel(int nenv, int n, uint32_t* mt,
                                                                                          double* out) {
  __shared__ uint32_t mt_sm[DX_PERT_WAVES][624];
  const int wave = (int)(threadIdx.x >> 6);
  const int env = blockIdx.x * DX_PERT_WAVES + wave;
  if (env >= nenv) return;
  MtWave w = mtw_begin(mt + (size_t)env * DX_MTW_WORDS, mt_sm[wave]);
  const double u = mtw_uniform(w, n, 0.0, 1.0);
  if (LANE < n) out[(size_t)env * n + LANE] = u;
}
#undef LANE
#undef SYNC
#undef __dmul_rn
#undef __dadd_rn

hipError_t dx_launch_perturb(hipStream_t stream, const Perturb& P) {
  hipLaunchKernelGGL(dx_perturb_kernel, dim3((P.nenv + DX_PERT_WAVES - 1) / DX_PERT_WAVES), dim3(DX_WAVE * DX_PERT_WAVES),
                     0, stream, P);
  return hipGetLastError();
}

hipError_t dx_launch_perturb_draw(hipStream_t stream, int nenv, int n, uint32_t* mt, double* out) {
  hipLaunchKernelGGL(dx_perturb_draw_kernel, dim3((nenv + DX_PERT_WAVES - 1) / DX_PERT_WAVES),
                     dim3(DX_WAVE * DX_PERT_WAVES), 0, stream, nenv, n, mt, out);
  return hipGetLastError();
}
