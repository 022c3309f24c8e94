// dx_obspipe.hip -- the observation pipeline (include/dx.h dx_env_set_obs_pipeline) for
// CDNA4: composer's per-observable update_interval / buffer_size / delay / aggregator /
// corruptor ([3P] dm_control composer observation updater and buffer) over the row
// DX_OUT_OBS || DX_OUT_HAND_OBS, as one kernel behind the step and the hand observables'
// gather.  The step kernels know nothing of it and it never feeds back.
//
// Per env, with n = control steps since the episode's FIRST observation, m the interval,
// d the delay, K the buffer size (all in control steps):
//   sample s_j is taken when n == j m (s_0 is the FIRST observation), corrupted once, at
//   that moment, and arrives at j m + d;
//   the read at n delivers s_{J - (K-1-k)} in slot k (0 oldest), J = floor((n - d) / m) for
//   n >= d, else -1; a negative index is padding: zeros, or s_0 (DX_OBS_PAD_INITIAL).
// The ring keeps sample j in slot j % S, S = K + ceil(d / m).  The newest sample taken is
// j_new = floor(n / m) <= J + ceil(d / m), and the oldest one a read can name is J - (K-1),
// so every index a read names is within (j_new - S, j_new]: its slot still holds it.  s_0
// is overwritten by sample S, taken when J >= S - ceil(d / m) = K, and padding is read only
// while J < K - 1 -- s_0 is never overwritten while padding can still read it; before it
// arrives (n < d) j_new < ceil(d / m) < S as well.  So an episode start clears nothing: the
// index rule alone decides what is padding.
//
// Layout: one wave per env, DX_OBSP_WAVES per workgroup, every wave with LDS of its own (a
// wave barrier orders all it shares).  A ring row is Wp = W rounded up to 32 words, whole
// 128-B lines, written and read with 16-B accesses; the sample is assembled in LDS (scalar,
// coalesced loads of the two source rows) and a read that names the sample just taken gets
// it from there, so no wave reads back global memory it wrote in the same launch.  The
// delivered rows are W floats apart (W is odd for every shipped task), not 16-B aligned:
// they are stored as scalars.  An env moves its K delivered rows and at most one sample.
// With an aggregator a lane owns one element instead and sorts / sums its K values in
// registers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dx.h"
#include "dx_internal.h"

#define OBSP_FIRST 0          // dm_env StepType.FIRST (dx_task.h TS_FIRST)

// From here on no product contracts with a sum: the noise is numpy's
// v + normal(scale=sigma) in fp64 and the aggregates are numpy's fp64 sums, neither with an
// fma; the mtw_* helpers get __dmul_rn / __dadd_rn as functions defined under the pragma
// (dx_task.hip has the reason: an fma in the polar method moved gaussians by hundreds of ulps).
#pragma clang fp contract(off)
__device__ __forceinline__ double dx_dmul_exact(double a, double b) { return a * b; }
__device__ __forceinline__ double dx_dadd_exact(double a, double b) { return a + b; }
#define __dmul_rn dx_dmul_exact
#define __dadd_rn dx_dadd_exact
#define LANE ((int)(threadIdx.x & (DX_WAVE - 1)))
#define SYNC() __builtin_amdgcn_wave_barrier()
#include "dx_mtw.h"

// lane 0's stores of the cached gaussian (mtw_normal) ahead of the wave's next loads of it:
// one CU, one L1 -- only the order is needed
__device__ __forceinline__ void obsp_order_stores() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  SYNC();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One aggregate over a[0 .. K) (oldest first), in fp64 as numpy computes it over the
// reference's float64 rows, rounded to fp32 once.  a[] lives in registers: every index is
// a constant after unrolling.  min / max keep the later of two equal values (numpy's
// minimum / maximum loops); a NaN never reaches here (a diverged env is reset before it is
// observed).
__device__ __forceinline__ float obsp_aggregate(float (&a)[DX_OBSP_KMAX], int K, int agg) {
  if (agg == DX_OBS_AGG_MIN || agg == DX_OBS_AGG_MAX) {
    float acc = a[0];
#pragma unroll
    for (int k = 1; k < DX_OBSP_KMAX; k++)
      if (k < K) acc = agg == DX_OBS_AGG_MIN ? (acc < a[k] ? acc : a[k]) : (acc > a[k] ? acc : a[k]);
    return acc;
  }
  if (agg == DX_OBS_AGG_SUM || agg == DX_OBS_AGG_MEAN) {
    double s = (double)a[0];
#pragma unroll
    for (int k = 1; k < DX_OBSP_KMAX; k++)
      if (k < K) s = s + (double)a[k];
    return (float)(agg == DX_OBS_AGG_MEAN ? s / (double)K : s);
  }
  // median: the K values sorted in registers (odd-even transposition over all 16, the
  // unused tail +inf so it stays behind), then the middle one or (a + b) * 0.5
#pragma unroll
  for (int k = 0; k < DX_OBSP_KMAX; k++)
    if (k >= K) a[k] = __builtin_inff();
#pragma unroll
  for (int pass = 0; pass < DX_OBSP_KMAX; pass++) {
#pragma unroll
    for (int k = pass & 1; k + 1 < DX_OBSP_KMAX; k += 2) {
      const float lo = fminf(a[k], a[k + 1]), hi = fmaxf(a[k], a[k + 1]);
      a[k] = lo;
      a[k + 1] = hi;
    }
  }
  float lo = a[0], hi = a[0];
#pragma unroll
  for (int k = 0; k < DX_OBSP_KMAX; k++) {
    if (k == (K - 1) / 2) lo = a[k];
    if (k == K / 2) hi = a[k];
  }
  return (float)(((double)lo + (double)hi) * 0.5);
}

extern "C" __global__ __launch_bounds__(DX_WAVE* DX_OBSP_WAVES) void dx_obs_pipe_kernel(ObsPipe O, int restart) {
  __shared__ uint32_t mt_sm[DX_OBSP_WAVES][624];
  __shared__ double pair_sm[DX_OBSP_WAVES][DX_WAVE];
  __shared__ __attribute__((aligned(16))) float row_sm[DX_OBSP_WAVES][DX_OBSP_WMAX];
  const int wave = (int)(threadIdx.x >> 6);
  const int env = blockIdx.x * DX_OBSP_WAVES + wave;
  if (env >= O.nenv) return;  // (the whole wave)
  // 1. the env's clock: FIRST (dx_env_reset, or the step that re-initialised the env)
  // restarts it; a LAST observation is an ordinary step of its episode
  const int n = (restart || O.step_type[env] == OBSP_FIRST) ? 0 : O.count[env] + 1;
  if (LANE == 0) O.count[env] = n;
  const int nq4 = O.Wp >> 2;
  float* row = row_sm[wave];
  const float4* row4 = (const float4*)row;
  float4* ring4 = (float4*)(O.ring + (size_t)env * O.S * O.Wp);
  // 2. the sample, when one is due: the row (with the noise, drawn once per sample: the
  // ring stores the corrupted value) into LDS, then into its slot
  const bool sample = n % O.m == 0;
  const int jnew = sample ? n / O.m : -1;
  if (sample) {
    MtWave w{};
    if (O.noise) w = mtw_begin(O.mt + (size_t)env * DX_MTW_WORDS, mt_sm[wave]);
    for (int base = 0; base < O.Wp; base += DX_WAVE) {
      const int i = base + LANE;
      float v = 0.f;
      if (i < O.obs_dim) v = O.obs[(size_t)env * O.obs_dim + i];
      else if (i < O.W) v = O.hand[(size_t)env * O.hand_dim + (i - O.obs_dim)];
      if (O.noise && base < O.W) {
        // the row's W legacy gaussians in element order, 64 at a time: numpy's cached
        // second value carries from chunk to chunk and from sample to sample; a zero sigma
        // still consumes its draw
        const double g = mtw_normal(w, min(DX_WAVE, O.W - base), 0.0, 1.0, pair_sm[wave]);
        if (i < O.W) v = (float)((double)v + O.sigma[i] * g);
        obsp_order_stores();
      }
      row[i] = v;  // i < Wp <= DX_OBSP_WMAX
    }
    SYNC();
    float4* dst = ring4 + (size_t)(jnew % O.S) * nq4;
    for (int q = LANE; q < nq4; q += DX_WAVE) dst[q] = row4[q];
  }
  // 3. the read: K delivered rows, or their aggregate
  const int J = n >= O.d ? (n - O.d) / O.m : -1;
  const int K = O.K, W = O.W;
  const bool pad0 = O.pad == DX_OBS_PAD_ZERO;
  auto load = [&](int idx, int q) -> float4 {
    if (idx < 0) {
      if (pad0) return make_float4(0.f, 0.f, 0.f, 0.f);
      idx = 0;
    }
    if (idx == jnew) return row4[q];  // the sample just taken
    return ring4[(size_t)(idx % O.S) * nq4 + q];
  };
  if (O.agg == DX_OBS_AGG_NONE) {
    float* out = O.out + (size_t)env * K * W;
    for (int q = LANE; q < nq4; q += DX_WAVE)
      for (int k = 0; k < K; k++) {
        const float4 v = load(J - (K - 1 - k), q);
        float* o = out + (size_t)k * W + 4 * q;
        if (4 * q + 0 < W) o[0] = v.x;
        if (4 * q + 1 < W) o[1] = v.y;
        if (4 * q + 2 < W) o[2] = v.z;
        if (4 * q + 3 < W) o[3] = v.w;
      }
  } else {
    // one lane per element: its K values in registers (4-B accesses here, a wave's still
    // 256 contiguous bytes of a row), one coalesced store of the result
    float* out = O.out + (size_t)env * W;
    const float* ring = (const float*)ring4;
    for (int i = LANE; i < W; i += DX_WAVE) {
      float a[DX_OBSP_KMAX];
#pragma unroll
      for (int k = 0; k < DX_OBSP_KMAX; k++) {
        int idx = J - (K - 1 - k);
        float v = 0.f;
        if (k < K && (idx >= 0 || !pad0)) {
          idx = max(idx, 0);
          v = idx == jnew ? row[i] : ring[(size_t)(idx % O.S) * O.Wp + i];
        }
        a[k] = v;
      }
      out[i] = obsp_aggregate(a, K, O.agg);
    }
  }
}

// Test hook: the next n standard normals of every env's noise stream (consumed).
extern "C" __global__ __launch_bounds__(DX_WAVE* DX_OBSP_WAVES) void dx_obs_noise_draw_kernel(int nenv, int n,
                                                                                             uint32_t* mt,
                                                                                             double* out) {
  __shared__ uint32_t mt_sm[DX_OBSP_WAVES][624];
  __shared__ double pair_sm[DX_OBSP_WAVES][DX_WAVE];
  const int wave = (int)(threadIdx.x >> 6);
  const int env = blockIdx.x * DX_OBSP_WAVES + wave;
  if (env >= nenv) return;
  MtWave w = mtw_begin(mt + (size_t)env * DX_MTW_WORDS, mt_sm[wave]);
  const double g = mtw_normal(w, n, 0.0, 1.0, pair_sm[wave]);
  if (LANE < n) out[(size_t)env * n + LANE] = g;
}
#undef LANE
#undef SYNC
#undef __dmul_rn
#undef __dadd_rn

hipError_t dx_launch_obs_pipe(hipStream_t stream, const ObsPipe& O, int restart) {
  hipLaunchKernelGGL(dx_obs_pipe_kernel, dim3((O.nenv + DX_OBSP_WAVES - 1) / DX_OBSP_WAVES),
                     dim3(DX_WAVE * DX_OBSP_WAVES), 0, stream, O, restart);
  return hipGetLastError();
}

hipError_t dx_launch_obs_noise_draw(hipStream_t stream, int nenv, int n, uint32_t* mt, double* out) {
  hipLaunchKernelGGL(dx_obs_noise_draw_kernel, dim3((nenv + DX_OBSP_WAVES - 1) / DX_OBSP_WAVES),
                     dim3(DX_WAVE * DX_OBSP_WAVES), 0, stream, nenv, n, mt, out);
  return hipGetLastError();
}
