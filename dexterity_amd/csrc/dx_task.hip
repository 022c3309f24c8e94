// dx_task.hip -- batched task logic on the device: the task kernels
// that bracket the step kernel when the task logic is not fused into it (reach, whose
// sampling pass runs between them; or DX_NO_FUSE=1), the MT19937 seeding kernels, the
// action pipeline ahead of the step (noise, previous action, EMA) and the bench / RL
// helpers.  The task logic itself is dx_task.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dx.h"
#include "dx_task.h"

__device__ __forceinline__ float urand(uint64_t seed, int env, int episode, int draw) {
  return dx_urand(seed, env, episode, draw);
}
// Seeds every env's two MT19937 streams with seed + env (numpy RandomState(seed + env)
// and np.random.seed(seed + env) of the env's process in the reference); the host passes
// seed + env0 for a shard whose env 0 is the job's env env0.
extern "C" __global__ void dx_mt_seed_kernel(int nenv, uint64_t seed, uint32_t* mt_env, uint32_t* mt_goal) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= nenv) return;
  const uint32_t s = (uint32_t)(seed + (uint64_t)env);
  dx_mt_seed(mt_env, nenv, env, s);
  dx_mt_seed(mt_goal, nenv, env, s);
}

// Reach: env e's RandomState(seed + e) as a contiguous block (state, pos = 624, no
// cached gaussian).
extern "C" __global__ void dx_mtw_seed_kernel(int nenv, uint64_t seed, uint32_t* mt) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= nenv) return;
  uint32_t* s = mt + (size_t)env * DX_MTW_WORDS;
  uint32_t v = (uint32_t)(seed + (uint64_t)env);
  for (int k = 0; k < 624; k++) {
    s[k] = v;
    v = 1812433253u * (v ^ (v >> 30)) + (uint32_t)(k + 1);
  }
  s[624] = 624;
  s[625] = 0;
  s[626] = 0;
  s[627] = 0;
}

extern "C" __global__ void dx_task_pre_kernel(TaskParams P, TaskState S, DevBatch B, const float* qpos0,
                                              const float* action) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= P.nenv) return;
  // action -> ctrl (effectors/mujoco_actuation.py:33; MuJoCo clamps internally)
  if (action)
    for (int i = 0; i < P.nu; i++) B.ctrl[(size_t)env * P.nu + i] = action[(size_t)env * P.nu + i];
  if (task_pre<false>(P, S, B, qpos0, env))
    for (int i = 0; i < P.nu; i++) B.ctrl[(size_t)env * P.nu + i] = 0;  // mj_resetData
}

// One 64-lane wave per env: lane 0 does the bookkeeping, all lanes write the
// observation (coalesced; a thread per env wrote 123 floats 492 B apart).
extern "C" __global__ void dx_task_post_kernel(TaskParams P, TaskState S, DevBatch B) {
  const int env = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (env >= P.nenv) return;
  const bool bad = B.bad && B.bad[env];
  task_post(P, S, B, env, lane, S.skip[env] != 0, bad, B.nstep[env]);
  if (lane == 0 && bad) B.bad[env] = 0;  // consumed (the env's episode ended with it)
}

// Uniform random actions within the actuator ctrlrange: the synthetic agent of
// manipulation_test.py:44-45 (random_state.uniform(spec.minimum, spec.maximum)).
// Keyed by the job-wide env index env0 + env, so a shard draws what the same envs of
// one unsharded batch draw.
extern "C" __global__ void dx_sample_actions_kernel(int nenv, int nu, const float* ctrlrange, uint64_t seed,
                                                    int step, int env0, float* out) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nenv * nu) return;
  int env = t / nu, i = t % nu;
  float u = urand(seed, env0 + env, step, 1000 + i);
  float lo = ctrlrange[2 * i], hi = ctrlrange[2 * i + 1];
  out[t] = lo + (hi - lo) * u;
}

extern "C" __global__ void dx_pack_outputs_kernel(int nenv, int obs_dim, const float* obs, const float* rew,
                                                  const float* disc, const int* st, float* dst) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  int w = obs_dim + 3;
  if (t >= nenv * w) return;
  int env = t / w, k = t % w;
  float v;
  if (k < obs_dim) v = obs[(size_t)env * obs_dim + k];
  else if (k == obs_dim) v = rew[env];
  else if (k == obs_dim + 1) v = disc[env];
  else v = (float)st[env];
  dst[t] = v;
}

// ------------------------------------------------------------------------ //
// the action pipeline ahead of the step (include/dx.h dx_env_set_action_filter)
// ------------------------------------------------------------------------ //
// One wave per env, DX_ACT_WAVES waves per workgroup: the mtw_* helpers index by the
// lane within the wave, and every wave has its own LDS (the MT19937 block and the
// accepted polar pairs), so a wave barrier orders all they share.
//
// From here to the end of this file no product contracts with a sum.  HIP's __dmul_rn /
// __dadd_rn are the plain operators, which the compiler's default (-ffp-contract=fast)
// fuses: with an fma in the polar method's x1 * x1 + x2 * x2 a gaussian with r2 close to 1
// came out up to 864 fp64 ulps from numpy's (log amplifies r2's last bit), and the moving
// average would not be numpy's either.  The pragma alone does not reach those two (their
// bodies are the HIP header's, parsed before it), so the mtw_* helpers get them as the
// two functions below, defined under it.  The step kernel's copy of the helpers
// (dx_step.hip, reach sampling) is compiled as before -- its draws agree with numpy after
// the cast to fp32, which is all it uses.
#pragma clang fp contract(off)
__device__ __forceinline__ double dx_dmul_exact(double a, double b) { return a * b; }
__device__ __forceinline__ double dx_dadd_exact(double a, double b) { return a + b; }
#define __dmul_rn dx_dmul_exact
#define __dadd_rn dx_dadd_exact
#define LANE ((int)(threadIdx.x & (DX_WAVE - 1)))
#define SYNC() __builtin_amdgcn_wave_barrier()
#include "dx_mtw.h"

// The reference's three action-side wrappers for env e's action row a[nu], in the order
// the reference nests them:
//   ActionNoise.step     (manipulation/wrappers/action_noise.py): x = clip(a + normal(scale =
//     scale * (max - min)), min, max) from the env's noise stream; drawn on every step,
//     also the one that turns out to reset the env (the wrapper draws before
//     environment.step knows).  The stddev is the reference's own value: numpy multiplies
//     the float32 bounds' difference by the scale in float32; the sum and the clip are
//     fp64, rounded to fp32 once.
//   PreviousAction       (effectors/wrappers/previous_action.py): the command set_control
//     received, zeros at initialize_episode.
//   SmoothAction         (effectors/wrappers/smooth_action.py): an exponential moving
//     average restarted at initialize_episode, alpha * held + (1 - alpha) * x in fp64.
// reinit is task_pre's own test (dx_task.h), made a moment before it: on such a step the
// env is re-initialised and the filtered action is ignored (ctrl = 0).  No product here
// may contract with a sum (numpy does not): the pragma above.
extern "C" __global__ __launch_bounds__(DX_WAVE* DX_ACT_WAVES) void dx_action_filter_kernel(ActFilter F,
                                                                                           const float* action) {
  __shared__ uint32_t mt_sm[DX_ACT_WAVES][624];
  __shared__ double pair_sm[DX_ACT_WAVES][DX_WAVE];
  const int wave = (int)(threadIdx.x >> 6);
  const int env = blockIdx.x * DX_ACT_WAVES + wave;
  if (env >= F.nenv) return;  // (the whole wave)
  const int i = LANE;
  const bool on = i < F.nu;
  const size_t at = (size_t)env * F.nu + (on ? i : 0);
  const bool reinit = F.step_type[env] == TS_LAST || F.episode[env] < 0;
  float x = on ? action[at] : 0.f;
  if (F.flags & DX_ACT_NOISE) {
    const float lo = on ? F.ctrlrange[2 * i] : 0.f, hi = on ? F.ctrlrange[2 * i + 1] : 0.f;
    const double sd = (double)(F.scale * (hi - lo));
    MtWave w = mtw_begin(F.mt + (size_t)env * DX_MTW_WORDS, mt_sm[wave]);
    const double noise = mtw_normal(w, F.nu, 0.0, sd, pair_sm[wave]);
    const double v = (double)x + noise;
    x = (float)fmin(fmax(v, (double)lo), (double)hi);  // np.clip
  }
  if (on) F.prev[at] = reinit ? 0.f : x;
  if (F.flags & DX_ACT_SMOOTH) {
    const int set = F.ema_set[env];
    if (reinit) {
      if (i == 0) F.ema_set[env] = 0;
    } else {
      if (set) x = (float)(F.alpha * (double)F.ema[at] + (1.0 - F.alpha) * (double)x);
      if (on) F.ema[at] = x;
      if (i == 0) F.ema_set[env] = 1;
    }
  }
  if (on) F.out[at] = x;
}

// Test hook: the next n standard normals of every env's noise stream (consumed).
extern "C" __global__ __launch_bounds__(DX_WAVE* DX_ACT_WAVES) void dx_action_noise_draw_kernel(int nenv, int n,
                                                                                               uint32_t* mt,
                                                                                               double* out) {
  __shared__ uint32_t mt_sm[DX_ACT_WAVES][624];
  __shared__ double pair_sm[DX_ACT_WAVES][DX_WAVE];
  const int wave = (int)(threadIdx.x >> 6);
  const int env = blockIdx.x * DX_ACT_WAVES + wave;
  if (env >= nenv) return;
  MtWave w = mtw_begin(mt + (size_t)env * DX_MTW_WORDS, mt_sm[wave]);
  const double g = mtw_normal(w, n, 0.0, 1.0, pair_sm[wave]);
  if (LANE < n) out[(size_t)env * n + LANE] = g;
}
#undef LANE
#undef SYNC
#undef __dmul_rn
#undef __dadd_rn
