// dx_api.hip -- the env unit: physics batch + on-device task logic, and the optional
// pipelines around a control step.
#include "dx_host.h"

extern "C" __global__ void dx_task_pre_kernel(TaskParams P, TaskState S, DevBatch B, const float* qpos0,
                                              const float* action);
extern "C" __global__ void dx_task_post_kernel(TaskParams P, TaskState S, DevBatch B);
extern "C" __global__ void dx_mt_seed_kernel(int nenv, uint64_t seed, uint32_t* mt_env, uint32_t* mt_goal);
extern "C" __global__ void dx_mtw_seed_kernel(int nenv, uint64_t seed, uint32_t* mt);
extern "C" __global__ void dx_action_filter_kernel(ActFilter F, const float* action);
extern "C" __global__ void dx_action_noise_draw_kernel(int nenv, int n, uint32_t* mt, double* out);

// The env's numpy-compatible streams: mt[k] seeded as RandomState(seed + env0 + k).
static hipError_t seed_streams(dx_env* e, uint64_t seed, uint32_t* mt) {
  hipLaunchKernelGGL(dx_mtw_seed_kernel, dim3((e->P.nenv + 63) / 64), dim3(64), 0, e->batch->stream, e->P.nenv,
                     seed + (uint64_t)e->P.env0, mt);
  return hipGetLastError();
}

static void obs_pipe_free(ObsPipe& O) {
  (void)hipFree(O.ring);
  (void)hipFree(O.count);
  (void)hipFree(O.mt);
  (void)hipFree((void*)O.sigma);
  (void)hipFree(O.out);
  O = ObsPipe{};
}

// The draws of the test hooks dx_env_*_draw: `launch` fills nenv * n doubles on the device,
// which come back to out_host; `what` starts the text of a HIP error.
template <class Launch>
static int env_draw(dx_env* e, int n, double* out_host, const char* what, Launch launch) {
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  double* dev = nullptr;
  const size_t bytes = (size_t)e->P.nenv * n * 8;
  HIPCHK(hipMalloc((void**)&dev, bytes));
  hipError_t err = launch(dev);
  if (err == hipSuccess) err = hipMemcpyAsync(out_host, dev, bytes, hipMemcpyDeviceToHost, b->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(b->stream);
  (void)hipFree(dev);
  if (err != hipSuccess) return dx_fail(DX_EHIP, what + std::string(hipGetErrorString(err)));
  return 0;
}

extern "C" dx_env* dx_env_create(const dx_model* m, int32_t nenv, int32_t device, int32_t task,
                                 uint64_t seed, const float* params, int32_t nparams) {
  return dx_env_create_shard(m, nenv, device, task, seed, 0, params, nparams);
}

extern "C" dx_env* dx_env_create_shard(const dx_model* m, int32_t nenv, int32_t device, int32_t task,
                                       uint64_t seed, int64_t env0, const float* params, int32_t nparams) {
  if (env0 < 0 || env0 + (int64_t)nenv > 0x7fffffffll) { dx_fail(DX_EINVAL, "env0 out of range"); return nullptr; }
  if (task != DX_TASK_REORIENT && task != DX_TASK_REACH && task != DX_TASK_HANDOVER) {
    dx_fail(DX_EINVAL, "unknown task kind");
    return nullptr;
  }
  if (!m) { dx_fail(DX_EINVAL, "null model"); return nullptr; }
  const int nq = m->dm.nq, nu = m->dm.nu;
  if (!params || (task == DX_TASK_REORIENT && nparams < DX_REORIENT_NPARAMS) ||
      (task == DX_TASK_HANDOVER && nparams < DX_HANDOVER_NPARAMS) ||
      (task == DX_TASK_REACH && nparams < DX_REACH_NPARAMS_HEAD + 3 * nq + nu * nq)) {
    dx_fail(DX_EINVAL, "too few task params");
    return nullptr;
  }
  dx_batch* b = dx_batch_create(m, nenv, device);
  if (!b) return nullptr;
  dx_env* e = new dx_env();
  e->batch = b;
  const DevModel& d = b->dm;
  TaskParams& P = e->P;
  memset(&P, 0, sizeof(P));
  P.kind = task == DX_TASK_REACH ? DX_KIND_REACH : task == DX_TASK_HANDOVER ? DX_KIND_HANDOVER : DX_KIND_REORIENT;
  P.nenv = nenv; P.nq = d.nq; P.nv = d.nv; P.nu = d.nu; P.nsite = d.nsite;
  P.seed = seed;
  P.env0 = (int)env0;
  e->nsub = (int)params[0];
  P.hand_nq = (int)params[1]; P.hand_nv = (int)params[2];
  int watch_geom = -1, watch_body = -1;
  bool bad = false;
  if (task != DX_TASK_REACH) {  // reorient, and the handover on the same params
    P.prop_qadr = (int)params[3]; P.prop_dadr = (int)params[4];
    int tip0 = (int)params[5];
    P.ntips = (int)params[6];
    for (int t = 0; t < P.ntips && t < DX_MAX_TIPS; t++) P.tip_sites[t] = tip0 + t;
    P.successes_needed = (int)params[7]; P.steps_before_change = (int)params[8];
    P.fall_termination = (int)params[9];
    P.threshold = params[10]; P.eps = params[11]; P.w_orient = params[12]; P.w_success = params[13];
    P.w_action = params[14]; P.max_time = params[15];
    for (int k = 0; k < 3; k++) {
      P.bbox_lo[k] = params[16 + k]; P.bbox_hi[k] = params[19 + k];
      // fp64 box: the raw bits of six doubles in params 26-37, when given
      P.bbox_lo_d[k] = params[16 + k];
      P.bbox_hi_d[k] = params[19 + k];
      if (nparams >= 38) {
        memcpy(&P.bbox_lo_d[k], params + 26 + 2 * k, 8);
        memcpy(&P.bbox_hi_d[k], params + 32 + 2 * k, 8);
      }
    }
    watch_geom = (int)params[22]; watch_body = (int)params[23];
    P.goal_dim = 4;  // the target quaternion, or (handover) the target point and receiving hand
    // (the handover has no hint prop: no target_prop/orientation block)
    const int prop_obs = P.prop_qadr < 0 ? 0 : task == DX_TASK_HANDOVER ? 13 : 17;
    P.obs_dim = 2 * P.hand_nq + P.hand_nv + 6 * P.ntips + prop_obs + 4;
    bad = P.prop_qadr >= 0 && (P.prop_qadr + 7 > d.nq || P.prop_dadr + 6 > d.nv);
    if (task == DX_TASK_HANDOVER) {
      for (int h = 0; h < 2; h++)
        for (int k = 0; k < 3; k++) P.hand_target[h][k] = params[38 + 3 * h + k];
      bad = bad || P.prop_qadr < 0;
    }
  } else {
    P.prop_qadr = -1; P.prop_dadr = -1;
    P.ntips = (int)params[3];
    for (int t = 0; t < P.ntips && t < DX_MAX_TIPS; t++) P.tip_sites[t] = (int)params[4 + t];
    P.successes_needed = (int)params[9]; P.steps_before_change = (int)params[10];
    P.threshold = params[11]; P.max_time = params[12]; P.dense = (int)params[13];
    P.range_frac = params[14]; P.goal_scale = params[15]; P.max_reject = (int)params[16];
    P.ncoupled = (int)params[17];
    for (int k = 0; k < P.ncoupled && k < 4; k++) {
      P.coupled[k][0] = (int)params[18 + 2 * k];
      P.coupled[k][1] = (int)params[19 + 2 * k];
      bad = bad || P.coupled[k][0] < 0 || P.coupled[k][0] >= nq || P.coupled[k][1] < 0 || P.coupled[k][1] >= nq;
    }
    P.goal_dim = 3 * P.ntips;
    P.obs_dim = 2 * P.hand_nq + P.hand_nv + 6 * P.ntips + P.goal_dim;
    bad = bad || P.hand_nq != d.nq || P.ncoupled > 4 || P.max_reject < 1;
  }
  for (int t = 0; t < P.ntips && t < DX_MAX_TIPS; t++) bad = bad || P.tip_sites[t] < 0 || P.tip_sites[t] >= d.nsite;
  if (bad || P.ntips > DX_MAX_TIPS || P.hand_nq > d.nq || P.hand_nv > d.nv || e->nsub < 1) {
    dx_fail(DX_EINVAL, "task parameters inconsistent with the model");
    dx_batch_destroy(b);
    delete e;
    return nullptr;
  }
  if (watch_geom >= 0 && dx_set_watch(b, watch_geom, watch_body) != 0) { dx_batch_destroy(b); delete e; return nullptr; }
  // the contact pads: bodies (other than the world's and the prop's) with a geom pair
  // against a geom of the prop body, in body order -- the hands' bodies, hand after hand
  if (task != DX_TASK_REACH && watch_body >= 1 && watch_body < d.nbody) {
    const auto& gg = m->hi.at("gpair_geom");
    const auto& gb = m->hi.at("geom_bodyid");
    std::vector<char> hit(d.nbody, 0);
    for (int k = 0; k < d.ngpair; k++) {
      const int b1 = gb[gg[2 * k]], b2 = gb[gg[2 * k + 1]];
      if (b1 == watch_body && b2 != watch_body) hit[b2] = 1;
      if (b2 == watch_body && b1 != watch_body) hit[b1] = 1;
    }
    for (int k = 1; k < d.nbody; k++)
      if (hit[k]) e->cf_pads.push_back({k, watch_body});
  }
  TaskState& S = e->S;
  size_t E = nenv;
  auto al = [&](void** p, size_t bytes) { return balloc(b, p, bytes); };
  int rc = 0;
  rc |= al((void**)&S.goal, E * P.goal_dim * 4); rc |= al((void**)&S.solve_start, E * 4);
  rc |= al((void**)&S.reward, E * 4); rc |= al((void**)&S.discount, E * 4);
  rc |= al((void**)&S.obs, E * P.obs_dim * 4);
  rc |= al((void**)&S.successes, E * 4); rc |= al((void**)&S.counter, E * 4);
  rc |= al((void**)&S.registered, E * 4); rc |= al((void**)&S.exceeded, E * 4);
  rc |= al((void**)&S.step_type, E * 4); rc |= al((void**)&S.episode, E * 4);
  rc |= al((void**)&S.skip, E * 4); rc |= al((void**)&S.failure, E * 4);
  rc |= al((void**)&S.need, E * 4); rc |= al((void**)&S.goalnum, E * 4); rc |= al((void**)&S.goalfail, E * 4);
  rc |= al((void**)&S.time_d, E * 8); rc |= al((void**)&S.solve_start_d, E * 8);
  rc |= al((void**)&S.nsub_d, E * 4); rc |= al((void**)&S.solve_n, E * 4);
  if (task == DX_TASK_REACH) rc |= al((void**)&S.goal_qpos, E * nq * 4);
  if (task != DX_TASK_REACH) {
    rc |= al((void**)&S.mt_env, E * DX_MT_WORDS * 4);
    rc |= al((void**)&S.mt_goal, E * DX_MT_WORDS * 4);
    if (!rc) {
      hipLaunchKernelGGL(dx_mt_seed_kernel, dim3((nenv + 63) / 64), dim3(64), 0, b->stream, nenv, seed + (uint64_t)env0, S.mt_env,
                         S.mt_goal);
      if (hipGetLastError() != hipSuccess) rc = dx_fail(DX_EHIP, "MT19937 seeding kernel launch failed");
    }
  }
  P.time_limit = INFINITY;
  P.time_limit_d = INFINITY;
  P.h_d = dx_getd(m, "timestep");
  P.max_time_d = P.max_time;  // dx_env_set_goal_time_limit gives the fp64 value
  float* tdata = nullptr;
  TaskParams* dP = nullptr;
  TaskState* dS = nullptr;
  if (!rc && task == DX_TASK_REACH) {
    size_t nt = 3 * (size_t)nq + (size_t)nu * nq;
    // optional fp64 block (raw bits of 6 x nq doubles) for numpy-compatible draws
    if (nparams >= DX_REACH_NPARAMS_HEAD + (int)nt + 12 * nq) {
      nt += 12 * (size_t)nq;
      P.tdata_f64 = 1;
      rc |= al((void**)&S.mt_reach, E * DX_MTW_WORDS * 4);
      if (!rc && seed_streams(e, seed, S.mt_reach) != hipSuccess) rc = dx_fail(DX_EHIP, "MT19937 seeding kernel launch failed");
    }
    rc |= al((void**)&tdata, nt * 4);
    // balloc zeroes on the batch's (non-blocking) stream: drain it before the
    // synchronous copies below, or a late memset can wipe what they wrote
    if (!rc && hipStreamSynchronize(b->stream) != hipSuccess) rc = dx_fail(DX_EHIP, "stream sync failed");
    if (!rc && hipMemcpy(tdata, params + DX_REACH_NPARAMS_HEAD, nt * 4, hipMemcpyHostToDevice) != hipSuccess)
      rc = dx_fail(DX_EHIP, "hipMemcpy failed");
    P.tdata = tdata;
  }
  if (!rc) rc |= al((void**)&dP, sizeof(TaskParams));
  if (!rc) rc |= al((void**)&dS, sizeof(TaskState));
  std::vector<int> neg(E, -1);
  if (!rc && hipStreamSynchronize(b->stream) != hipSuccess) rc = dx_fail(DX_EHIP, "stream sync failed");
  if (!rc && (hipMemcpy(S.episode, neg.data(), E * 4, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(dP, &P, sizeof(P), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(dS, &S, sizeof(S), hipMemcpyHostToDevice) != hipSuccess))
    rc = dx_fail(DX_EHIP, "hipMemcpy failed");
  if (rc) { dx_batch_destroy(b); delete e; return nullptr; }
  b->db.skip = S.skip;
  b->db.out_bodies = 0;  // the tasks read sites and qpos only (dx_set_outputs turns body poses back on)
  b->db.tp = dP;
  b->db.ts = dS;
  return e;
}

extern "C" int dx_env_goal_dim(const dx_env* e) { return e ? e->P.goal_dim : dx_fail(DX_EINVAL, "null env"); }

extern "C" void dx_env_destroy(dx_env* e) {
  if (!e) return;
  obs_pipe_free(e->O);
  dx_batch_destroy(e->batch);
  delete e;
}

extern "C" dx_batch* dx_env_batch(dx_env* e) { return e ? e->batch : nullptr; }
extern "C" int dx_env_obs_dim(const dx_env* e) { return e ? e->P.obs_dim : dx_fail(DX_EINVAL, "null env"); }

extern "C" __global__ void dx_sample_actions_kernel(int nenv, int nu, const float* ctrlrange, uint64_t seed,
                                                    int step, int env0, float* out);

// The optional hand observables' gather (dx_observe.hip), queued on the batch stream behind
// a control step's last launch: launch_step has returned, so the overflow tier's launch --
// where the mid tier's side stream is joined on the device -- or the order kernel of a
// contact-free scene is ahead of it, and every tier's observation pass has written the
// batch arrays it reads.  No stream event; nothing is launched while the feature is off.
enum { HOBS_NEEDS_BODIES = DX_HOBS_TIP_ORIENTATIONS | DX_HOBS_TIP_POSITIONS_EGO };
static int env_hand_obs(dx_env* e) {
  if (!e->H.mask) return 0;
  HIPCHK(dx_launch_hand_obs(e->batch->stream, e->H));
  return 0;
}
// What follows a control step's last launch: the hand observables' gather, then the
// observation pipeline (dx_obspipe.hip), which reads DX_OUT_OBS, the step type and that
// gather's rows -- all on the batch stream, so the launch point above orders it too.
// Nothing is launched while the pipeline is off.
static int env_observe(dx_env* e) {
  // the contact forces (dx_sensor.hip) of the step's last physics step, zero for the envs
  // that returned FIRST: at the same launch point, where every tier has written its stash
  // and the step types
  if (e->cf_on)
    if (int rc = launch_sensor(e->batch, &e->CF, e->cf_out)) return rc;
  if (int rc = env_hand_obs(e)) return rc;
  // the cameras (dx_render.hip) over the body poses the same observation pass wrote: an env
  // that returned FIRST shows its reset state
  if (e->batch->RA.ncam)
    if (int rc = dx_render(e->batch)) return rc;
  if (!e->O.on) return 0;
  HIPCHK(dx_launch_obs_pipe(e->batch->stream, e->O, 0));
  return 0;
}

// One control step.  The task logic runs fused into the step kernel (task_pre in each
// env's first physics-step task, task_post in its last; dx_task.h): a reorient control step
// is the step kernel plus the overflow tier's launch.  Reach (a reach scene's
// specialization) also runs its sampling pass -- goal rollouts, joint sampling -- in the
// env's first task (dx_step.hip fused_reach_prep): the step kernel plus the order kernel
// (contact-free Shadow reach) or the overflow tier (Adroit).  DX_NO_FUSE=1 selects the
// task kernels and the separate sampling launch instead.
// random: actions drawn in the kernel by the random agent (seed, step) instead of read.
static int env_run(dx_env* e, const float* action, bool random = false, uint64_t seed = 0, int step = 0) {
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  if ((e->H.mask & HOBS_NEEDS_BODIES) || b->RA.ncam) b->db.out_bodies = 1;  // (whatever dx_set_outputs was told since)
  if (e->PT.nb && (action || random)) {
    // the random pushes: one launch ahead of the step's, which then read the env's own xfrc
    // rows (per-env mode again, from the current shared array, had dx_set_xfrc left it)
    if (int rc = xfrc_env_mode(b)) return rc;
    e->PT.xfrc = b->xfrc_env;
    HIPCHK(dx_launch_perturb(b->stream, e->PT));
  }
  if (e->F.flags && (action || random)) {
    // the action pipeline: one launch ahead of the step's, which then read the filtered
    // buffer (never the caller's); the random agent draws into the action buffer first --
    // the same function of (seed, env, step) as the step kernel's own draw
    if (random) {
      if (int rc = dx_env_sample_actions(e, seed, step)) return rc;
      action = (const float*)e->allocs[0];
      random = false;
    }
    hipLaunchKernelGGL(dx_action_filter_kernel, dim3((e->P.nenv + DX_ACT_WAVES - 1) / DX_ACT_WAVES),
                       dim3(DX_WAVE * DX_ACT_WAVES), 0, b->stream, e->F, action);
    HIPCHK(hipGetLastError());
    action = e->F.out;
  }
  const bool fuse = !getenv("DX_NO_FUSE") && ((e->P.kind != DX_KIND_REACH && b->db.defer) ||
                                              (e->P.kind == DX_KIND_REACH && b->spec >= 0 && dx_spec_reach(b->spec)));
  if (fuse) {
    DevBatch& B = b->db;
    const int* skip = B.skip;
    B.fuse = 1;
    B.skip = nullptr;
    B.action = action;
    B.act_random = random ? 1 : 0;
    B.act_seed = seed;
    B.act_step = step;
    const int rc = launch_step(b, e->nsub, 0);
    B.fuse = 0;
    B.skip = skip;
    B.action = nullptr;
    B.act_random = 0;
    if (rc) return rc;
    return env_observe(e);
  }
  if (random) {  // the random agent into the action buffer, then the step
    if (int rc = dx_env_sample_actions(e, seed, step)) return rc;
    action = (const float*)e->allocs[0];
  }
  int nb = (e->P.nenv + 63) / 64;
  hipLaunchKernelGGL(dx_task_pre_kernel, dim3(nb), dim3(64), 0, b->stream, e->P, e->S, b->db,
                     b->dm.qpos0, action);
  HIPCHK(hipGetLastError());
  // reach: goal rollouts / joint sampling for the envs that need them (the rest of
  // the grid exits at once)
  if (e->P.kind == DX_KIND_REACH)
    if (int rc = launch_step(b, 1, 2)) return rc;
  if (int rc = launch_step(b, e->nsub, 0)) return rc;
  hipLaunchKernelGGL(dx_task_post_kernel, dim3((e->P.nenv + 3) / 4), dim3(256), 0, b->stream, e->P, e->S, b->db);  // a wave per env
  HIPCHK(hipGetLastError());
  return env_observe(e);
}

// The pushes' initialize_episode for every env: no wrench held, every row the base again
// (the per-env rows refilled from the shared array), nothing drawn.
static int perturb_clear(dx_env* e) {
  dx_batch* b = e->batch;
  const size_t E = e->P.nenv;
  HIPCHK(hipMemsetAsync(e->PT.remain, 0, E * DX_PERT_MAXB * 4, b->stream));
  HIPCHK(hipMemsetAsync(e->PT.wrench, 0, E * DX_PERT_MAXB * 6 * 4, b->stream));
  b->db.xfrc = e->pt_shared ? b->xfrc : nullptr;
  b->db.xfrc_stride = 0;
  return xfrc_env_mode(b);
}

extern "C" int dx_env_reset(dx_env* e) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  if (e->PT.nb) {
    // (dx_set_xfrc on the env's batch since: that array is the base now)
    if (!e->batch->db.xfrc_stride) e->pt_shared = e->batch->db.xfrc != nullptr;
    if (int rc = perturb_clear(e)) return rc;
  }
  // step_type LAST makes the pre-kernel run initialize_episode for every env
  std::vector<int> last(e->P.nenv, 2);
  HIPCHK(hipMemcpyAsync(e->S.step_type, last.data(), last.size() * 4, hipMemcpyHostToDevice, e->batch->stream));
  if (e->F.flags) {  // the action pipeline's initialize_episode: no draw, no EMA value, zero previous action
    const size_t E = e->P.nenv;
    HIPCHK(hipMemsetAsync(e->F.ema_set, 0, E * 4, e->batch->stream));
    HIPCHK(hipMemsetAsync(e->F.prev, 0, E * e->P.nu * 4, e->batch->stream));
  }
  HIPCHK(hipStreamSynchronize(e->batch->stream));
  return env_run(e, nullptr);
}

// ---- the action pipeline (dx_task.hip dx_action_filter_kernel) ----
extern "C" int dx_env_set_action_filter(dx_env* e, const dx_action_filter* f) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));  // may be called between steps
  const int flags = f ? f->flags : 0;
  if (flags & ~(DX_ACT_NOISE | DX_ACT_SMOOTH | DX_ACT_PREVIOUS)) return dx_fail(DX_EINVAL, "unknown action filter flags");
  ActFilter& F = e->F;
  if (!flags) {  // off: the step's launches, outputs and checkpoint are those of an env never configured
    F.flags = 0;
    return 0;
  }
  const int nu = e->P.nu;
  const size_t E = e->P.nenv;
  if (nu > DX_ACT_NU_MAX) return dx_fail(DX_ELIMIT, "action filter: more than 64 actuators");
  if (nu < 1) return dx_fail(DX_EINVAL, "action filter: the model has no actuators");
  if ((flags & DX_ACT_SMOOTH) && !(f->smooth_alpha >= 0.0 && f->smooth_alpha <= 1.0))
    return dx_fail(DX_EINVAL, "action filter: smooth_alpha must be within [0, 1]");
  if (flags & DX_ACT_NOISE) {
    if (!std::isfinite(f->noise_scale) || f->noise_scale < 0.f)
      return dx_fail(DX_EINVAL, "action filter: noise_scale must be finite and non-negative");
    // the reference's stddev, scale * (maximum - minimum), is infinite for an unbounded actuator
    const auto& lim = b->model->hi.at("actuator_ctrllimited");
    for (int i = 0; i < nu; i++)
      if (i >= (int)lim.size() || !lim[i]) return dx_fail(DX_EINVAL, "action filter: noise needs every actuator ctrllimited");
  }
  if (!F.mt) {  // first use (balloc zeroes: no EMA value, zero previous action)
    ActFilter A{};
    int rc = balloc(b, (void**)&A.out, E * nu * 4);
    if (!rc) rc = balloc(b, (void**)&A.ema, E * nu * 4);
    if (!rc) rc = balloc(b, (void**)&A.prev, E * nu * 4);
    if (!rc) rc = balloc(b, (void**)&A.ema_set, E * 4);
    if (!rc) rc = balloc(b, (void**)&A.mt, E * DX_MTW_WORDS * 4);
    if (rc) return rc;
    A.nenv = e->P.nenv;
    A.nu = nu;
    A.ctrlrange = (const float*)b->dm.actuator_ctrlrange;
    A.step_type = e->S.step_type;
    A.episode = e->S.episode;
    F = A;
  } else {
    // a stage switched on again starts as at initialize_episode
    if (!F.flags) HIPCHK(hipMemsetAsync(F.prev, 0, E * nu * 4, b->stream));
    if (!(F.flags & DX_ACT_SMOOTH)) HIPCHK(hipMemsetAsync(F.ema_set, 0, E * 4, b->stream));
  }
  if (flags & DX_ACT_NOISE) {  // env e draws from RandomState(noise_seed + env0 + e)
    HIPCHK(seed_streams(e, f->noise_seed, F.mt));
    F.scale = f->noise_scale;
  }
  if (flags & DX_ACT_SMOOTH) F.alpha = f->smooth_alpha;
  HIPCHK(hipStreamSynchronize(b->stream));
  F.flags = flags;
  return 0;
}

extern "C" int dx_env_action_noise_draw(dx_env* e, int32_t n, double* out_host) {
  if (!e || !out_host) return dx_fail(DX_EINVAL, "null argument");
  if (!(e->F.flags & DX_ACT_NOISE)) return dx_fail(DX_EINVAL, "action noise is not enabled");
  if (n < 1 || n > DX_WAVE) return dx_fail(DX_EINVAL, "between 1 and 64 normals per call");
  return env_draw(e, n, out_host, "action noise draw: ", [&](double* dev) {
    hipLaunchKernelGGL(dx_action_noise_draw_kernel, dim3((e->P.nenv + DX_ACT_WAVES - 1) / DX_ACT_WAVES),
                       dim3(DX_WAVE * DX_ACT_WAVES), 0, e->batch->stream, e->P.nenv, (int)n, e->F.mt, dev);
    return hipGetLastError();
  });
}

// ---- the random pushes (dx_perturb.hip dx_perturb_kernel) ----
extern "C" int dx_env_set_perturbation(dx_env* e, const dx_perturbation* p) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));  // may be called between steps
  Perturb& T = e->PT;
  if (!p || p->nbody == 0) {  // off: shared mode, the launches, outputs and checkpoint of an env never configured
    if (T.nb) {
      if (b->db.xfrc_stride) {  // (else dx_set_xfrc has already left per-env mode)
        b->db.xfrc = e->pt_shared ? b->xfrc : nullptr;
        b->db.xfrc_stride = 0;
      }
      T.nb = 0;
    }
    return 0;
  }
  // every check ahead of every change: a rejected call leaves everything as it was
  if (e->P.kind == DX_KIND_REACH)
    return dx_fail(DX_EINVAL, "perturbation: not for the reach tasks (their goal rollouts step the physics inside the reset)");
  if (p->nbody < 0) return dx_fail(DX_EINVAL, "perturbation: negative body count");
  if (p->nbody > DX_PERT_MAXB) return dx_fail(DX_ELIMIT, "perturbation: more than 4 bodies");
  for (int k = 0; k < p->nbody; k++) {
    if (p->bodies[k] < 1 || p->bodies[k] >= b->dm.nbody)
      return dx_fail(DX_EINVAL, "perturbation: a body id outside [1, nbody) (the world body cannot be pushed)");
    for (int j = 0; j < k; j++)
      if (p->bodies[j] == p->bodies[k]) return dx_fail(DX_EINVAL, "perturbation: a repeated body id");
  }
  if (!(p->probability >= 0.0 && p->probability <= 1.0)) return dx_fail(DX_EINVAL, "perturbation: probability outside [0, 1]");
  auto range_ok = [](double lo, double hi) { return std::isfinite(lo) && std::isfinite(hi) && lo >= 0.0 && lo <= hi; };
  if (!range_ok(p->force_min, p->force_max)) return dx_fail(DX_EINVAL, "perturbation: force range must be finite, non-negative, min <= max");
  if (!range_ok(p->torque_min, p->torque_max)) return dx_fail(DX_EINVAL, "perturbation: torque range must be finite, non-negative, min <= max");
  if (p->duration < 1) return dx_fail(DX_EINVAL, "perturbation: duration below one control step");
  if (!T.nb && b->db.xfrc_stride)
    return dx_fail(DX_EINVAL, "perturbation: the env's batch already has per-env xfrc rows of the caller's (dx_set_xfrc_env)");
  const size_t E = e->P.nenv;
  if (!T.mt) {  // first use
    Perturb A{};
    int rc = balloc(b, (void**)&A.mt, E * DX_MTW_WORDS * 4);
    if (!rc) rc = balloc(b, (void**)&A.remain, E * DX_PERT_MAXB * 4);
    if (!rc) rc = balloc(b, (void**)&A.wrench, E * DX_PERT_MAXB * 6 * 4);
    if (rc) return rc;
    A.nenv = e->P.nenv;
    A.nbody = b->dm.nbody;
    A.step_type = e->S.step_type;
    A.episode = e->S.episode;
    A.base = b->xfrc;
    T = A;
  }
  if (!T.nb || !b->db.xfrc_stride) e->pt_shared = b->db.xfrc != nullptr;
  // env e draws from RandomState(seed + env0 + e)
  HIPCHK(seed_streams(e, p->seed, T.mt));
  if (int rc = perturb_clear(e)) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  for (int k = 0; k < DX_PERT_MAXB; k++) T.body[k] = k < p->nbody ? p->bodies[k] : 0;
  T.prob = p->probability;
  T.fmin = p->force_min; T.fmax = p->force_max;
  T.tmin = p->torque_min; T.tmax = p->torque_max;
  T.duration = p->duration;
  T.xfrc = b->xfrc_env;
  T.nb = p->nbody;
  return 0;
}

extern "C" int dx_env_perturb_draw(dx_env* e, int32_t n, double* out_host) {
  if (!e || !out_host) return dx_fail(DX_EINVAL, "null argument");
  if (!e->PT.nb) return dx_fail(DX_EINVAL, "the perturbation is not enabled");
  if (n < 1 || n > DX_WAVE) return dx_fail(DX_EINVAL, "between 1 and 64 doubles per call");
  return env_draw(e, n, out_host, "perturbation draw: ", [&](double* dev) {
    return dx_launch_perturb_draw(e->batch->stream, e->P.nenv, (int)n, e->PT.mt, dev);
  });
}

// ---- the optional hand observables (dx_observe.hip dx_hand_obs_kernel) ----
// Body poses of the env's CURRENT state into DX_XPOS / DX_XQUAT, for a batch that has been
// stepping without them: the step kernel itself (the batch's own specialization, so the
// poses are bit for bit those a step with body poses on would have left) launched over
// every env as a just-reset one -- no physics step, only the observation pass -- on a
// copy of the batch record whose every other output points at scratch memory.  The state
// arrays it stores back (qpos, qvel, warm start, time, step count) get the values it
// loaded.  Called with the stream drained; drains it again.
static int env_refresh_body_poses(dx_env* e) {
  dx_batch* b = e->batch;
  const DevModel& d = b->dm;
  const size_t E = b->nenv, ns = std::max(d.nsite, 1);
  const size_t words[] = {E, E, E, E, E * d.nv, E * 3 * ns, E * 6 * ns};  // skip, ncon, niter, ncand, qacc, sites
  size_t tot = 0;
  for (size_t w : words) tot += w;
  float* scratch = nullptr;
  HIPCHK(hipMalloc((void**)&scratch, tot * 4));
  std::vector<int> ones(E, 1);
  hipError_t err = hipMemcpy(scratch, ones.data(), E * 4, hipMemcpyHostToDevice);
  DevBatch B = b->db;
  float* p = scratch;
  B.skip = (const int*)p; p += words[0];
  B.ncon = (int*)p; p += words[1];
  B.niter = (int*)p; p += words[2];
  B.ncand = (int*)p; p += words[3];
  B.qacc = p; p += words[4];
  B.site_xpos = p; p += words[5];
  B.site_vel = p;
  B.out_bodies = 1;
  B.fuse = 0;
  B.order = nullptr;  // workgroup k takes env k
  B.cost = nullptr;
  B.onext = 0;
  B.bad = nullptr;    // (DX_DIVERGED keeps the last step's report)
  B.watch = nullptr;
  B.sen_stash = nullptr;
  B.stage_acc = nullptr;
  B.dbg_qacc_smooth = nullptr;
  B.mid = 0;
  if (err == hipSuccess)
    err = dx_launch_step(b->spec, b->nenv, (size_t)b->model->lds.total * 4, b->stream, b->dm_dev, B, b->model->lds,
                         e->nsub, 0);
  if (err == hipSuccess) err = hipStreamSynchronize(b->stream);
  (void)hipFree(scratch);
  if (err != hipSuccess) return dx_fail(DX_EHIP, std::string("hand observables: body poses: ") + hipGetErrorString(err));
  return 0;
}

extern "C" int dx_env_set_hand_observables(dx_env* e, const dx_hand_obs* cfg) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));  // may be called between steps
  const int mask = cfg ? cfg->mask : 0;
  const int all = DX_HOBS_JOINT_POSITIONS | DX_HOBS_TIP_ORIENTATIONS | DX_HOBS_TIP_ANGULAR_VELOCITIES |
                  DX_HOBS_TIP_POSITIONS_EGO;
  if (mask & ~all) return dx_fail(DX_EINVAL, "hand observables: unknown bit in the mask");
  // the mask sets the width of the observation pipeline's row
  if (e->O.on)
    return dx_fail(DX_EINVAL, "hand observables: switch the observation pipeline off first (dx_env_set_obs_pipeline(e, NULL))");
  HandObs& H = e->H;
  const TaskParams& P = e->P;
  const DevModel& d = b->dm;
  if (!mask) {  // off: a control step launches what an env never configured launches
    H.mask = 0;
    if (e->hobs_prev_bodies >= 0) b->db.out_bodies = e->hobs_prev_bodies;
    e->hobs_prev_bodies = -1;
    return 0;
  }
  const int nhands = P.kind == DX_KIND_HANDOVER ? 2 : 1;
  if (cfg->nhands != nhands) return dx_fail(DX_EINVAL, "hand observables: nhands differs from the task's hand count");
  for (int h = 0; h < nhands; h++)
    if (cfg->root_body[h] < 0 || cfg->root_body[h] >= d.nbody)
      return dx_fail(DX_EINVAL, "hand observables: root body outside [0, nbody)");
  if (P.hand_nq % nhands || P.ntips % nhands) return dx_fail(DX_EINVAL, "hand observables: the hands differ in size");
  const int hnq = P.hand_nq / nhands, nt = P.ntips / nhands;
  const int hand_dim = ((mask & DX_HOBS_JOINT_POSITIONS) ? hnq : 0) + ((mask & DX_HOBS_TIP_ORIENTATIONS) ? 4 * nt : 0) +
                       ((mask & DX_HOBS_TIP_ANGULAR_VELOCITIES) ? 3 * nt : 0) +
                       ((mask & DX_HOBS_TIP_POSITIONS_EGO) ? 3 * nt : 0);
  if (hand_dim < 1) return dx_fail(DX_EINVAL, "hand observables: the task has nothing of what the mask names");
  const int full = nhands * (hnq + 10 * nt);  // every observable on
  if ((size_t)P.nenv * full >= 0x7fffffffull) return dx_fail(DX_ELIMIT, "hand observables: nenv * width above 2^31");
  if (!H.out) {  // first use: the buffer at its full width, the task's fingertip sites and their site_quat
    HandObs A{};
    const auto& sq = b->model->hf.at("site_quat");
    std::vector<float> tq(4 * std::max(P.ntips, 1), 0.f);
    for (int t = 0; t < P.ntips; t++)
      for (int k = 0; k < 4; k++) tq[4 * t + k] = sq[4 * P.tip_sites[t] + k];
    int rc = balloc(b, (void**)&A.out, (size_t)P.nenv * full * 4);
    if (!rc) rc = balloc(b, (void**)&A.tip_site, (size_t)std::max(P.ntips, 1) * 4);
    if (!rc) rc = balloc(b, (void**)&A.tip_quat, tq.size() * 4);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));  // balloc zeroes on the stream: ahead of the copies
    HIPCHK(hipMemcpy((void*)A.tip_site, P.tip_sites, (size_t)P.ntips * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((void*)A.tip_quat, tq.data(), tq.size() * 4, hipMemcpyHostToDevice));
    const DevBatch& B = b->db;
    A.nenv = P.nenv; A.nq = d.nq; A.nsite = d.nsite; A.nbody = d.nbody;
    A.nhands = nhands; A.hand_nq = hnq; A.ntips = nt;
    A.qpos = B.qpos; A.site_xpos = B.site_xpos; A.site_vel = B.site_vel; A.xpos = B.xpos; A.xquat = B.xquat;
    A.site_bodyid = (const int*)d.site_bodyid;
    A.body_ipos = (const float*)d.body_ipos;
    A.body_imat = (const float*)d.body_imat;
    H = A;
  }
  // body poses of the current state, when the batch has been stepping without them
  if ((mask & HOBS_NEEDS_BODIES) && !b->db.out_bodies)
    if (int rc = env_refresh_body_poses(e)) return rc;
  if (mask & HOBS_NEEDS_BODIES) {
    if (e->hobs_prev_bodies < 0) e->hobs_prev_bodies = b->db.out_bodies;
    b->db.out_bodies = 1;
  } else if (e->hobs_prev_bodies >= 0) {
    b->db.out_bodies = e->hobs_prev_bodies;
    e->hobs_prev_bodies = -1;
  }
  for (int h = 0; h < nhands; h++) H.root[h] = cfg->root_body[h];
  H.hand_dim = hand_dim;
  H.dim = nhands * hand_dim;
  H.mask = mask;
  // the output holds the current state's values from here on (enabling mid-episode)
  if (int rc = env_hand_obs(e)) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// The cameras of the env's batch.  The batch of a dx_env steps without body poses by default:
// they are refreshed for the current state first, so the images the call leaves describe it.
extern "C" int dx_env_set_cameras(dx_env* e, const dx_camera* cams, int32_t ncam, int32_t width, int32_t height,
                                  int32_t flags) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  dx_batch* b = e->batch;
  const int bodies = b->db.out_bodies;
  if (int rc = dx_render_set_cameras(b, cams, ncam, width, height, flags)) return rc;
  if (!ncam) {
    if (e->H.mask & HOBS_NEEDS_BODIES) b->db.out_bodies = 1;  // the hand observables still read them
    return 0;
  }
  if (!bodies)
    if (int rc = env_refresh_body_poses(e)) return rc;
  if (int rc = dx_render(b)) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// The shading settings of the env's batch; RGB images that are on are rendered afresh.
extern "C" int dx_env_set_shading(dx_env* e, const float* geom_rgb, const int32_t* face_geom, const float* face_rgb,
                                  int32_t nface, const dx_light* lights, int32_t nlight, const dx_shading* shading) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  dx_batch* b = e->batch;
  if (int rc = dx_render_set_shading(b, geom_rgb, face_geom, face_rgb, nface, lights, nlight, shading)) return rc;
  if (!b->RA.ncam || !(b->rnd_flags & DX_RENDER_RGB)) return 0;
  if (int rc = dx_render(b)) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" int dx_env_hand_obs_dim(const dx_env* e) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  return e->H.mask ? e->H.dim : 0;
}

// ---- the contact forces of the task's pads (dx_sensor.hip, launched by env_observe) ----
extern "C" int dx_env_set_contact_forces(dx_env* e, int enable) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));  // may be called between steps
  if (!enable) {  // off: a control step launches what an env never configured launches
    e->cf_on = false;
    return stash_use(b, dx_batch::STASH_ENV, false);
  }
  // (a reach scene's pairs have a margin: a collision-free reset state can carry force,
  // and a reset env runs no forward pass that would solve it)
  if (e->P.kind == DX_KIND_REACH) return dx_fail(DX_EINVAL, "contact forces: the reach tasks have no prop to touch");
  const int npad = (int)e->cf_pads.size();
  if (npad < 1) return dx_fail(DX_EINVAL, "contact forces: no body has a collision pair with the prop");
  if (npad > DX_MAX_PADS) return dx_fail(DX_ELIMIT, "contact forces: more than 64 pads");
  const size_t bytes = (size_t)e->P.nenv * 3 * npad * 4;
  if (!e->cf_out) {
    float* out = nullptr;
    int* pads = nullptr;
    if (int rc = balloc(b, (void**)&out, bytes)) return rc;
    if (int rc = balloc(b, (void**)&pads, (size_t)npad * 8)) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));  // balloc zeroes on the stream: ahead of the copy
    HIPCHK(hipMemcpy(pads, e->cf_pads.data(), (size_t)npad * 8, hipMemcpyHostToDevice));
    e->cf_out = out;
    e->CF.pads = pads;
    e->CF.npad = npad;
    e->CF.first = e->S.step_type;
  }
  if (int rc = stash_use(b, dx_batch::STASH_ENV, true)) return rc;
  // zeros until the next step: the stash holds nothing of the current episode
  if (!e->cf_on) HIPCHK(hipMemset(e->cf_out, 0, bytes));
  e->cf_on = true;
  return 0;
}

extern "C" int dx_env_contact_force_dim(const dx_env* e) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  return e->cf_on ? 3 * (int)e->cf_pads.size() : 0;
}

extern "C" int dx_env_contact_force_bodies(const dx_env* e, int32_t* out, int32_t n) {
  if (!e || (n > 0 && !out)) return dx_fail(DX_EINVAL, "null argument");
  if (e->P.kind == DX_KIND_REACH) return dx_fail(DX_EINVAL, "contact forces: the reach tasks have no prop to touch");
  for (int k = 0; k < n && k < (int)e->cf_pads.size(); k++) out[k] = e->cf_pads[k].body;
  return (int)e->cf_pads.size();
}

// ---- the observation pipeline (dx_obspipe.hip dx_obs_pipe_kernel) ----
extern "C" int dx_env_set_obs_pipeline(dx_env* e, const dx_obs_pipeline* p) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));  // may be called between steps
  if (!p) {  // off: the step's launches, outputs and checkpoint are those of an env never configured
    obs_pipe_free(e->O);
    return 0;
  }
  // every check ahead of every change: a rejected call leaves the configuration as it was
  if (p->update_interval < 1 || p->update_interval > 64)
    return dx_fail(DX_EINVAL, "observation pipeline: update_interval outside 1..64 control steps");
  if (p->delay < 0 || p->delay > 64) return dx_fail(DX_EINVAL, "observation pipeline: delay outside 0..64 control steps");
  if (p->buffer_size < 1 || p->buffer_size > DX_OBSP_KMAX)
    return dx_fail(DX_EINVAL, "observation pipeline: buffer_size outside 1..16");
  if (p->aggregator < DX_OBS_AGG_NONE || p->aggregator > DX_OBS_AGG_SUM)
    return dx_fail(DX_EINVAL, "observation pipeline: unknown aggregator");
  if (p->padding != DX_OBS_PAD_ZERO && p->padding != DX_OBS_PAD_INITIAL)
    return dx_fail(DX_EINVAL, "observation pipeline: unknown padding");
  if (p->noise != 0 && p->noise != 1) return dx_fail(DX_EINVAL, "observation pipeline: noise must be 0 or 1");
  const int hand_dim = e->H.mask ? e->H.dim : 0;
  const int W = e->P.obs_dim + hand_dim;
  if (p->noise) {
    if (!p->noise_sigma || p->nsigma != W)
      return dx_fail(DX_EINVAL, "observation pipeline: noise needs one sigma per row element (nsigma = obs_dim + hand_obs_dim)");
    for (int i = 0; i < W; i++)
      if (!std::isfinite(p->noise_sigma[i]) || p->noise_sigma[i] < 0.0)
        return dx_fail(DX_EINVAL, "observation pipeline: every sigma must be finite and non-negative");
  }
  const int m = p->update_interval, d = p->delay, K = p->buffer_size;
  const int S = K + (d + m - 1) / m;
  if (S > DX_OBSP_SLOTS_MAX) return dx_fail(DX_ELIMIT, "observation pipeline: more than 80 ring slots");
  if (W > DX_OBSP_WMAX) return dx_fail(DX_ELIMIT, "observation pipeline: a row above 512 floats");
  ObsPipe A{};
  A.nenv = e->P.nenv; A.obs_dim = e->P.obs_dim; A.hand_dim = hand_dim;
  A.W = W; A.Wp = (W + 31) & ~31;
  A.m = m; A.d = d; A.K = K; A.S = S;
  A.agg = p->aggregator; A.pad = p->padding; A.noise = p->noise;
  A.obs = e->S.obs; A.hand = hand_dim ? e->H.out : nullptr; A.step_type = e->S.step_type;
  const size_t E = e->P.nenv, nout = E * (A.agg ? 1 : K) * W;
  hipError_t err = hipMalloc((void**)&A.ring, E * S * A.Wp * 4);
  if (err == hipSuccess) err = hipMalloc((void**)&A.count, E * 4);
  if (err == hipSuccess) err = hipMalloc((void**)&A.out, nout * 4);
  if (err == hipSuccess) err = hipMemsetAsync(A.ring, 0, E * S * A.Wp * 4, b->stream);
  if (err == hipSuccess) err = hipMemsetAsync(A.count, 0, E * 4, b->stream);
  if (err == hipSuccess && p->noise) {  // env e draws from RandomState(noise_seed + env0 + e)
    err = hipMalloc((void**)&A.mt, E * DX_MTW_WORDS * 4);
    if (err == hipSuccess) err = hipMalloc((void**)&A.sigma, (size_t)W * 8);
    if (err == hipSuccess) err = hipMemcpyAsync((void*)A.sigma, p->noise_sigma, (size_t)W * 8, hipMemcpyHostToDevice, b->stream);
    if (err == hipSuccess) err = seed_streams(e, p->noise_seed, A.mt);
  }
  // every env's history afresh from its current row: n = 0, s_0 taken (and corrupted), the
  // buffer left holding that read
  if (err == hipSuccess) err = dx_launch_obs_pipe(b->stream, A, 1);
  if (err == hipSuccess) err = hipStreamSynchronize(b->stream);  // (the sigma copy has read the caller's array)
  if (err != hipSuccess) {
    obs_pipe_free(A);
    return dx_fail(err == hipErrorOutOfMemory ? DX_ENOMEM : DX_EHIP, std::string("observation pipeline: ") + hipGetErrorString(err));
  }
  obs_pipe_free(e->O);
  A.on = 1;
  e->O = A;
  return 0;
}

extern "C" int dx_env_obs_pipe_dims(const dx_env* e, int32_t out[3]) {
  if (!e || !out) return dx_fail(DX_EINVAL, "null argument");
  out[0] = e->P.obs_dim + (e->H.mask ? e->H.dim : 0);
  out[1] = !e->O.on ? 0 : e->O.agg ? 1 : e->O.K;
  out[2] = e->O.on;
  return 0;
}

extern "C" int dx_env_obs_noise_draw(dx_env* e, int32_t n, double* out_host) {
  if (!e || !out_host) return dx_fail(DX_EINVAL, "null argument");
  if (!e->O.on || !e->O.noise) return dx_fail(DX_EINVAL, "observation noise is not enabled");
  if (n < 1 || n > DX_WAVE) return dx_fail(DX_EINVAL, "between 1 and 64 normals per call");
  return env_draw(e, n, out_host, "observation noise draw: ", [&](double* dev) {
    return dx_launch_obs_noise_draw(e->batch->stream, e->P.nenv, (int)n, e->O.mt, dev);
  });
}

static int env_params_upload(dx_env* e) {
  HIPCHK(hipSetDevice(e->batch->device));
  HIPCHK(hipStreamSynchronize(e->batch->stream));  // the device copy is read by the sampling pass
  HIPCHK(hipMemcpy((void*)e->batch->db.tp, &e->P, sizeof(TaskParams), hipMemcpyHostToDevice));
  return 0;
}

extern "C" int dx_env_set_time_limit(dx_env* e, double seconds) {
  if (!e || !(seconds > 0)) return dx_fail(DX_EINVAL, "null env or non-positive time limit");
  e->P.time_limit = (float)seconds;
  e->P.time_limit_d = seconds;
  return env_params_upload(e);
}

extern "C" int dx_env_set_goal_time_limit(dx_env* e, double seconds) {
  if (!e || !(seconds >= 0)) return dx_fail(DX_EINVAL, "null env or negative time");
  e->P.max_time = (float)seconds;
  e->P.max_time_d = seconds;
  return env_params_upload(e);
}

extern "C" int dx_env_step(dx_env* e, const float* action) {
  if (!e || !action) return dx_fail(DX_EINVAL, "null env or action");
  return env_run(e, action);
}

extern "C" int dx_env_step_random(dx_env* e, uint64_t seed, int32_t step) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  return env_run(e, nullptr, true, seed, step);
}

// checkpoint / resume: every device array whose contents carry from one
// control step to the next -- physics state (qpos, qvel, ctrl, warm start, fp32 time, the
// physics-step count behind the fp64 time), task state (goals, counters, step types, fp64
// times, observation, rewards), both numpy-compatible MT19937 streams of an env (reach:
// the RandomState block with numpy's cached gaussian), and the longest-first order.  The
// separating-direction cache is left out: it never changes a result (dx_step.hip
// mpr_init).  Restoring into an env of the same task, model and size resumes the run bit
// for bit.
struct StateField {
  const char* name;
  void* ptr;
  size_t bytes;
};
static std::vector<StateField> env_state_fields(dx_env* e) {
  dx_batch* b = e->batch;
  const DevBatch& B = b->db;
  const TaskState& S = e->S;
  const TaskParams& P = e->P;
  const size_t E = b->nenv;
  const DevModel& d = b->dm;
  std::vector<StateField> f = {
      {"qpos", B.qpos, E * d.nq * 4}, {"qvel", B.qvel, E * d.nv * 4},
      {"ctrl", B.ctrl, E * std::max(d.nu, 1) * 4}, {"qacc_warmstart", B.qacc_ws, E * d.nv * 4},
      {"qacc", B.qacc, E * d.nv * 4}, {"time", B.time, E * 4}, {"nstep", B.nstep, E * 4},
      {"diverged", B.bad, E * 4},
      {"goal", S.goal, E * P.goal_dim * 4}, {"solve_start", S.solve_start, E * 4},
      {"reward", S.reward, E * 4}, {"discount", S.discount, E * 4}, {"obs", S.obs, E * P.obs_dim * 4},
      {"successes", S.successes, E * 4}, {"counter", S.counter, E * 4}, {"registered", S.registered, E * 4},
      {"exceeded", S.exceeded, E * 4}, {"step_type", S.step_type, E * 4}, {"episode", S.episode, E * 4},
      {"skip", S.skip, E * 4}, {"failure", S.failure, E * 4}, {"need", S.need, E * 4},
      {"goalnum", S.goalnum, E * 4}, {"goalfail", S.goalfail, E * 4}, {"time_d", S.time_d, E * 8},
      {"solve_start_d", S.solve_start_d, E * 8}, {"nsub_d", S.nsub_d, E * 4}, {"solve_n", S.solve_n, E * 4},
  };
  if (S.goal_qpos) f.push_back({"goal_qpos", S.goal_qpos, E * d.nq * 4});
  if (S.mt_env) f.push_back({"mt_env", S.mt_env, E * DX_MT_WORDS * 4});
  if (S.mt_goal) f.push_back({"mt_goal", S.mt_goal, E * DX_MT_WORDS * 4});
  if (S.mt_reach) f.push_back({"mt_reach", S.mt_reach, E * DX_MTW_WORDS * 4});
  if (B.cost) f.push_back({"step_cost", B.cost, E * 4});
  if (B.order) f.push_back({"order", (void*)B.order, E * 4});
  if (e->F.flags) {  // the action pipeline's state, while it is enabled (its configuration is not saved)
    const ActFilter& F = e->F;
    f.push_back({"act_ema", F.ema, E * d.nu * 4});
    f.push_back({"act_ema_set", F.ema_set, E * 4});
    f.push_back({"prev_action", F.prev, E * d.nu * 4});
    f.push_back({"mt_noise", F.mt, E * DX_MTW_WORDS * 4});
  }
  // the hand observables' rows, while they are on (their configuration is not saved): a
  // loaded env reads what the saved one would have, before its next step rewrites them
  if (e->H.mask) f.push_back({"hand_obs", e->H.out, E * e->H.dim * 4});
  if (e->O.on) {  // the observation pipeline's state, while it is on (its configuration is not saved)
    const ObsPipe& O = e->O;
    f.push_back({"obs_ring", O.ring, E * O.S * O.Wp * 4});
    f.push_back({"obs_count", O.count, E * 4});
    if (O.noise) f.push_back({"mt_obs_noise", O.mt, E * DX_MTW_WORDS * 4});
    f.push_back({"obs_buffer", O.out, E * (O.agg ? 1 : O.K) * O.W * 4});
  }
  // the contact forces' rows, while they are on (as the hand observables' rows above)
  if (e->cf_on) f.push_back({"contact_force", e->cf_out, E * 3 * e->cf_pads.size() * 4});
  if (e->PT.nb) {  // the pushes' state, while they are on (their configuration is not saved)
    const Perturb& T = e->PT;
    f.push_back({"perturb_remain", T.remain, E * T.nb * 4});
    f.push_back({"perturb_wrench", T.wrench, E * T.nb * 6 * 4});
    f.push_back({"mt_perturb", T.mt, E * DX_MTW_WORDS * 4});
  }
  return f;
}

extern "C" int dx_env_state_field(dx_env* e, int32_t i, const char** name, size_t* offset, size_t* nbytes) {
  if (!e || !name || !offset || !nbytes) return dx_fail(DX_EINVAL, "null argument");
  const auto f = env_state_fields(e);
  if (i < 0) return (int)f.size();
  if (i >= (int)f.size()) return dx_fail(DX_EINVAL, "state field out of range");
  size_t off = 0;
  for (int k = 0; k < i; k++) off += f[k].bytes;
  *name = f[i].name;
  *offset = off;
  *nbytes = f[i].bytes;
  return (int)f.size();
}

extern "C" int dx_env_save(dx_env* e, void* dst, size_t nbytes) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  const auto f = env_state_fields(e);
  size_t tot = 0;
  for (auto& x : f) tot += x.bytes;
  if (!dst) return (int)std::min<size_t>(tot, 0x7fffffff);  // the size query
  if (nbytes < tot) return dx_fail(DX_EINVAL, "checkpoint buffer too small");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  size_t off = 0;
  for (auto& x : f) {
    HIPCHK(hipMemcpyAsync((char*)dst + off, x.ptr, x.bytes, hipMemcpyDefault, b->stream));
    off += x.bytes;
  }
  HIPCHK(hipStreamSynchronize(b->stream));
  return queue_check(b);
}

extern "C" int dx_env_load(dx_env* e, const void* src, size_t nbytes) {
  if (!e || !src) return dx_fail(DX_EINVAL, "null argument");
  const auto f = env_state_fields(e);
  size_t tot = 0;
  for (auto& x : f) tot += x.bytes;
  if (nbytes != tot) return dx_fail(DX_EINVAL, "checkpoint size does not match this env (task, model, batch size)");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  size_t off = 0;
  for (auto& x : f) {
    HIPCHK(hipMemcpyAsync(x.ptr, (const char*)src + off, x.bytes, hipMemcpyDefault, b->stream));
    off += x.bytes;
  }
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" int dx_env_output(dx_env* e, int which, void** devptr) {
  if (!e || !devptr) return dx_fail(DX_EINVAL, "null argument");
  switch (which) {
    case DX_OUT_OBS: *devptr = e->S.obs; return 0;
    case DX_OUT_REWARD: *devptr = e->S.reward; return 0;
    case DX_OUT_DISCOUNT: *devptr = e->S.discount; return 0;
    case DX_OUT_STEP_TYPE: *devptr = e->S.step_type; return 0;
    case DX_OUT_GOAL: *devptr = e->S.goal; return 0;
    case DX_OUT_SUCCESSES: *devptr = e->S.successes; return 0;
    case DX_OUT_GOAL_FAILURES: *devptr = e->S.goalfail; return 0;
    case DX_OUT_GOAL_QPOS:
      if (!e->S.goal_qpos) return dx_fail(DX_EINVAL, "goal joints exist for the reach task only");
      *devptr = e->S.goal_qpos;
      return 0;
    case DX_OUT_PREV_ACTION:
      if (!e->F.prev) return dx_fail(DX_EINVAL, "no previous action: the action pipeline was never configured");
      *devptr = e->F.prev;
      return 0;
    case DX_OUT_HAND_OBS:
      if (!e->H.mask) return dx_fail(DX_EINVAL, "no hand observables: dx_env_set_hand_observables has none enabled");
      *devptr = e->H.out;
      return 0;
    case DX_OUT_OBS_BUFFER:
      if (!e->O.on) return dx_fail(DX_EINVAL, "no observation buffer: the observation pipeline is off (dx_env_set_obs_pipeline)");
      *devptr = e->O.out;
      return 0;
    case DX_OUT_CONTACT_FORCE:
      if (!e->cf_on) return dx_fail(DX_EINVAL, "no contact forces: dx_env_set_contact_forces has not enabled them");
      *devptr = e->cf_out;
      return 0;
    case DX_OUT_PERTURB:
      if (!e->PT.nb) return dx_fail(DX_EINVAL, "no pushes: dx_env_set_perturbation has not enabled them");
      *devptr = e->PT.wrench;
      return 0;
    case DX_OUT_DEPTH:
      if (!e->batch->RA.ncam || !(e->batch->rnd_flags & DX_RENDER_DEPTH))
        return dx_fail(DX_EINVAL, "no depth images: dx_env_set_cameras has no camera with DX_RENDER_DEPTH on");
      *devptr = e->batch->RA.depth;
      return 0;
    case DX_OUT_SEGMENTATION:
      if (!e->batch->RA.ncam || !(e->batch->rnd_flags & DX_RENDER_SEGMENTATION))
        return dx_fail(DX_EINVAL, "no segmentation images: dx_env_set_cameras has no camera with DX_RENDER_SEGMENTATION on");
      *devptr = e->batch->RA.seg;
      return 0;
    case DX_OUT_RGB:
      if (!e->batch->RA.ncam || !(e->batch->rnd_flags & DX_RENDER_RGB))
        return dx_fail(DX_EINVAL, "no RGB images: dx_env_set_cameras has no camera with DX_RENDER_RGB on");
      *devptr = e->batch->rnd_rgb;
      return 0;
  }
  return dx_fail(DX_EINVAL, "unknown output");
}

extern "C" int dx_env_action_buffer(dx_env* e, void** devptr) {
  if (!e || !devptr) return dx_fail(DX_EINVAL, "null argument");
  if (e->allocs.empty()) {
    void* p = nullptr;
    if (int rc = balloc(e->batch, &p, (size_t)e->P.nenv * std::max(e->P.nu, 1) * 4)) return rc;
    e->allocs.push_back(p);
  }
  *devptr = e->allocs[0];
  return 0;
}

extern "C" int dx_env_sample_actions(dx_env* e, uint64_t seed, int32_t step) {
  if (!e) return dx_fail(DX_EINVAL, "null env");
  void* buf = nullptr;
  if (int rc = dx_env_action_buffer(e, &buf)) return rc;
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  int n = e->P.nenv * e->P.nu;
  hipLaunchKernelGGL(dx_sample_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, b->stream, e->P.nenv,
                     e->P.nu, b->dm.actuator_ctrlrange, seed, step, e->P.env0, (float*)buf);
  HIPCHK(hipGetLastError());
  return 0;
}

// packs [obs | reward | discount | step_type] per env into dst (device, [nenv][obs_dim+3])
extern "C" __global__ void dx_pack_outputs_kernel(int nenv, int obs_dim, const float* obs, const float* rew,
                                                  const float* disc, const int* st, float* dst);

extern "C" int dx_env_pack_outputs(dx_env* e, float* dst_dev) {
  if (!e || !dst_dev) return dx_fail(DX_EINVAL, "null argument");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  int n = e->P.nenv * (e->P.obs_dim + 3);
  hipLaunchKernelGGL(dx_pack_outputs_kernel, dim3((n + 255) / 256), dim3(256), 0, b->stream, e->P.nenv,
                     e->P.obs_dim, e->S.obs, e->S.reward, e->S.discount, e->S.step_type, dst_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

// The reference's own call shape: GoalEnvironment.step(action) with a host action and a
// host TimeStep back (environment.py:25-34, task.py:63-73).  One stream: the action's
// upload into the library's action buffer, the control step, the pack of [obs | reward |
// discount | step_type] and its download, then one synchronisation.  With page-locked
// host buffers both copies are DMA transfers queued behind / ahead of the kernels.
extern "C" int dx_env_step_host(dx_env* e, const float* action_host, float* out_host) {
  if (!e || !action_host || !out_host) return dx_fail(DX_EINVAL, "null argument");
  dx_batch* b = e->batch;
  HIPCHK(hipSetDevice(b->device));
  void* act = nullptr;
  if (int rc = dx_env_action_buffer(e, &act)) return rc;
  const size_t nout = (size_t)e->P.nenv * (e->P.obs_dim + 3);
  if (e->allocs.size() < 2) {  // the packed outputs' device buffer
    void* p = nullptr;
    if (int rc = balloc(b, &p, nout * 4)) return rc;
    e->allocs.push_back(p);
  }
  float* pack = (float*)e->allocs[1];
  HIPCHK(hipMemcpyAsync(act, action_host, (size_t)e->P.nenv * e->P.nu * 4, hipMemcpyHostToDevice, b->stream));
  if (int rc = env_run(e, (const float*)act)) return rc;
  if (int rc = dx_env_pack_outputs(e, pack)) return rc;
  HIPCHK(hipMemcpyAsync(out_host, pack, nout * 4, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}
