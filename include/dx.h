/*
 * dx.h -- C ABI of the MI355X batched physics step (libdx.so).
 *
 * This is the drop-in boundary for the reference's hot path.  In the reference
 * (v-wewei/dexterity) every environment owns one MuJoCo mjModel/mjData pair behind
 * dm_control's `mjcf.Physics`, and the path is driven through these calls
 * ([3P] MuJoCo C API):
 *
 *   physics.step()            -> mj_step2(m,d); mj_step1(m,d)   (composer substep loop,
 *                                 reorient.py:58,61,168 / reach.py:54,59,139)
 *   physics.forward()         -> mj_forward(m,d)                (fingertip_position.py:95)
 *   physics.bind(acts).ctrl=  -> d->ctrl                        (effectors/mujoco_actuation.py:33)
 *   bind(joints).qpos/.qvel   -> d->qpos / d->qvel              (shadow_hand_e.py:121, reorient.py:187)
 *   xfrc_applied[:] = -m g    -> d->xfrc_applied                (utils/mujoco_utils.py:91-99)
 *   bind(sites).xpos          -> d->site_xpos                   (dexterous_hand.py:286-291)
 *   physics.data.contact      -> d->contact, d->ncon            (utils/mujoco_collisions.py:95-119)
 *
 * Here one handle (`dx_batch`) owns B environments that share one compiled model;
 * all state stays resident in HBM and one call advances every environment.
 *
 * Conventions:
 *  - every function returns 0 on success or a negative DX_E* code; the message of
 *    the last failure on the calling thread is in dx_last_error();
 *  - state arrays are float32, environment-major: field[env][n];
 *  - pointers passed to dx_set_field / dx_get_field may be host or device memory
 *    (resolved through HIP's unified addressing);
 *  - calls on one dx_batch are serialised on its own HIP stream; a dx_batch is not
 *    thread-safe; different handles are independent;
 *  - the library owns all device memory it allocates.
 */
#ifndef DX_H
#define DX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DX_ABI_VERSION 1

typedef struct dx_model dx_model;
typedef struct dx_batch dx_batch;

enum dx_error {
  DX_OK = 0,
  DX_EINVAL = -1,   /* bad argument                        */
  DX_EMODEL = -2,   /* malformed or unsupported model blob */
  DX_EHIP = -3,     /* HIP runtime failure                 */
  DX_ENOMEM = -4,   /* allocation failure                  */
  DX_ELIMIT = -5    /* model exceeds kernel limits         */
};

/* Per-environment fields addressable through dx_set_field / dx_get_field /
 * dx_field_ptr.  Widths are per environment. */
enum dx_field {
  DX_QPOS = 0,          /* nq                                    rw */
  DX_QVEL = 1,          /* nv                                    rw */
  DX_CTRL = 2,          /* nu                                    rw */
  DX_QACC_WARMSTART = 3,/* nv                                    rw */
  DX_QACC = 4,          /* nv   last solved acceleration         r  */
  DX_TIME = 5,          /* 1                                     rw */
  DX_SITE_XPOS = 6,     /* 3*nsite  (after dx_step / dx_forward) r  */
  DX_SITE_VEL = 7,      /* 6*nsite  linear(3) + angular(3), world frame, at site r */
  DX_XPOS = 8,          /* 3*nbody                               r  */
  DX_XQUAT = 9,         /* 4*nbody                               r  */
  DX_NCON = 10,         /* 1  (int32 bits)                       r  */
  DX_GROUND_CONTACT = 11, /* 1 (int32 bits): any contact involving geom
                           `ground_geom` with dist <= 1e-8 (reorient.py:229-235) */
  DX_NITER = 12,        /* 1  (int32 bits) solver iterations of the last substep */
  DX_NCAND = 13,        /* 1  (int32 bits) narrowphase candidates of the last collision pass */
  DX_STEP_COST = 14,    /* 1  (uint32 bits) shader cycles / 1024 the env's last dx_step took
                           (feeds the longest-first dispatch order; 0 if disabled) */
  DX_SENSOR_TORQUE = 15,/* 3*nbody  r  (after dx_sensor_enable): 3-axis `torque` sensor of a
                           site at each body's origin, in the body frame -- the joint torque
                           sensors of shadow_hand_e.py:176-196 / adroit_hand.py:153-172
                           (mj_rnePostConstraint + mj_sensorAcc of the last substep, before
                           its integration, as after dm_control's physics.step()) */
  DX_DIVERGED = 16,     /* 1  (int32 bits) r: the env's state diverged during the last dx_step /
                           dx_forward (a non-finite qpos / qvel / qacc, or |qacc| > 1e10: MuJoCo's
                           BADQACC, [3P] mj_checkAcc) and was reset to qpos0 (mj_resetData) */
  DX_CFRC_EXT = 17,     /* 6*nbody  r  (after dx_contact_enable): MuJoCo's cfrc_ext, per body
                           [torque(3) about the subtree com of the body's tree root, force(3)],
                           world axes; the world body's row is zero */
  DX_PAD_FORCE = 18,    /* 3*npad   r  (after dx_contact_enable, pads from dx_contact_set_pads):
                           per pad the contact force on its body, in the body's frame.  The pads
                           are a batch's: dx_field_width (a model's) answers 0, a batch's width is
                           3 * dx_contact_npad */
  DX_NFIELD
};

/* Model ------------------------------------------------------------------ */
/* Loads a compiled-model blob (dexterity_amd/blob.py).  The blob is copied. */
dx_model* dx_model_load(const void* blob, size_t nbytes);
void dx_model_free(dx_model* m);
/* Sizes: out[0..11] = nq nv nbody njnt ngeom nsite nu ntendon nbpair ngpair ncon_max nefc_max
 * (ncon_max / nefc_max: the contact pool and constraint-row capacity of a physics step,
 * DX_NCON_HI = 256 contacts with the overflow tier) */
int dx_model_sizes(const dx_model* m, int32_t out[12]);
/* Bytes of LDS one environment (one 64-lane workgroup) of dx_step uses. */
int dx_model_lds_bytes(const dx_model* m);
/* Test hook: index of the vertex the device's support scan returns for hull `mesh`
   along local direction dir (direction-binned hulls); info =
   [vertex, cube-map cells per face edge (0: not binned), cell capacity]. */
int dx_hull_support(const dx_model* m, int32_t mesh, const float dir[3], int32_t info[3]);
/* Build hook: the per-env LDS layout (dx_internal.h Lds, in words) followed by 16
   model dimensions, for compile-time kernel specialization; returns the count. */
int dx_model_layout(const dx_model* m, int32_t* out, int32_t n);
/* Width (in 4-byte words per environment) of a dx_field. */
int dx_field_width(const dx_model* m, int field);

/* Batch ------------------------------------------------------------------ */
/* Allocates nenv environments on HIP device `device`, reset to qpos0. */
dx_batch* dx_batch_create(const dx_model* m, int32_t nenv, int32_t device);
void dx_batch_destroy(dx_batch* b);
int dx_batch_nenv(const dx_batch* b);
/* Resets environments [env0, env0+n) to qpos0, zero velocity, zero ctrl. */
int dx_reset(dx_batch* b, int32_t env0, int32_t n);

/* Copies n environments' worth of a field, starting at env0. */
int dx_set_field(dx_batch* b, int field, const void* src, int32_t env0, int32_t n);
int dx_get_field(dx_batch* b, int field, void* dst, int32_t env0, int32_t n);
/* Device pointer of a field's [nenv][width] array (zero-copy access). */
int dx_field_ptr(dx_batch* b, int field, void** devptr);
/* Applied body wrenches, MuJoCo's d->xfrc_applied: per body (force, torque) in the world
 * frame at the body's com.  A batch holds them in one of two modes.
 *  shared   one xfrc_applied[nbody][6] read by every env: dx_set_xfrc, the
 *    gravity-compensation write of utils/mujoco_utils.py:91-99 (NULL: none).  The default.
 *  per-env  rows [nenv][nbody][6], every env its own as in MjData: dx_set_xfrc_env writes
 *    rows [n][nbody][6] for envs env0 .. env0+n-1 from host or device memory (as
 *    dx_set_field).  The call that leaves shared mode first gives every env the shared
 *    array's rows (zeros when none is set), so envs outside [env0, env0+n) keep what they
 *    had been reading.  The step's arithmetic is the same in both modes: per-env rows that
 *    all equal the shared array give the shared mode's bits.
 * dx_set_xfrc (an array, or NULL) returns the batch to shared mode.  dx_get_xfrc_env reads
 * back what env0 .. env0+n-1 read, in either mode (it synchronises the stream).
 * dx_xfrc_ptr gives the per-env rows' device address and the stride between two envs in
 * floats (6 * nbody; stride may be null) for writes from device code on dx_stream, and
 * DX_EINVAL in shared mode.  dx_reset does not touch applied wrenches in either mode
 * (mj_resetData zeroes them; here the gravity compensation is set once and must survive
 * every reset, and the per-env rows follow the same rule). */
int dx_set_xfrc(dx_batch* b, const float* xfrc, int32_t nbody);
int dx_set_xfrc_env(dx_batch* b, const float* xfrc, int32_t env0, int32_t n);
int dx_get_xfrc_env(dx_batch* b, float* dst, int32_t env0, int32_t n);
int dx_xfrc_ptr(dx_batch* b, void** devptr, int32_t* stride);
/* Geom whose contacts set DX_GROUND_CONTACT (-1 disables). */
int dx_set_ground_geom(dx_batch* b, int32_t geom);
/* DX_GROUND_CONTACT watches contacts between `geom` and any geom of `body`
 * (reorient.py:229-235: prop geoms vs the arena ground). */
int dx_set_watch(dx_batch* b, int32_t geom, int32_t body);

/* Stepping --------------------------------------------------------------- */
/* Advances every environment by nsubstep physics steps (ctrl held constant),
 * then recomputes position-dependent outputs (site poses, velocities, ground
 * contact) at the new state: the step2->step1 contract of dm_control. */
int dx_step(dx_batch* b, int32_t nsubstep);
/* mj_forward equivalent: outputs at the current state, no integration. */
int dx_forward(dx_batch* b);
/* Stream the batch's kernels are enqueued on (hipStream_t) and a blocking sync. */
void* dx_stream(dx_batch* b);
int dx_sync(dx_batch* b);

/* Whether dx_step / dx_forward write the body poses DX_XPOS / DX_XQUAT (default 1 for
 * a dx_batch, 0 for the batch of a dx_env, whose tasks never read them: 28 B per body
 * and env-step of HBM writes saved). */
int dx_set_outputs(dx_batch* b, int bodies);

/* Sensors ---------------------------------------------------------------- */
/* Enables DX_SENSOR_TORQUE: dx_step / dx_forward then also compute every body's torque
 * sensor (one extra small kernel per call; nothing when disabled). */
int dx_sensor_enable(dx_batch* b, int enable);

/* Contact force sensing -------------------------------------------------- */
/* The contact forces the step solves, read back from the same stash and in the same small
 * kernel as the torque sensors (one launch for both when both are on; nothing when all is
 * off), with their timing: after dx_step(n) they describe the last physics step before its
 * integration (mj_sensorAcc in mj_step2, as after dm_control's physics.step()), after
 * dx_forward the current state.  Contacts up to DX_NCON_HI, whichever tier ran the step; the
 * sums run in the contact list's order, so results are deterministic.
 *  DX_CFRC_EXT   [3P] mj_rnePostConstraint's cfrc_ext: xfrc_applied moved from xipos, plus
 *    every contact's force (+ on its body 2, - on its body 1), layout and content as
 *    d->cfrc_ext.
 *  DX_PAD_FORCE  for each configured pad {body, partner_body}: the sum of the forces that
 *    contacts with partner_body (-1: any body, the world body's geoms included) exert on
 *    body, in body's frame at that state (xmat^T F).  No torque and no count; a MuJoCo
 *    `touch` scalar needs the contact normal, which the stash does not carry.
 * dx_contact_set_pads: npad = 0 clears the pads; DX_EINVAL when a body is outside [1, nbody)
 * or a partner outside [-1, nbody), DX_ELIMIT above 64 pads; a rejected call leaves the
 * configuration unchanged.  It synchronises the stream, and the rows read zero until the
 * next dx_step / dx_forward. */
int dx_contact_enable(dx_batch* b, int enable);
typedef struct { int32_t body, partner_body; } dx_contact_pad;
int dx_contact_set_pads(dx_batch* b, const dx_contact_pad* pads, int32_t npad);
int dx_contact_npad(const dx_batch* b);

/* Health (always on) ----------------------------------------------------- */
/* Counters of capacity overflows and divergences since the batch was created or last
 * cleared, out[0 .. min(n, DX_HEALTH_WORDS)):
 *   0 env-substeps that found more contacts than the contact pool holds, DX_NCON_HI = 256
 *     (above the Shadow scenes' nconmax = 200, shadow_hand_series_e.xml:8): the first 256
 *     in generation (candidate) order are kept, as MuJoCo fills its pool and drops the
 *     rest with mjWARN_CONTACTFULL
 *   1 env-substeps whose broadphase / narrowphase candidate lists overflowed
 *   2 contacts whose Jacobian spans more than DX_DOFMAX dofs (truncated)
 *   3 env-substeps with more constraint rows than the LDS block holds (truncated)
 *   4 env-substeps that diverged (DX_DIVERGED) and reset their env
 *   5 the most contacts one env-substep found, when above 16 (else 0)
 *   6 env-substeps that found more than the 32 contacts the step kernel keeps in LDS and
 *     were therefore run by a larger pool -- the mid tier (64 contacts, beside a queued
 *     step launch on a side stream) or the overflow tier (256, behind the launch), the
 *     same physics: not a truncation
 *   7 mid-tier launches that stopped waiting for deferrals before their step launch ended
 *     (~14 ms without a finished task: a serialised dispatch order or an aborted launch)
 *   8 step-kernel deferrals run by the overflow tier behind the launch instead of by the
 *     mid tier beside it (words 7 and 8: speed only, the same physics)
 * then, when the histogram is on (dx_ncon_histogram), out[16 .. 16 + 65): env-substeps
 * by contacts found (bins 0..63, then >= 64).  Synchronises the batch's stream. */
#define DX_HEALTH_WORDS 16
#define DX_NCON_HIST 65
int dx_health(dx_batch* b, uint32_t* out, int32_t n);
int dx_health_clear(dx_batch* b);
int dx_ncon_histogram(dx_batch* b, int enable);

/* Debug / parity -------------------------------------------------------- */
/* When enabled, dx_forward/dx_step record per-env intermediates of the LAST
 * substep: qacc_smooth, qfrc_bias(+applied), qfrc_actuator, M (nv*nv), contacts. */
int dx_debug_enable(dx_batch* b, int enable);
/* name: "qacc_smooth" "qfrc_smooth" "M" "contact" (16 floats/contact: pos3 frame9
 * dist geom1 geom2 condim) "efc_count" ; dst is host memory for all envs.
 * "health" (no dx_debug_enable needed): dx_health's words, as uint32 bits.
 * "queue_timeouts" (1 word, int32 bits, no dx_debug_enable needed): nonzero if a
 * task of the substep queue ever stopped waiting for its predecessor. */
int dx_debug_get(dx_batch* b, const char* name, float* dst, size_t nfloats);

/* Environments: a dx_batch plus on-device task logic ------------------- */
/* One dx_env is B copies of a reference task (composer.Environment + Task,
 * environment.py:9-34, task.py:137-204): dx_env_step = GoalTask.before_step,
 * n_sub_steps physics steps, after_step, reward, discount, termination and the
 * observation vector, for every env, with dm_env auto-reset (an env that returned
 * LAST is re-initialised by its next step and returns FIRST). */
typedef struct dx_env dx_env;
enum dx_task_kind { DX_TASK_REORIENT = 0, DX_TASK_REACH = 1, DX_TASK_HANDOVER = 2 };
/* Reorient params (float[26], or float[38] with the fp64 bbox), reorient.py:40-78 / task.py:120-135:
 *  0 n_sub_steps  1 hand_nq  2 hand_nv  3 prop_qposadr  4 prop_dofadr
 *  5 first fingertip site  6 n fingertips  7 successes_needed
 *  8 steps_before_changing_goal  9 fall_termination  10 success_threshold
 *  11 orientation_eps  12 w_orientation  13 w_success  14 w_action
 *  15 max_time_per_goal  16-18 prop bbox lower  19-21 prop bbox upper
 *  22 ground geom  23 prop body  24-25 reserved
 *  26-37 (optional) the bbox in fp64: raw bits of lower[3], upper[3] (two words each)
 * Randomness: env e draws from numpy-compatible MT19937 streams seeded with
 * seed + e -- its RandomState (PropPlacer) and numpy's global stream (goals, which
 * the reference's PropOrientation draws from np.random: prop_orientation.py:38). */
#define DX_REORIENT_NPARAMS 26
/* Reach params (float[26 + 3*nq + nu*nq]), reach.py:43-70, task.py:120-135,
 * fingertip_position.py:21-35, dexterous_hand.py:120-168:
 *  0 n_sub_steps  1 hand_nq (= nq)  2 hand_nv  3 n fingertips  4-8 fingertip sites
 *  9 successes_needed  10 steps_before_changing_goal  11 success_threshold
 *  12 max_time_per_goal  13 dense reward (1) / sparse (0)  14 init joint range fraction
 *  15 goal sampling scale  16 max rejection samples  17 n coupled joint pairs
 *  18-25 coupled pairs (joint, source joint): qpos[joint] = qpos[source]
 *  26..  joint midrange [nq], lower [nq], upper [nq], position->control [nu][nq]
 *  then, optionally, six fp64 arrays [nq] as raw bits (two words each): the goal
 *  sampler's mean (joint midrange) and scale (0.1 x range), the joint limits, and the
 *  initial-joint bounds (range_fraction x limits).  With them env e draws from a
 *  numpy-compatible RandomState(seed + e) in the reference's order (goal normals with
 *  numpy's cached polar gaussians, then the uniform joint angles); without them, from a
 *  counter-based stream. */
#define DX_REACH_NPARAMS_HEAD 26
/* Handover params (float[44]): a two-hand scene (BASELINE config 5; the reference has no
 * bimanual task -- its pattern is Juggle's two hands and effectors, juggle.py:147-177,
 * arenas/arena.py:58-105), the cube handed from palm to palm behind the GoalTask surface.
 * 0-37 as reorient's, with hand_nq / hand_nv / fingertips counting both hands and the
 * bbox the giving (first) hand's spawn box; then 38-40 / 41-43 the target points above
 * the first / second hand's palm.  The goal is [target xyz, receiving hand]: at reset
 * the second hand's target; after steps_before_changing_goal successes it switches to
 * the other hand (the cube handed back).  Reward reorient.py:238-284's shape on the
 * cube-to-target distance d: w_orientation / (d + eps) + w_success [d <= threshold] +
 * w_action |ctrl|^2; the cube touching the ground ends the episode (discount 1). */
#define DX_HANDOVER_NPARAMS 44
enum dx_env_out { DX_OUT_OBS = 0, DX_OUT_REWARD = 1, DX_OUT_DISCOUNT = 2, DX_OUT_STEP_TYPE = 3,
                  DX_OUT_GOAL = 4, DX_OUT_SUCCESSES = 5, DX_OUT_GOAL_FAILURES = 6,
                  DX_OUT_GOAL_QPOS = 7 /* reach: [nenv][nq] f32, FingertipCartesianPosition.qpos
                                          (fingertip_position.py:136-139) */,
                  DX_OUT_PREV_ACTION = 8 /* [nenv][nu] f32, PreviousAction.previous_action; once the
                                            action pipeline has been configured (below) */,
                  DX_OUT_HAND_OBS = 9 /* [nenv][dx_env_hand_obs_dim] f32, the optional hand
                                         observables; while they are on (below) */,
                  DX_OUT_OBS_BUFFER = 10 /* [nenv][K][W] f32 oldest first, or [nenv][W] with an
                                            aggregator: the observation pipeline's delivered rows;
                                            while it is on (below) */,
                  DX_OUT_CONTACT_FORCE = 11 /* [nenv][3 * npad] f32, the contact forces of the task's
                                               pads; while they are on (below) */,
                  DX_OUT_PERTURB = 12 /* [nenv][nb][6] f32, the random pushes' wrenches (force,
                                         torque) on the nb configured bodies; while they are on
                                         (below) */,
                  DX_OUT_DEPTH = 13 /* [nenv][ncam][H][W] f32, the cameras' depth images; while
                                       cameras with DX_RENDER_DEPTH are on (dx_env_set_cameras) */,
                  DX_OUT_SEGMENTATION = 14 /* [nenv][ncam][H][W] int32, the geom id each pixel sees
                                              (-1: none); while cameras with DX_RENDER_SEGMENTATION
                                              are on */,
                  DX_OUT_RGB = 15 /* [nenv][ncam][H][W][3] uint8, the shaded images; while cameras
                                     with DX_RENDER_RGB are on */ };
dx_env* dx_env_create(const dx_model* m, int32_t nenv, int32_t device, int32_t task, uint64_t seed,
                      const float* params, int32_t nparams);
/* One shard of a job's environments: this handle's env e is the job's env env0 + e.
 * Every per-env stream is keyed by the job-wide index (numpy-compatible MT19937 seeded
 * with seed + env0 + e, dx_env_sample_actions keyed by env0 + e), so shard r of a
 * sharded job behaves exactly like envs [env0, env0 + nenv) of one unsharded batch --
 * the reference's one-RandomState-per-env seed contract (manipulation/__init__.py:56-86)
 * with env i seeded seed + i.  dx_env_create(...) = dx_env_create_shard(..., 0, ...). */
dx_env* dx_env_create_shard(const dx_model* m, int32_t nenv, int32_t device, int32_t task, uint64_t seed,
                            int64_t env0, const float* params, int32_t nparams);
void dx_env_destroy(dx_env* e);
dx_batch* dx_env_batch(dx_env* e);
int dx_env_obs_dim(const dx_env* e);
/* Goal width: 4 (reorient quaternion) or 3 * n fingertips (reach positions). */
int dx_env_goal_dim(const dx_env* e);
/* Re-initialises every env (initialize_episode) and computes FIRST observations. */
int dx_env_reset(dx_env* e);
/* One control step for every env; action is [nenv][nu] float32, device memory.  The
 * reorient task's before_step / after_step / reward / observation run inside the step
 * kernel: a control step is the step kernel, the mid contact tier beside it (a side
 * stream) and the overflow tier's launch after it, which also orders the next launch. */
int dx_env_step(dx_env* e, const float* action);
/* composer.Environment's time_limit (manipulation/__init__.py:61,83): an episode also
 * ends (LAST, with the task's discount) once its physics time reaches `seconds`.
 * Default: none (task.time_limit = inf). */
int dx_env_set_time_limit(dx_env* e, double seconds);
/* max_time_per_goal (task.py:120-135, 180-183) in fp64; default: the float in the task
 * params.  Both limits compare against the env's time accumulated in fp64 as MuJoCo
 * accumulates d->time (one += timestep per physics step), so a limit on a control-step
 * boundary ends the episode at the same step as the reference. */
int dx_env_set_goal_time_limit(dx_env* e, double seconds);
/* Device pointers of the outputs: obs [nenv][obs_dim] f32, reward/discount [nenv] f32,
 * step_type [nenv] i32 (0 FIRST, 1 MID, 2 LAST), goal [nenv][goal_dim] f32, successes i32,
 * goal failures i32 (the GoalInitializationErrors the reference would have raised: goal
 * draws that exhausted max_rejection_samples, fingertip_position.py:112-117; like
 * GoalEnvironment, environment.py:14-34, the env retries -- the step's goal draw, or the
 * whole reset -- from its continuing RandomState, up to 64 times per goal). */
int dx_env_output(dx_env* e, int which, void** devptr);
/* Library-owned [nenv][nu] device action buffer, and a fill of it with actions
 * drawn uniformly within each actuator's ctrlrange (the random agent of
 * manipulation_test.py:44-45), keyed by (seed, env, step). */
int dx_env_action_buffer(dx_env* e, void** devptr);
int dx_env_sample_actions(dx_env* e, uint64_t seed, int32_t step);
/* dx_env_step with the actions dx_env_sample_actions(e, seed, step) would draw, drawn
 * inside the step kernel (no action buffer, no extra launch): the random agent of the
 * reference's environment tests and of the benchmark. */
int dx_env_step_random(dx_env* e, uint64_t seed, int32_t step);

/* The action pipeline: the reference's three action-side wrappers on the device, one small
 * kernel ahead of every control step (dx_env_step, dx_env_step_host, dx_env_step_random;
 * the step then reads a library-owned filtered buffer, never the caller's).  Per env, in
 * the order the reference nests them:
 *  DX_ACT_NOISE     ActionNoise (manipulation/wrappers/action_noise.py): x = clip(a +
 *    normal(scale = noise_scale * (max - min)), min, max) over the action spec's bounds,
 *    the stddev in float32 as numpy computes it, the sum and the clip in fp64.  Drawn on
 *    every step, also the one that re-initialises the env.  Env e draws from a stream of
 *    its own, a numpy-compatible RandomState(noise_seed + env0 + e): replayable from numpy,
 *    a shard equals the unsharded batch, and no other stream or checkpoint field moves (the
 *    reference's wrapper shares the environment's RandomState: a stated deviation).
 *  DX_ACT_PREVIOUS  PreviousAction (effectors/wrappers/previous_action.py), DX_OUT_PREV_ACTION:
 *    the command of the last step, after the noise and before the smoothing; zeros at
 *    initialize_episode (dx_env_reset, and the step that returns FIRST).  Kept whenever
 *    the pipeline is on.
 *  DX_ACT_SMOOTH    SmoothAction (effectors/wrappers/smooth_action.py): ctrl = alpha * held +
 *    (1 - alpha) * x in fp64, restarted at initialize_episode (the first command of an
 *    episode passes unchanged).
 * dx_env_set_action_filter may be called between steps (it synchronises the stream);
 * NULL or flags 0 switches the pipeline off, and the step's launches, the outputs and the
 * checkpoint are then those of an env never configured.  DX_ACT_NOISE seeds (re-seeds) the
 * noise stream.  DX_EINVAL: smooth_alpha outside [0, 1] or not finite, noise_scale negative
 * or not finite, noise with an actuator that is not ctrllimited (an infinite stddev);
 * DX_ELIMIT: more than 64 actuators.  dx_env_reset draws nothing.
 * While the pipeline is on, the checkpoint (dx_env_save) carries its state after the
 * other fields -- act_ema, act_ema_set (int32), prev_action, mt_noise -- but not this
 * configuration: load a checkpoint into an env configured the same way. */
enum { DX_ACT_NOISE = 1, DX_ACT_SMOOTH = 2, DX_ACT_PREVIOUS = 4 };
typedef struct dx_action_filter {
  int32_t flags;
  float noise_scale;
  double smooth_alpha;
  uint64_t noise_seed;
} dx_action_filter;
int dx_env_set_action_filter(dx_env* e, const dx_action_filter* f);
/* Test hook: the next n (1..64) standard normals of every env's noise stream, consumed;
 * out_host [nenv][n] f64.  DX_ACT_NOISE must be on. */
int dx_env_action_noise_draw(dx_env* e, int32_t n, double* out_host);

/* The optional hand observables: those of the reference's hand entity
 * (models/hands/dexterous_hand.py:245-372) that the fixed observation does not carry, as
 * one small gather kernel behind every call that produces DX_OUT_OBS (dx_env_reset,
 * dx_env_step, dx_env_step_random, dx_env_step_host); its values describe the same state
 * as that observation, also on the FIRST step of an auto-reset env.  Per hand, in the
 * reference's declaration order (hand_nq joints and ntips fingertips PER HAND):
 *  DX_HOBS_JOINT_POSITIONS         hand_nq    qpos at the hand's joints (bit-equal to DX_QPOS)
 *  DX_HOBS_TIP_ORIENTATIONS        4 ntips    unit quaternion (w, x, y, z) of each fingertip
 *    site's xmat, canonical with w >= 0 ([3P] dm_robotics mat_to_quat's sign): normalised
 *    xquat[site_bodyid] (x) site_quat, negated when w < 0
 *  DX_HOBS_TIP_ANGULAR_VELOCITIES  3 ntips    world-frame angular velocity at each fingertip
 *    site (mj_objectVelocity, utils/mujoco_utils.py:10-35; bit-equal to DX_SITE_VEL words 3-5)
 *  DX_HOBS_TIP_POSITIONS_EGO       3 ntips    each fingertip site in the hand's root body's
 *    INERTIAL frame ([3P] framepos with reftype="body"): ximat^T (site_xpos - xipos)
 * DX_OUT_HAND_OBS is a library-owned [nenv][dx_env_hand_obs_dim] f32 buffer: hands in the
 * task's order (handover: left, then right; nhands = 2, else 1), within a hand the
 * enabled observables in the order above.  An element's value does not depend on the
 * mask.  The fingertip sites are the task's (the ones `fingertip_positions` uses).
 * dx_env_set_hand_observables may be called between steps (it synchronises the stream)
 * and, with a non-zero mask, leaves the buffer holding the env's current state: enabling
 * mid-episode equals enabling before dx_env_reset.  While orientations or ego positions
 * are on, the env's batch writes body poses (dx_set_outputs(batch, 1); the setting from
 * before is restored when the feature goes off).  NULL or mask 0 switches the feature off
 * (the default): a control step then launches what it launched before, and
 * dx_env_output(DX_OUT_HAND_OBS) fails.  DX_EINVAL (configuration unchanged): an unknown
 * bit, a root body outside [0, nbody), nhands other than the task's.  While the feature
 * is on, the checkpoint carries the buffer as its last field, hand_obs, but not this
 * configuration.  DX_OUT_OBS, dx_env_obs_dim and the packed rows are never affected.
 * joint_torques stays at the physics level (DX_SENSOR_TORQUE): a freshly reset env is only
 * observed, so the env step has no solved forces for it. */
enum { DX_HOBS_JOINT_POSITIONS = 1, DX_HOBS_TIP_ORIENTATIONS = 2, DX_HOBS_TIP_ANGULAR_VELOCITIES = 4,
       DX_HOBS_TIP_POSITIONS_EGO = 8 };
typedef struct dx_hand_obs {
  int32_t mask;          /* DX_HOBS_* */
  int32_t nhands;        /* the task's hand count */
  int32_t root_body[2];  /* one root body id per hand (the reference's hand.root_body) */
} dx_hand_obs;
int dx_env_set_hand_observables(dx_env* e, const dx_hand_obs* cfg);
/* Row width of DX_OUT_HAND_OBS; 0 while the feature is off. */
int dx_env_hand_obs_dim(const dx_env* e);

/* The contact forces between the hands and the prop (DX_PAD_FORCE at the env level): the
 * pads are fixed by the task -- per hand, in body order, every hand body that has a
 * collision pair with a geom of the task's prop body (params word 23), the prop their
 * partner: 23 for the Shadow reorient scene, 2 x 23 for the handover.  DX_OUT_CONTACT_FORCE is
 * a library-owned [nenv][3 * npad] f32 buffer, each pad's force in its body's frame, written
 * by one small kernel behind every control step (and dx_env_reset).
 *  - MID and LAST rows are those of the step's last physics step (the torque sensors' timing).
 *  - Rows are zero after dx_env_reset and for every env whose step returned FIRST: such an
 *    env ran no physics step, and a freshly spawned prop touches nothing.
 *  - Enabling between steps is allowed (it synchronises the stream) and leaves zeros until
 *    the next step.
 * Off is the default: the launches, every output and the checkpoint are then those of an env
 * never configured, and dx_env_output(DX_OUT_CONTACT_FORCE) fails.  While on, the checkpoint
 * carries the buffer as its last field, contact_force, but not the setting.  DX_OUT_OBS, the
 * packed rows, dx_env_step_host, the all-gather and the observation pipeline's row are
 * unaffected.  The reach tasks return DX_EINVAL: they have no prop, and Adroit's pairs have a
 * margin, so a collision-free reset state can carry force that no forward pass solves.
 * dx_env_contact_force_dim: 3 * npad while on, else 0.  dx_env_contact_force_bodies: the pads'
 * body ids into out[0 .. min(n, npad)), returns npad (on or off). */
int dx_env_set_contact_forces(dx_env* e, int enable);
int dx_env_contact_force_dim(const dx_env* e);
int dx_env_contact_force_bodies(const dx_env* e, int32_t* out, int32_t n);

/* Random pushes: the third part of the robustness kit beside the action noise and the
 * observation pipeline -- random wrenches on the prop (or up to four bodies), on the device:
 * one small kernel ahead of every control step (dx_env_step, dx_env_step_host,
 * dx_env_step_random), beside the action filter's, that writes the env's own xfrc_applied
 * rows.  While the feature is on the env's batch runs in per-env xfrc mode (above).
 * Env e owns a numpy-compatible RandomState(seed + env0 + e) of its own, keyed by the
 * job-wide env index: replayable from numpy, a shard equals the unsharded batch, no other
 * stream moves.  Per (env, configured body) the state is `remain` (int32) and `wrench`
 * (fp32 [6]: force, torque; world frame at the body's com, xfrc_applied's convention).
 * Per control step, for each configured body in order, exactly seven random_sample
 * doubles are drawn -- u_gate, u_fmag, u_fz, u_fphi, u_tmag, u_tz, u_tphi -- whichever
 * rule then applies.  Draws that go unused are intended: a step's consumption is fixed, so
 * a replay is one random_sample(7 * nb) per step.  The first rule that matches:
 *  - the step re-initialises the env (it returns FIRST): remain = 0, wrench = 0;
 *  - remain > 0: remain -= 1, the wrench is kept;
 *  - else wrench = 0, and if u_gate < probability: remain = duration - 1 and
 *      force  = (force_min + (force_max - force_min) u_fmag) * dir(u_fz, u_fphi),
 *      torque = (torque_min + (torque_max - torque_min) u_tmag) * dir(u_tz, u_tphi),
 *      dir(u_z, u_phi) = (s cos phi, s sin phi, z), z = 2 u_z - 1, s = sqrt(1 - z z),
 *      phi = 2 pi u_phi (uniform on the sphere); fp64 without contraction, each component
 *      magnitude * direction rounded to fp32 once.
 * A push therefore lasts exactly `duration` control steps (every physics step of them), and
 * a new one can start on the step after one ends.  The kernel writes xfrc[e][body] =
 * base[body] + wrench, one fp32 add per component, base being the batch's shared array (the
 * gravity compensation; dx_set_xfrc on the env's batch while the feature is on replaces the
 * base), and DX_OUT_PERTURB [nenv][nb][6], a library-owned buffer holding the wrench.
 * dx_env_reset clears the state (zero wrenches, rows = base) and draws nothing.
 * dx_env_set_perturbation may be called between steps (it synchronises the stream); an
 * accepted call seeds the streams and clears the state.  NULL or nbody == 0 switches the
 * feature off (the default): the batch returns to shared mode, and the step's launches,
 * every output and the checkpoint are those of an env never configured;
 * dx_env_output(DX_OUT_PERTURB) fails.  While on, the checkpoint carries the state after the
 * other optional fields -- perturb_remain (int32), perturb_wrench, mt_perturb -- but not
 * this configuration: load into an env configured the same way.
 * A rejected call changes nothing.  DX_EINVAL: a body id outside [1, nbody) (the world body
 * cannot be pushed) or repeated; probability outside [0, 1]; a negative or non-finite range
 * or min > max; duration < 1; a batch already put in per-env xfrc mode by the caller; the
 * reach tasks (their goal rollouts step the physics inside the reset, so a push would
 * change the goal sampling).  DX_ELIMIT: more than 4 bodies. */
typedef struct dx_perturbation {
  int32_t nbody;          /* 1..4 configured bodies; 0: off */
  int32_t bodies[4];      /* body ids, never the world body (0) */
  double probability;     /* of a new push per control step and body, while none is held */
  double force_min, force_max;    /* N */
  double torque_min, torque_max;  /* N m */
  int32_t duration;       /* control steps, >= 1 */
  uint64_t seed;
} dx_perturbation;
int dx_env_set_perturbation(dx_env* e, const dx_perturbation* p);
/* Test hook: the next n (1..64) random_sample doubles of every env's push stream, consumed;
 * out_host [nenv][n] f64.  The feature must be on. */
int dx_env_perturb_draw(dx_env* e, int32_t n, double* out_host);

/* The observation pipeline: the options the reference gives every observable
 * (ObservableSpec, manipulation/shared/observations.py:8-17, handed on by make_options
 * :114-120) -- update_interval, buffer_size, delay, aggregator, corruptor -- as composer's
 * observation updater applies them ([3P] dm_control composer observation updater / buffer),
 * on the device: one small kernel behind every call that produces DX_OUT_OBS (dx_env_reset,
 * dx_env_step, dx_env_step_random, dx_env_step_host), behind the hand observables' gather.
 * The row it works on is DX_OUT_OBS followed, while the hand observables are on, by
 * DX_OUT_HAND_OBS: W = dx_env_obs_dim + dx_env_hand_obs_dim floats.  One option set applies
 * to the whole row; noise_sigma is per element.
 * All times are CONTROL steps (composer counts physics steps: divide by n_sub_steps; only
 * multiples can be expressed, dexterity_amd.manipulation.obs_pipeline_options does it).
 * Per env, with n = control steps since the episode's FIRST observation (FIRST: n = 0),
 * m = update_interval, d = delay, K = buffer_size:
 *  - sample s_j is taken when n == j m; s_0 is the FIRST observation (the updater's reset
 *    inserts at time 0); it arrives at j m + d;
 *  - the corruptor runs once per sample and the buffer keeps the corrupted value:
 *    float32(double(o_i) + noise_sigma[i] * g_i), the product and the sum in fp64 without
 *    contraction, g the next W standard normals, in element order, of the env's own
 *    numpy-compatible RandomState(noise_seed + env0 + e) (legacy polar gaussians; the cached
 *    second value carries from sample to sample; a zero sigma still consumes its draw; a step
 *    that takes no sample draws nothing).  The stream of its own is the stated deviation of
 *    the action noise above, for the same reasons;
 *  - the read at n: J = floor((n - d) / m) for n >= d, else -1; delivered slot k (0 oldest,
 *    K-1 newest) is s_{J - (K-1-k)}; a negative index is padding -- zeros (DX_OBS_PAD_ZERO,
 *    composer's default) or s_0 (DX_OBS_PAD_INITIAL), also while s_0 has not arrived;
 *  - the aggregator, over the K delivered slots, padding included, in fp64 (the reference's
 *    rows are float64) rounded to fp32 once: the sum in slot order, oldest first; mean = sum
 *    / K; the median of an even K is (a + b) * 0.5;
 *  - dx_env_reset and the step that returns FIRST for an auto-reset env restart the env's
 *    history (n = 0, s_0 from that FIRST observation); LAST is an ordinary step.
 * DX_OUT_OBS_BUFFER is a library-owned buffer, [nenv][K][W] oldest first or [nenv][W] with
 * an aggregator.  Nothing else changes: DX_OUT_OBS, reward, discount, step type, goal, the
 * packed rows, dx_env_step_host's row and the all-gather keep their values and widths; the
 * pipeline never feeds back.
 * dx_env_set_obs_pipeline may be called between steps (it synchronises the stream).  NULL
 * switches the pipeline off (the default): a control step's launches, every output and the
 * checkpoint are then those of an env never configured, and dx_env_output(DX_OUT_OBS_BUFFER)
 * fails.  Switching it on, or reconfiguring it, starts every env's history afresh: n = 0,
 * s_0 = the env's current row, DX_OUT_OBS_BUFFER left holding that read, the noise streams
 * seeded again.  A rejected call leaves the configuration and the buffer as they were.
 * While the pipeline is on dx_env_set_hand_observables fails (DX_EINVAL): the mask sets W;
 * switch the pipeline off, change the mask, configure the pipeline again.
 * DX_EINVAL: a field outside its range, an unknown enum, noise other than 0 / 1, noise with
 * nsigma != W or a null, negative or non-finite sigma.  DX_ELIMIT: more than 80 ring slots
 * S = K + ceil(d / m) (the field ranges already keep S <= 80), or a row above 512 floats.
 * While the pipeline is on the checkpoint carries its state after the other fields --
 * obs_ring, obs_count (int32), mt_obs_noise (with numpy's has_gauss / gauss; while noise is
 * on), obs_buffer -- but not this configuration: load into an env configured the same way. */
enum { DX_OBS_PAD_ZERO = 0, DX_OBS_PAD_INITIAL = 1 };
enum { DX_OBS_AGG_NONE = 0, DX_OBS_AGG_MIN, DX_OBS_AGG_MAX, DX_OBS_AGG_MEAN, DX_OBS_AGG_MEDIAN, DX_OBS_AGG_SUM };
typedef struct dx_obs_pipeline {
  int32_t update_interval;   /* m, control steps, 1..64 */
  int32_t delay;             /* d, control steps, 0..64 */
  int32_t buffer_size;       /* K, 1..16 */
  int32_t aggregator;        /* DX_OBS_AGG_* */
  int32_t padding;           /* DX_OBS_PAD_* */
  int32_t noise;             /* 0 / 1 */
  uint64_t noise_seed;
  const double* noise_sigma; /* host, [W] when noise, else ignored */
  int32_t nsigma;            /* must equal W when noise */
} dx_obs_pipeline;
int dx_env_set_obs_pipeline(dx_env* e, const dx_obs_pipeline* p);
/* out = { W of the current row, delivered rows per env (K; 1 with an aggregator; 0 while
 * off), 1 on / 0 off }. */
int dx_env_obs_pipe_dims(const dx_env* e, int32_t out[3]);
/* Test hook: the next n (1..64) standard normals of every env's observation-noise stream,
 * consumed; out_host [nenv][n] f64.  The pipeline must be on with noise. */
int dx_env_obs_noise_draw(dx_env* e, int32_t n, double* out_host);

/* Checkpoint / resume.  An env's state is the set of device arrays that carry from one
 * control step to the next (physics and task state, the numpy-compatible MT19937 streams,
 * the dispatch order).  dx_env_save(e, NULL, 0) returns the state's size in bytes;
 * dx_env_save copies it to dst (host or device memory), dx_env_load restores it into an
 * env of the same task, model and batch size: the run then continues bit for bit as the
 * saved one would have.  dx_env_state_field(e, i, ...) describes field i (name, byte
 * offset in the saved buffer, bytes; i < 0: the count) and returns the field count. */
int dx_env_save(dx_env* e, void* dst, size_t nbytes);
int dx_env_load(dx_env* e, const void* src, size_t nbytes);
int dx_env_state_field(dx_env* e, int32_t i, const char** name, size_t* offset, size_t* nbytes);

/* Packs [obs | reward | discount | step_type] per env into dst ([nenv][obs_dim+3]
 * f32, device memory) on the env's stream: the shard an RCCL all-gather collates. */
int dx_env_pack_outputs(dx_env* e, float* dst_dev);
/* The reference's call shape, GoalEnvironment.step(action) -> TimeStep
 * (environment.py:25-34, task.py:63-73): action_host [nenv][nu] f32 and out_host
 * [nenv][obs_dim+3] f32 ([obs | reward | discount | step_type as float]) are host memory
 * (page-locked for asynchronous DMA); upload, control step, pack and download run on the
 * env's stream, and the call returns once out_host holds the TimeStep. */
int dx_env_step_host(dx_env* e, const float* action_host, float* out_host);

/* Multi-GPU observation collation over RCCL -------- */
/* The reference runs one environment per process and has no collective; here each
 * process (one per GPU) owns a dx_env shard of the job's environments and the only
 * exchange is one all-gather of the packed outputs per control step, over xGMI.
 * Bootstrap: rank 0 calls dx_comm_unique_id and hands the DX_COMM_ID_BYTES bytes to
 * every rank (file, env var, socket: the caller's choice) before dx_comm_init. */
typedef struct dx_comm dx_comm;
#define DX_COMM_ID_BYTES 128
int dx_comm_unique_id(void* id /* DX_COMM_ID_BYTES */);
/* Collective over nranks processes (ncclCommInitRank); device = this rank's GPU. */
dx_comm* dx_comm_init(const void* id, int32_t nranks, int32_t rank, int32_t device);
void dx_comm_destroy(dx_comm* c);
int dx_comm_rank(const dx_comm* c);
int dx_comm_size(const dx_comm* c);
/* All-gather of every rank's packed [obs | reward | discount | step_type] rows into
 * dst ([nranks * nenv][obs_dim + 3] f32, device memory on this rank's GPU): rank r's
 * environments land at rows [r * nenv, (r + 1) * nenv).  Enqueued on the env's stream
 * after its step (no host synchronisation); every rank must pass an env with the same
 * nenv and obs_dim. */
int dx_allgather_obs(dx_env* e, dx_comm* c, float* dst_dev);
/* Blocking max over ranks of a host scalar (also a barrier): the bench's job time. */
int dx_comm_allreduce_max(dx_comm* c, double* value);
int dx_comm_barrier(dx_comm* c);

/* Kinematic queries and batched inverse kinematics ---------------------- */
/* mj_jacSite (utils/mujoco_utils.py:67-73, compute_object_6d_jacobian) for every env
 * at its current qpos (kinematics + com positions are recomputed first; the batch's
 * state is not modified).  jacp / jacr: [nenv][nsite][3][nv] f32, host or device
 * memory; either may be null. */
int dx_jac_site(dx_batch* b, const int32_t* sites, int32_t nsite, float* jacp, float* jacr);

/* IKSolver.solve (inverse_kinematics/ik_solver.py:71-167) for every env of a batch.
 * Each attempt integrates damped-least-squares joint velocities
 * (controllers/dls/dls.py:43-77: (J^T J + reg I) qdot = J^T twist, twist = gain *
 * (target - site) / 1 s) with mj_integratePos over dt = 1 s, clips the solved
 * joints to their range, and re-runs kinematics, for at most max_steps steps
 * (ik_solver.py:169-236; early stop when every site is within linear_tol, abort
 * when error / progress > progress_threshold for any site).  Attempt 0 starts the
 * solved joints at their midrange, attempt a > 0 at numpy's a-th
 * np.random.uniform(*range.T) over the passed joints (ik_solver.py:127-130), env e
 * replaying a global stream seeded np.random.seed(seed + e) bit for bit; the other
 * qpos entries come from the batch.  The attempts run in parallel, one wavefront
 * each; the selection follows ik_solver.py:132-152: among attempts with every
 * error <= linear_tol, the first one (stop_on_first_successful_attempt) or the one
 * closest to the midrange (first on ties).  3 * nsite <= 32, njoint <= 64. */
typedef struct dx_ik_options {
  float linear_tol;          /* 1e-3  (ik_solver.py:73)                 */
  float regularization;      /* 1e-5  (_REGULARIZATION_WEIGHT, :24)     */
  float gain;                /* 0.95  (_LINEAR_VELOCITY_GAIN, :18)      */
  float progress_threshold;  /* 20    (_PROGRESS_THRESHOLD, :29)        */
  int32_t max_steps;         /* 100                                     */
  int32_t early_stop;        /* 0                                       */
  int32_t num_attempts;      /* 30                                      */
  int32_t stop_on_first;     /* 0 (stop_on_first_successful_attempt)    */
  uint64_t seed;
} dx_ik_options;
/* targets [nenv][nsite][3]; outputs (host or device memory, any may be null):
 * qpos_out [nenv][njoint] (the selected attempt's solved joints; when no attempt
 * succeeded -- the reference returns None -- the last attempt's), success [nenv]
 * (int32 0/1), linear_err [nenv][nsite] (of the returned joints), attempt [nenv]
 * (int32 index of the returned attempt), steps [nenv] (int32 integration steps it
 * took). */
int dx_ik_solve(dx_batch* b, const dx_ik_options* opt, const int32_t* sites, int32_t nsite,
                const int32_t* joints, int32_t njoint, const float* targets, float* qpos_out,
                int32_t* success, float* linear_err, int32_t* attempt, int32_t* steps);

/* Cartesian-to-joint velocity mapping ------------------------------------- */
/* The controlled objects of dx_jac_object / dx_dls_map: bodies, geoms and sites
 * (controllers/mapper.py:57-81), each a (type, id) pair.  A body is controlled at its
 * frame origin xpos (mj_jacBody), a geom at geom_xpos (mj_jacGeom), a site at site_xpos
 * (mj_jacSite).  3 * nobj <= 32 and nv <= 64, else DX_ELIMIT; an unknown type, an id out
 * of range or nobj < 1 is DX_EINVAL.  Every argument error returns before any launch.
 *
 * Host or device arguments: the work is enqueued on the batch's stream.  Each data array
 * (jacp, jacr, target_vel, qvel_out, status) that is device memory is read or written in
 * place by the kernel; one that is host memory is staged through device scratch.  A call
 * whose data arrays are all device memory returns without synchronising (dx_sync, or any
 * later call on the batch, orders after it); a call with a host array synchronises the
 * stream before it returns.  (dx_jac_site and dx_ik_solve stage every array and always
 * synchronise.)  types / ids are always host memory and are consumed before the return. */
enum dx_obj_type { DX_OBJ_BODY = 1, DX_OBJ_GEOM = 5, DX_OBJ_SITE = 6 };   /* MuJoCo's mjtObj values */
/* compute_object_6d_jacobian (utils/mujoco_utils.py:38-73) for bodies, geoms and sites of
 * every env at its current qpos (kinematics + com positions are recomputed first; the
 * batch's state is not modified): jacp / jacr [nenv][nobj][3][nv] f32, host or device
 * memory, either may be null.  For sites the values equal dx_jac_site's bit for bit. */
int dx_jac_object(dx_batch* b, const int32_t* types, const int32_t* ids, int32_t nobj,
                  float* jacp, float* jacr);
/* DampedLeastSquaresMapper.compute_joint_velocities (controllers/dls/dls.py:43-77) for
 * every env at its current qpos: with J [3 * nobj][nv] the stacked translational Jacobians
 * (the rotational halves are dropped, dls.py:62) and V = target_vel,
 *   qvel_out = J^T (J J^T + regularization I)^-1 V,
 * the solution of dls.py:69-74's (J^T J + regularization I) qdot = J^T V; with
 * regularization = 0 (dls.py:75-77, np.linalg.lstsq) the minimum-norm solution for a J of
 * full row rank.  A dof no object depends on gets exactly 0.
 * Rank guard (a deviation from lstsq, which would return a least-squares solution): when a
 * Cholesky pivot of J J^T + regularization I is <= eps_fp32 * max(3 * nobj, nv) * its
 * largest diagonal entry, the env's status is 1 and its qvel_out row is all zeros.
 * target_vel [nenv][nobj][3], qvel_out [nenv][nv], status [nenv] int32 (0 ok, 1
 * rank-deficient; may be null); host or device memory.  A negative or non-finite
 * regularization is DX_EINVAL.  The batch's state is not modified. */
int dx_dls_map(dx_batch* b, const int32_t* types, const int32_t* ids, int32_t nobj,
               float regularization, const float* target_vel, float* qvel_out, int32_t* status);

/* Depth and segmentation cameras, batched rays -------------------------- */
/* The reference's vision observables (manipulation/shared/observations.py:62-111, the 84 x 84
 * camera spec with its `depth` and `segmentation` switches; cameras.py:22-50) as a ray cast
 * against the geoms the compiled model holds -- the plane, boxes, spheres, capsules and
 * convex hulls -- in one launch behind the step (dx_render.hip).  Shaded RGB images come from
 * a second launch over the same cast (below: "Shaded RGB").
 *
 * Camera model ([3P] MuJoCo's pinhole).  The frame comes from xyaxes: x normalised, y made
 * orthogonal to x and normalised, z = x (x) y; the camera looks along -z.  fovy is the
 * vertical field of view in degrees.  Pixel (r, c), row 0 on top, has its centre at
 * (c + 0.5, r + 0.5); with f = 0.5 H / tan(fovy / 2) its ray is
 *   x (c + 0.5 - W/2) / f - y (r + 0.5 - H/2) / f - z,
 * not normalised, so the ray parameter of a hit is the depth along the optical axis in
 * metres (what dm_control's depth=True returns).  body = -1: pos / xyaxes are in the world;
 * body >= 0: in that body's frame, the camera rigidly attached (a palm camera).
 *
 * A pixel sees the nearest geom whose ENTRY depth lies in [near_, far_].  A hull is clipped
 * against its face planes, a box against its slabs, spheres and capsules in closed form; the
 * plane is infinite and one-sided (seen only from the side its normal faces).  Misses write
 * far_ to the depth and -1 to the segmentation; hits write the compiled model's geom id.
 * Stated deviations from an OpenGL render: a geom the near plane cuts (the camera inside
 * it, or its entry nearer than near_) is not seen at all, rather than showing its inside;
 * only compiled geoms exist -- the collision geoms, not the visual meshes and not the
 * reorient task's hint cube; and a hull is seen along a ray only where its chord is longer
 * than 8 ulp of the depth (about 5e-7 m at half a metre): the Shadow hand's meshes hold flat
 * pieces 6e-8 m thick, which fp32 would otherwise see or miss by rounding.  Such a piece is
 * therefore invisible also when it faces the camera: the pixel shows what lies behind it.
 *
 * Hull face planes are derived by the library on the host when cameras or rays are first
 * used (the assets carry vertices and adjacency, no faces): the plane through a vertex and
 * two neighbours that are neighbours of each other is a face when every vertex lies on one
 * side of it (tolerance 1e-9 max|v|); coplanar triangles are merged.  dx_model_hull_planes
 * (test hook, like dx_hull_support) copies the first min(n, count) planes of hull `mesh` to
 * out as (nx, ny, nz, d), unit n, n.x + d <= 0 inside, geom frame, and returns the count.
 *
 * dx_render_set_cameras: flags selects the outputs (at least one of DX_RENDER_DEPTH,
 * DX_RENDER_SEGMENTATION, DX_RENDER_RGB); DX_RENDER_NO_CULL renders without the per-tile geom cull and
 * gives bit-identical images (a test and measurement switch).  ncam = 0 switches the
 * feature off and frees nothing a later call would need.  While cameras are on the batch
 * writes body poses (dx_set_outputs(batch, 1); the earlier setting is restored when they
 * go off, and a dx_set_outputs call made while they are on does not switch the poses off:
 * it sets what is restored); on a batch that was stepping without them the poses are those
 * of the next dx_step / dx_forward.  It synchronises the stream.  DX_EINVAL (configuration unchanged):
 * a degenerate xyaxes, fovy outside (0, 180), near_ <= 0 or far_ <= near_, a body outside
 * [-1, nbody), no output flag; DX_ELIMIT: more than 8 cameras, a side above 512, or
 * nenv * ncam * height * width >= 2^31.
 * dx_render renders the batch's current poses (after dx_step or dx_forward) on its stream.
 * dx_render_output gives the device address of [nenv][ncam][height][width] f32
 * (which = DX_RENDER_DEPTH) or int32 (DX_RENDER_SEGMENTATION); dx_render_get copies envs
 * env0 .. env0+n-1 of one to host memory and synchronises.
 * Exact contracts: a pixel's value does not depend on the tile it falls in, on the other
 * cameras or on the cull; two renders of one state are bit-identical.
 * dx_render_stats (measurement): enable != 0 makes later renders count, per pixel tile,
 * the geoms that survive the cull; out (may be null) = {survivors summed, their maximum,
 * tiles} since the last call, which also clears them.  It synchronises the stream.
 *
 * dx_ray: nray rays per env, origin / dir [nenv][nray][3], dist [nenv][nray] f32, geom
 * [nenv][nray] int32, each in host or device memory as dx_dls_map accepts them.  dir is
 * normalised by the library and dist is along it: the nearest geom ENTERED at dist >= 0, a
 * miss gives -1 and geom -1 ([3P] mj_ray's return convention).  Unlike mj_ray, which can
 * report the far side of a geom the ray starts inside, a ray here never sees a geom it
 * starts inside; the camera rules above (one-sided plane, thin hulls) hold too.  It reads the poses the last dx_step / dx_forward wrote (body poses
 * must be on, the default of a dx_batch). */
typedef struct dx_camera {
  float pos[3];
  float xyaxes[6];
  float fovy;            /* degrees */
  float near_, far_;     /* metres along the optical axis */
  int32_t body;          /* -1: world-fixed */
} dx_camera;
enum { DX_RENDER_DEPTH = 1, DX_RENDER_SEGMENTATION = 2, DX_RENDER_NO_CULL = 4, DX_RENDER_RGB = 8 };
#define DX_RENDER_MAX_CAMERAS 8
#define DX_RENDER_MAX_SIDE 512
#define DX_RENDER_MAX_LIGHTS 4
#define DX_RENDER_MAX_FACE_GEOMS 8
int dx_model_hull_planes(const dx_model* m, int32_t mesh, float* out /* [n][4] or NULL */, int32_t n);
int dx_render_set_cameras(dx_batch* b, const dx_camera* cams, int32_t ncam, int32_t width, int32_t height,
                          int32_t flags);
int dx_render(dx_batch* b);
int dx_render_output(dx_batch* b, int which, void** devptr);
int dx_render_get(dx_batch* b, int which, void* dst_host, int32_t env0, int32_t n);
int dx_render_stats(dx_batch* b, int enable, uint64_t out[3]);
int dx_ray(dx_batch* b, const float* origin, const float* dir, int32_t nray, float* dist, int32_t* geom);
/* Env level: the cameras of a dx_env's batch, rendered behind every call that produces the
 * observation (dx_env_reset, dx_env_step, dx_env_step_random, dx_env_step_host), after its
 * last launch: DX_OUT_DEPTH / DX_OUT_SEGMENTATION / DX_OUT_RGB describe the same state as DX_OUT_OBS, and an
 * env that returned FIRST shows its reset state.  dx_env_set_cameras may be called between
 * steps and leaves the images holding the current state; ncam = 0 switches them off (the
 * default: a control step then launches what it launched before, and dx_env_output of the two
 * fails).  The images are not part of the packed row, dx_env_step_host's row, the all-gather,
 * the observation pipeline or the checkpoint: after dx_env_load they are stale until the next
 * step or reset. */
int dx_env_set_cameras(dx_env* e, const dx_camera* cams, int32_t ncam, int32_t width, int32_t height,
                       int32_t flags);

/* Shaded RGB -------------------------------------------------------------- */
/* DX_RENDER_RGB adds [nenv][ncam][height][width][3] uint8 images (dx_render_output /
 * dx_render_get with which = DX_RENDER_RGB; DX_OUT_RGB at the env level), shaded by a second
 * kernel behind the cast, which reads the cast's depth and geom id per pixel.  With
 * DX_RENDER_RGB alone the cast still runs, into buffers of the library's own: DX_RENDER_DEPTH
 * and DX_RENDER_SEGMENTATION then stay "not enabled".  The exact contracts of the cast hold
 * for the bytes too (cull, tiling, other cameras, two renders).
 *
 * The shading model (written down so that a numpy restatement pins it; it is not OpenGL's).
 * With O the camera origin, D the pixel's unnormalised direction and t the cast's depth,
 * P = O + t D is the hit point and p the same point in the hit geom's frame.
 *  Normal, from p alone: plane +z; sphere p/|p|; capsule q/|q| with q = p - clamp(p_z, -h, h) e_z;
 *   box: axis k = argmax_k (|p_k| - size_k), lowest k on a tie, n = sign(p_k) e_k, face
 *   f = 2k + (p_k < 0) (+x, -x, +y, -y, +z, -z); hull: the normal of the face plane with the
 *   largest n_i.p + d_i (dx_model_hull_planes' planes, lowest index on a tie): flat per facet.
 *   The geom's pose turns it to the world.
 *  Lights (at most DX_RENDER_MAX_LIGHTS): l = -dir/|dir| for a directional light, else
 *   (pos - P)/|pos - P|.  The optional headlight has l = the camera's +z axis for every pixel
 *   and casts no shadow.
 *  Shadows: a light with castshadow does not reach a pixel with n.l > 0 when the line
 *   P + tau l enters a geom other than the hit one at 0 < tau < tau_max (infinity for a
 *   directional light, |pos - P| else); "enters" is the cast's own entry test, so an entry at
 *   tau <= 0 does not occlude and a hull thinner than the cast resolves casts no shadow.
 *   Every geom is convex and shadows itself exactly where n.l <= 0: no bias, no epsilon.
 *  Colour, linear (no gamma, no specular term):
 *   c = albedo * min(1, ambient + sum_l s_l diffuse_l max(0, n.l_l)), stored as
 *   floor(255 c + 0.5) clamped to 0..255; a miss stores `background`.
 *  Albedo: geom_rgb[g]; for a box registered in face_geom, face_rgb[slot][f]; for a plane geom
 *   with checker_cell > 0, checker_rgb[(floor(p_x / cell) + floor(p_y / cell)) & 1].
 * No alpha, textures, materials, highlights, reflectance, skybox or visual meshes.
 *
 * dx_render_set_shading: the settings persist across dx_render_set_cameras and may be given
 * before or after it; without a call the defaults hold.  geom_rgb NULL: the default palette --
 * the world's geoms (0.45, 0.45, 0.5), the geoms of each hand (a tree whose root has no free
 * joint, in root order) (0.85, 0.65, 0.5) or (0.5, 0.65, 0.85) in turn, a free-jointed prop's
 * (0.8, 0.8, 0.8) -- and, when face_geom is NULL too, the first box geom of a free-jointed body
 * with the six face colours red, green, blue, yellow, magenta, cyan (dexterity_amd/cameras.py
 * holds the values).  face_geom non-NULL with nface = 0: no face colours.  lights NULL: the
 * reference arena's light, directional, straight down (dir (0, 0, -1)), diffuse 0.5,
 * castshadow; lights non-NULL with nlight = 0: no lights.  shading NULL: ambient 0.2,
 * background 0, headlight 0.3 ([3P] MuJoCo's default headlight is on), no checker.  DX_EINVAL: a face_geom that is no box geom or is repeated, a
 * non-finite value, a negative checker_cell, a zero dir on a directional light, a null array
 * with a positive count; DX_ELIMIT: more than DX_RENDER_MAX_LIGHTS lights or
 * DX_RENDER_MAX_FACE_GEOMS face geoms.  It synchronises the stream; a refused call changes nothing.
 * dx_render_stats2 (measurement): as dx_render_stats, for the shadow pass's cull (geoms that
 * survive per pixel tile and shadow-casting light); one switch serves both. */
typedef struct dx_light {
  float pos[3], dir[3], diffuse[3];
  int32_t directional, castshadow;
} dx_light;
typedef struct dx_shading {
  float ambient[3], background[3];
  float headlight[3];      /* diffuse; all 0 = off */
  float checker_rgb[2][3];
  float checker_cell;      /* metres; 0 = off */
} dx_shading;
int dx_render_set_shading(dx_batch* b, const float* geom_rgb /* [ngeom][3] or NULL */, const int32_t* face_geom,
                          const float* face_rgb /* [nface][6][3] */, int32_t nface, const dx_light* lights,
                          int32_t nlight, const dx_shading* shading /* or NULL */);
int dx_env_set_shading(dx_env* e, const float* geom_rgb, const int32_t* face_geom, const float* face_rgb,
                       int32_t nface, const dx_light* lights, int32_t nlight, const dx_shading* shading);
int dx_render_stats2(dx_batch* b, uint64_t out[3]);

/* Timing ---------------------------------------------------------------- */
/* When enabled, HIP events bracket the step-kernel launches on the batch stream -- every
 * launch (enable = 1) or every enable-th one (enable > 1: the events' own packets cost
 * ~5 us per bracketed launch); dx_timing_read syncs, returns the summed kernel time and
 * the count of bracketed launches, and clears. */
int dx_timing_enable(dx_batch* b, int enable);
int dx_timing_read(dx_batch* b, double* total_ms, int32_t* count);
/* Per-stage shader-clock accounting inside the fused step kernel (diagnostics):
 * out[k] = summed s_memtime cycles of stage k over all envs since the last read
 * (n < nenv * 40), or out[env * 40 + k] per env (n >= nenv * 40). */
int dx_stage_timing(dx_batch* b, int enable);
int dx_stage_read(dx_batch* b, uint64_t* out, int32_t n);
/* Test hook: overwrites the LDS of every CU on `device` with NaN patterns. */
int dx_debug_poison_lds(int32_t device);

const char* dx_last_error(void);
/* The hash of the sources the library was built from (dexterity_amd/build.py source_key):
 * the Python layer refuses an in-tree library whose sources have changed since. */
const char* dx_build_key(void);
int dx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
