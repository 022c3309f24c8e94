// dx_batch.hip -- the model's device copies and dx_batch: it owns the per-env state arrays
// ([nenv][width], fp32) and a HIP stream, and launches the step kernels.
#include "dx_host.h"

extern "C" __global__ void dx_reset_kernel(DevModel m, DevBatch B, int env0, int n);

extern "C" void dx_model_free(dx_model* m) {
  if (!m) return;
  for (auto& kv : m->dev_allocs) {
    int cur;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(kv.first);
    for (void* p : kv.second) (void)hipFree(p);
    (void)hipSetDevice(cur);
  }
  delete m;
}

// The plane table on `device`, uploaded once (freed with the model).
int render_tables(dx_model* m, int device, dx_model::RenderDev* out) {
  // (batches of one model on several devices may first use cameras from different threads)
  std::lock_guard<std::recursive_mutex> lock(g_render_mu);
  if (int rc = hull_planes(m)) return rc;
  auto it = m->render_dev.find(device);
  if (it != m->render_dev.end()) { *out = it->second; return 0; }
  std::vector<void*>& allocs = m->dev_allocs[device];
  auto up = [&](const void* src, size_t bytes, const void** dst) -> int {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
    allocs.push_back(p);
    if (bytes) HIPCHK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *dst = p;
    return 0;
  };
  dx_model::RenderDev r{};
  if (int rc = up(m->plane4.data(), m->plane4.size() * 4, (const void**)&r.plane4)) return rc;
  if (int rc = up(m->planeadr.data(), m->planeadr.size() * 4, (const void**)&r.planeadr)) return rc;
  if (int rc = up(m->planenum.data(), m->planenum.size() * 4, (const void**)&r.planenum)) return rc;
  m->render_dev[device] = r;
  *out = r;
  return 0;
}

// Upload the model to `device` once; returns the DevModel with device pointers.
static int device_model(dx_model* m, int device, DevModel* out) {
  auto it = m->dev_models.find(device);
  if (it != m->dev_models.end()) { *out = it->second; return 0; }
  DevModel d = m->dm;
  std::vector<void*>& allocs = m->dev_allocs[device];
  auto up = [&](const void* src, size_t words, const void** dst) -> int {  // (float and int tables alike)
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, std::max<size_t>(words, 1) * 4));
    allocs.push_back(p);
    if (words) HIPCHK(hipMemcpy(p, src, words * 4, hipMemcpyHostToDevice));
    *dst = p;
    return 0;
  };
#define UP(map, field) { auto& v_ = m->map[#field]; const void* p_; if (int rc = up(v_.data(), v_.size(), &p_)) return rc; d.field = (decltype(d.field))p_; }
#define UF(field) UP(hf, field)
#define UI(field) UP(hi, field)
  UI(body_parent); UI(body_rootidx); UI(body_jntnum); UI(body_jntadr); UI(body_dofnum); UI(body_dofadr);
  UI(lvl_adr); UI(lvl_body); UI(root_body);
  UF(body_pos); UF(body_quat); UF(body_ipos); UF(body_imat); UF(body_mass); UF(body_inertia);
  UF(body_bsphere); UF(body_invweight0);
  UI(jnt_type); UI(jnt_bodyid); UI(jnt_qposadr); UI(jnt_dofadr);
  UF(jnt_pos); UF(jnt_axis); UF(jnt_range); UF(jnt_margin); UF(jnt_solref); UF(jnt_solimp); UF(qpos0);
  UI(limj_jnt); UI(dof_bodyid); UI(dof_parentid); UI(dof_jntid); UI(fric_dof); UI(dof_fricrow);
  UF(dof_armature); UF(dof_damping); UF(dof_frictionloss); UF(dof_solref); UF(dof_solimp); UF(dof_invweight0);
  UI(geom_type); UI(geom_bodyid); UI(geom_dataid);
  UF(geom_size); UF(geom_pos); UF(geom_mat); UF(geom_center); UF(geom_bsphere); UF(geom_bsphere_b); UF(geom_obb_b);
  UI(mesh_vertadr); UI(mesh_vertnum); UF(mesh_vert4);
  UI(mesh_binn); UI(mesh_bincap); UI(mesh_binadr); UF(mesh_bin4);
  UF(geom_rec); UF(gpair_rec); UF(geom_crec); UF(bpair_rec); UF(bp_item); UI(bp_cull); UF(body_rec); UF(dof_rec); UI(ldl_tab);
  UI(site_bodyid); UF(site_pos); UF(site_mat);
  UI(tendon_adr); UI(tendon_num); UI(wrap_dof); UI(wrap_qadr); UI(limt_ten);
  UF(tendon_range); UF(tendon_margin); UF(tendon_solref); UF(tendon_solimp); UF(tendon_invweight0);
  UF(wrap_coef); UF(tendon_J);
  UI(actuator_trntype); UI(actuator_trnid); UI(actuator_biastype); UI(actuator_ctrllimited);
  UI(actuator_forcelimited);
  UF(actuator_gear); UF(actuator_gainprm); UF(actuator_biasprm); UF(actuator_ctrlrange); UF(actuator_forcerange);
  UI(bpair_body); UI(bpair_adr); UI(bpair_num); UI(bpair_plane); UF(bpair_sphere); UI(gpair_geom); UI(gpair_condim);
  UF(gpair_friction); UF(gpair_solref); UF(gpair_solimp); UF(gpair_margin);
#undef UF
#undef UI
#undef UP
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, m->body_chain.size() * 8));
  allocs.push_back(p);
  HIPCHK(hipMemcpy(p, m->body_chain.data(), m->body_chain.size() * 8, hipMemcpyHostToDevice));
  d.body_chain = (decltype(d.body_chain))p;
  // the struct itself, for the kernels that read the model through a pointer
  HIPCHK(hipMalloc(&p, sizeof(DevModel)));
  allocs.push_back(p);
  HIPCHK(hipMemcpy(p, &d, sizeof(DevModel), hipMemcpyHostToDevice));
  m->dev_model_ptrs[device] = (const DevModel*)p;
  m->dev_models[device] = d;
  *out = d;
  return 0;
}

// ---- batch ----
#define DX_HI_GRID 32  // workgroups of the overflow tier (each loops over the deferred steps)

int balloc(dx_batch* b, void** p, size_t bytes) {
  HIPCHK(hipMalloc(p, std::max<size_t>(bytes, 4)));
  HIPCHK(hipMemsetAsync(*p, 0, std::max<size_t>(bytes, 4), b->stream));
  b->allocs.push_back(*p);
  return 0;
}

// Sets b->slots, the chip's resident 64-lane workgroups of the step kernel the batch
// launches (the instrumented twin's with stage timing on), and returns the count per CU
// (LDS and VGPR limits; 8 when the runtime cannot say), with the occupancy experiment
// DX_LDS_PAD (extra LDS bytes).
static int step_slots(dx_batch* b) {
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, b->device) != hipSuccess || ncu < 1) ncu = 256;
  const char* pad = getenv("DX_LDS_PAD");
  const size_t lds = (size_t)b->model->lds.total * 4 + (pad ? (size_t)atol(pad) : 0);
  int per = dx_step_occupancy(b->spec, lds, b->db.stage_acc != nullptr);
  if (per < 1) per = (int)std::max<size_t>(1, std::min<size_t>(8, 163840 / lds));
  b->slots = ncu * per;
  return per;
}

extern "C" dx_batch* dx_batch_create(const dx_model* mc, int32_t nenv, int32_t device) {
  dx_model* m = const_cast<dx_model*>(mc);
  if (!m || nenv < 1) { dx_fail(DX_EINVAL, "bad model or nenv"); return nullptr; }
  if (nenv > (1 << DX_DEFER_ENV_BITS)) { dx_fail(DX_ELIMIT, "nenv above 2^20 per batch (deferral entries)"); return nullptr; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    dx_fail(DX_EHIP, "invalid HIP device (is a GPU visible?)");
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) { dx_fail(DX_EHIP, "hipSetDevice failed"); return nullptr; }
  dx_batch* b = new dx_batch();
  b->model = m;
  b->device = device;
  b->nenv = nenv;
  b->debug = false;
  b->xfrc = nullptr;
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
    dx_fail(DX_EHIP, "hipStreamCreate failed");
    delete b;
    return nullptr;
  }
  if (device_model(m, device, &b->dm) != 0) { delete b; return nullptr; }
  b->dm_dev = m->dev_model_ptrs[device];
  b->spec = getenv("DX_GENERIC_KERNEL") ? -1 : dx_spec_find(b->dm, m->lds);
  const DevModel& d = b->dm;
  DevBatch& B = b->db;
  memset(&B, 0, sizeof(B));
  B.nenv = nenv;
  size_t E = nenv;
  int rc = 0;
  rc |= balloc(b, (void**)&B.qpos, E * d.nq * 4);
  rc |= balloc(b, (void**)&B.qvel, E * d.nv * 4);
  rc |= balloc(b, (void**)&B.ctrl, E * std::max(d.nu, 1) * 4);
  rc |= balloc(b, (void**)&B.qacc_ws, E * d.nv * 4);
  rc |= balloc(b, (void**)&B.qacc, E * d.nv * 4);
  rc |= balloc(b, (void**)&B.time, E * 4);
  rc |= balloc(b, (void**)&B.site_xpos, E * 3 * std::max(d.nsite, 1) * 4);
  rc |= balloc(b, (void**)&B.site_vel, E * 6 * std::max(d.nsite, 1) * 4);
  rc |= balloc(b, (void**)&B.xpos, E * 3 * d.nbody * 4);
  rc |= balloc(b, (void**)&B.xquat, E * 4 * d.nbody * 4);
  rc |= balloc(b, (void**)&B.ncon, E * 4);
  rc |= balloc(b, (void**)&B.watch, E * 4);
  rc |= balloc(b, (void**)&B.niter, E * 4);
  rc |= balloc(b, (void**)&B.ncand, E * 4);
  if (!getenv("DX_NO_SEPCACHE"))  // (A/B and traffic attribution: MPR without the separating-direction cache)
    rc |= balloc(b, (void**)&B.sepcache, E * DX_SEP_SLOTS * 16);
  rc |= balloc(b, (void**)&B.health, DX_HEALTH_WORDS * 4);
  rc |= balloc(b, (void**)&B.bad, E * 4);
  rc |= balloc(b, (void**)&B.nstep, E * 4);
  // the overflow tier's deferral list (models that can have contacts)
  if (!d.disable_contact && d.ngpair > 0) rc |= balloc(b, (void**)&B.defer, (E + 2) * 4);
  if (!getenv("DX_NO_LPT_ORDER")) {
    void* po = nullptr;
    rc |= balloc(b, (void**)&B.cost, E * 4);
    rc |= balloc(b, &po, E * 4);
    B.order = (const int*)po;
    rc |= balloc(b, (void**)&B.ohist, 2 * 256 * 4);
    rc |= balloc(b, (void**)&B.okey, E * 4);
  }
  rc |= balloc(b, (void**)&b->xfrc, 6 * d.nbody * 4);
  // substep queue state (DX_NO_QUEUE=1: one workgroup per env for the whole step)
  b->queue = !getenv("DX_NO_QUEUE");
  rc |= balloc(b, (void**)&B.qhead, DX_QUEUES * DX_QHEAD_STRIDE * 4);
  rc |= balloc(b, (void**)&B.progress, E * 4);
  rc |= balloc(b, (void**)&B.qerr, 8);  // [0] queue timeout, [1] the overflow kernel's finished workgroups
  B.hand_stride = (d.nq + 2 * d.nv + 4 + 31) / 32 * 32;
  rc |= balloc(b, (void**)&B.hand, E * B.hand_stride * 4);
  B.epoch = 0;
  // one queue per XCD (DX_ONE_QUEUE=1: a single queue for the whole chip)
  B.nqueue = getenv("DX_ONE_QUEUE") ? 1 : DX_QUEUES;
  B.np_wide = getenv("DX_NP_WIDE") ? atoi(getenv("DX_NP_WIDE")) : DX_WAVE / 8;
  B.defer_at = getenv("DX_DEFER_AT") ? atoi(getenv("DX_DEFER_AT")) : DX_NCON_MAX;  // (tests / probes)
  B.order_last = getenv("DX_ORDER_LAST") ? atoi(getenv("DX_ORDER_LAST")) : 1;
  b->hi_grid = getenv("DX_HI_GRID") ? std::max(1, atoi(getenv("DX_HI_GRID"))) : DX_HI_GRID;
  {
    const int per = step_slots(b);
    // the mid tier: its workgroup fits a CU that holds one step-kernel workgroup fewer
    // (LDS in 512-B granules; its VGPRs fit the SIMD that then runs one wave)
    auto g512 = [](size_t x) { return (x + 511) / 512 * 512; };
    const char* pad = getenv("DX_LDS_PAD");
    const size_t lds = (size_t)m->lds.total * 4 + (pad ? (size_t)atol(pad) : 0);
    const size_t lmid = (size_t)m->lds_mid.total * 4;
    b->mid = b->queue && B.defer && m->lds_mid.nefc_max > 0 && !getenv("DX_NO_MID") && per >= 2 &&
             (size_t)(per - 1) * g512(lds) + g512(lmid) <= 163840;
  }
  if (b->mid) {
    rc |= balloc(b, (void**)&B.defer2, (E + 2) * 4);
    rc |= balloc(b, (void**)&B.qdone, 2 * 4);
    B.mid_defer_at = getenv("DX_MID_DEFER_AT") ? atoi(getenv("DX_MID_DEFER_AT")) : DX_NCON_MID;  // (tests)
    if (hipStreamCreateWithFlags(&b->side, hipStreamNonBlocking) != hipSuccess)
      rc |= dx_fail(DX_EHIP, "mid-tier stream creation failed");
  }
  if (rc) { dx_batch_destroy(b); return nullptr; }
  B.xfrc = nullptr;  // enabled by dx_set_xfrc
  if (B.order && dx_launch_order(nenv, b->stream, B.cost, (int*)B.order, nullptr) != hipSuccess) {  // a permutation
    dx_fail(DX_EHIP, "order kernel launch failed");
    dx_batch_destroy(b);
    return nullptr;
  }
  B.watch_geom = -1;
  B.watch_body = -1;
  B.out_bodies = 1;
  if (dx_reset(b, 0, nenv) != 0) { dx_batch_destroy(b); return nullptr; }
  // the mid tier's stream is ordered after nothing on the batch stream: its first launch
  // must not read the deferral list or the exit counts before their zeroing above
  if (b->mid && hipStreamSynchronize(b->stream) != hipSuccess) {
    dx_fail(DX_EHIP, "stream sync failed");
    dx_batch_destroy(b);
    return nullptr;
  }
  return b;
}

extern "C" void dx_batch_destroy(dx_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  (void)hipStreamSynchronize(b->stream);
  if (b->side) (void)hipStreamSynchronize(b->side);
  for (void* p : b->allocs) (void)hipFree(p);
  if (b->side) (void)hipStreamDestroy(b->side);
  (void)hipStreamDestroy(b->stream);
  delete b;
}

extern "C" int dx_batch_nenv(const dx_batch* b) { return b ? b->nenv : dx_fail(DX_EINVAL, "null batch"); }

extern "C" int dx_reset(dx_batch* b, int32_t env0, int32_t n) {
  if (!b || env0 < 0 || n < 0 || env0 + n > b->nenv) return dx_fail(DX_EINVAL, "bad env range");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(dx_reset_kernel, dim3(n), dim3(64), 0, b->stream, b->dm, b->db, env0, n);
  HIPCHK(hipGetLastError());
  return 0;
}

static void* field_base(dx_batch* b, int field) {
  DevBatch& B = b->db;
  switch (field) {
    case DX_QPOS: return B.qpos;
    case DX_QVEL: return B.qvel;
    case DX_CTRL: return B.ctrl;
    case DX_QACC_WARMSTART: return B.qacc_ws;
    case DX_QACC: return B.qacc;
    case DX_TIME: return B.time;
    case DX_SITE_XPOS: return B.site_xpos;
    case DX_SITE_VEL: return B.site_vel;
    case DX_XPOS: return B.xpos;
    case DX_XQUAT: return B.xquat;
    case DX_NCON: return B.ncon;
    case DX_GROUND_CONTACT: return B.watch;
    case DX_NITER: return B.niter;
    case DX_NCAND: return B.ncand;
    case DX_STEP_COST: return B.cost;
    case DX_SENSOR_TORQUE: return b->sensor;
    case DX_DIVERGED: return B.bad;
    case DX_CFRC_EXT: return b->cfrc_ext;
    case DX_PAD_FORCE: return b->pad_force;
  }
  return nullptr;
}

// A substep-queue launch that timed out waiting for a predecessor task aborts
// (dx_step.hip step_queue); the batch state is then unusable.  Checked at every
// host synchronisation point.
int queue_check(dx_batch* b) {
  if (!b->db.qerr) return 0;
  int err = 0;
  HIPCHK(hipMemcpy(&err, b->db.qerr, 4, hipMemcpyDeviceToHost));
  if (err) return dx_fail(DX_EHIP, "substep queue timed out waiting for a predecessor task (launch aborted)");
  return 0;
}

extern "C" int dx_field_ptr(dx_batch* b, int field, void** devptr) {
  if (!b || !devptr) return dx_fail(DX_EINVAL, "null argument");
  void* p = field_base(b, field);
  if (!p) return dx_fail(DX_EINVAL, "unknown field");
  *devptr = p;
  return 0;
}

extern "C" int dx_set_field(dx_batch* b, int field, const void* src, int32_t env0, int32_t n) {
  if (!b || !src) return dx_fail(DX_EINVAL, "null argument");
  if (env0 < 0 || n < 0 || env0 + n > b->nenv) return dx_fail(DX_EINVAL, "bad env range");
  if (field != DX_QPOS && field != DX_QVEL && field != DX_CTRL && field != DX_QACC_WARMSTART && field != DX_TIME)
    return dx_fail(DX_EINVAL, "field is read-only");
  int w = dx_field_width(b->model, field);
  if (w <= 0) return 0;
  char* base = (char*)field_base(b, field);
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(base + (size_t)env0 * w * 4, src, (size_t)n * w * 4, hipMemcpyDefault, b->stream));
  return 0;
}

extern "C" int dx_get_field(dx_batch* b, int field, void* dst, int32_t env0, int32_t n) {
  if (!b || !dst) return dx_fail(DX_EINVAL, "null argument");
  if (env0 < 0 || n < 0 || env0 + n > b->nenv) return dx_fail(DX_EINVAL, "bad env range");
  char* base = (char*)field_base(b, field);
  if (!base) return dx_fail(DX_EINVAL, "unknown field");
  int w = field == DX_PAD_FORCE ? 3 * b->npad : dx_field_width(b->model, field);
  if (w <= 0) return 0;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(dst, base + (size_t)env0 * w * 4, (size_t)n * w * 4, hipMemcpyDefault, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return queue_check(b);
}

extern "C" int dx_set_xfrc(dx_batch* b, const float* xfrc, int32_t nbody) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (!xfrc) {  // (the unused shared array is kept zero: what every env then reads back)
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemsetAsync(b->xfrc, 0, (size_t)b->dm.nbody * 6 * 4, b->stream));
    b->db.xfrc = nullptr;
    b->db.xfrc_stride = 0;
    return 0;
  }
  if (nbody != b->dm.nbody) return dx_fail(DX_EINVAL, "xfrc must be [nbody][6]");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(b->xfrc, xfrc, (size_t)nbody * 6 * 4, hipMemcpyDefault, b->stream));
  b->db.xfrc = b->xfrc;
  b->db.xfrc_stride = 0;
  return 0;
}

// Shared -> per-env mode: every env's rows start as the shared array (zero without one,
// dx_set_xfrc), by doubling copies on the stream.
int xfrc_env_mode(dx_batch* b) {
  if (b->db.xfrc_stride) return 0;
  const size_t row = (size_t)b->dm.nbody * 6 * 4;
  HIPCHK(hipSetDevice(b->device));
  if (!b->xfrc_env && balloc(b, (void**)&b->xfrc_env, (size_t)b->nenv * row)) return DX_EHIP;
  HIPCHK(hipMemcpyAsync(b->xfrc_env, b->xfrc, row, hipMemcpyDeviceToDevice, b->stream));
  for (size_t have = 1; have < (size_t)b->nenv; have *= 2) {
    const size_t n = std::min(have, (size_t)b->nenv - have);
    HIPCHK(hipMemcpyAsync((char*)b->xfrc_env + have * row, b->xfrc_env, n * row, hipMemcpyDeviceToDevice, b->stream));
  }
  b->db.xfrc = b->xfrc_env;
  b->db.xfrc_stride = 6 * b->dm.nbody;
  return 0;
}

extern "C" int dx_set_xfrc_env(dx_batch* b, const float* xfrc, int32_t env0, int32_t n) {
  if (!b || !xfrc) return dx_fail(DX_EINVAL, "null argument");
  if (env0 < 0 || n < 0 || env0 + n > b->nenv) return dx_fail(DX_EINVAL, "bad env range");
  if (int rc = xfrc_env_mode(b)) return rc;
  const size_t row = (size_t)b->dm.nbody * 6 * 4;
  if (n > 0) HIPCHK(hipMemcpyAsync((char*)b->xfrc_env + (size_t)env0 * row, xfrc, (size_t)n * row, hipMemcpyDefault, b->stream));
  return 0;
}

extern "C" int dx_get_xfrc_env(dx_batch* b, float* dst, int32_t env0, int32_t n) {
  if (!b || !dst) return dx_fail(DX_EINVAL, "null argument");
  if (env0 < 0 || n < 0 || env0 + n > b->nenv) return dx_fail(DX_EINVAL, "bad env range");
  const size_t row = (size_t)b->dm.nbody * 6 * 4;
  HIPCHK(hipSetDevice(b->device));
  if (b->db.xfrc_stride) {
    if (n > 0) HIPCHK(hipMemcpyAsync(dst, (char*)b->xfrc_env + (size_t)env0 * row, (size_t)n * row, hipMemcpyDefault, b->stream));
  } else {  // shared mode: every env reads the shared array (zeros without one)
    for (int k = 0; k < n; k++) HIPCHK(hipMemcpyAsync((char*)dst + k * row, b->xfrc, row, hipMemcpyDefault, b->stream));
  }
  HIPCHK(hipStreamSynchronize(b->stream));
  return queue_check(b);
}

extern "C" int dx_xfrc_ptr(dx_batch* b, void** devptr, int32_t* stride) {
  if (!b || !devptr) return dx_fail(DX_EINVAL, "null argument");
  if (!b->db.xfrc_stride) return dx_fail(DX_EINVAL, "the batch's applied wrenches are shared (dx_set_xfrc_env switches to per-env rows)");
  *devptr = b->xfrc_env;
  if (stride) *stride = b->db.xfrc_stride;
  return 0;
}

// The body pairs the watch test of the observation pass has to look at: those with
// `body` on one side and the watched geom's body on the other (as filtered in
// dx_step.hip collision), listed once here instead of filtered per env and step.
static int set_watch_pairs(dx_batch* b) {
  DevBatch& B = b->db;
  std::vector<int> list;
  if (B.watch_geom >= 0 && B.watch_body >= 0) {
    const auto& bb = b->model->hi.at("bpair_body");
    const int gbody = b->model->hi.at("geom_bodyid")[B.watch_geom];
    for (int k = 0; k < b->dm.nbpair; k++) {
      const int b1 = bb[2 * k], b2 = bb[2 * k + 1];
      if ((b1 == B.watch_body || b2 == B.watch_body) && (gbody == b1 || gbody == b2)) list.push_back(k);
    }
  }
  if (!b->watch_list) {
    void* p = nullptr;
    if (balloc(b, &p, (size_t)std::max(b->dm.nbpair, 1) * 4)) return DX_EHIP;
    b->watch_list = (int*)p;
  }
  if (!list.empty())
    HIPCHK(hipMemcpyAsync(b->watch_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  B.watch_pairs = b->watch_list;
  B.watch_npairs = (int)list.size();
  return 0;
}

extern "C" int dx_set_ground_geom(dx_batch* b, int32_t geom) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (geom >= b->dm.ngeom) return dx_fail(DX_EINVAL, "geom out of range");
  b->db.watch_geom = geom;
  return set_watch_pairs(b);
}

extern "C" int dx_set_watch(dx_batch* b, int32_t geom, int32_t body) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (geom >= b->dm.ngeom || body >= b->dm.nbody) return dx_fail(DX_EINVAL, "watch out of range");
  b->db.watch_geom = geom;
  b->db.watch_body = body;
  return set_watch_pairs(b);
}

// ---- kernel timing (HIP events around every step-kernel launch on the batch stream) ----
struct TimingState {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  bool on = false;
  unsigned n = 0, every = 1;
};
static std::map<const dx_batch*, TimingState> g_timing;

static void timing_begin(dx_batch* b, hipEvent_t* start) {
  auto it = g_timing.find(b);
  *start = nullptr;
  if (it == g_timing.end() || !it->second.on) return;
  if (it->second.n++ % it->second.every) return;  // (every every-th launch, dx_timing_enable)
  (void)hipEventCreate(start);
  (void)hipEventRecord(*start, b->stream);
}
static void timing_end(dx_batch* b, hipEvent_t start) {
  if (!start) return;
  hipEvent_t stop;
  (void)hipEventCreate(&stop);
  (void)hipEventRecord(stop, b->stream);
  g_timing[b].ev.emplace_back(start, stop);
}

extern "C" int dx_timing_enable(dx_batch* b, int enable) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  auto& st = g_timing[b];
  st.on = enable != 0;
  st.every = (unsigned)std::max(1, enable);
  st.n = 0;
  return 0;
}

extern "C" int dx_timing_read(dx_batch* b, double* total_ms, int32_t* count) {
  if (!b || !total_ms || !count) return dx_fail(DX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  double tot = 0;
  auto& st = g_timing[b];
  for (auto& p : st.ev) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
    tot += ms;
    (void)hipEventDestroy(p.first);
    (void)hipEventDestroy(p.second);
  }
  *total_ms = tot;
  *count = (int32_t)st.ev.size();
  st.ev.clear();
  return queue_check(b);
}

// The sensor kernel over the batch's stash (dx_sensor.hip): the torque sensors and the
// batch's contact sensing, whichever are on -- or, with `env_pads`, only a dx_env's pad
// forces into `env_out`, zero for the envs whose step type is FIRST.
int launch_sensor(dx_batch* b, const ContactSense* env_pads, float* env_out) {
  ContactSense C{};
  float* torque = nullptr;
  if (env_pads) {
    C = *env_pads;
    C.pad_force = env_out;
  } else {
    if (b->stash_users & dx_batch::STASH_TORQUE) torque = b->sensor;
    if (b->stash_users & dx_batch::STASH_CONTACT) {
      C.cfrc_ext = b->cfrc_ext;
      C.pad_force = b->npad ? b->pad_force : nullptr;
      C.pads = b->pads;
      C.npad = b->npad;
    }
  }
  HIPCHK(dx_launch_sensor(b->nenv, ((size_t)b->model->lds.total + 6 * DX_MAX_NV) * 4, b->stream, b->dm_dev, b->db,
                          b->model->lds, torque, C));
  return 0;
}

int launch_step(dx_batch* b, int nsub, int mode) {
  HIPCHK(hipSetDevice(b->device));
  size_t lds = (size_t)b->model->lds.total * 4;
  if (const char* pad = getenv("DX_LDS_PAD")) lds += (size_t)atol(pad);  // occupancy experiment
  // (progress tags 30 and 31 are markers: dx_step.hip DX_QUEUE_NSUB; a deferral entry
  // holds the physics step in 8 bits)
  if (b->db.defer && nsub > 255) return dx_fail(DX_EINVAL, "at most 255 physics steps per call");
  // The substep queue pays off when the batch has more envs than the chip has wave slots
  // (heavy contact-rich envs balanced over the slots).  A contact-free batch that fits the
  // slots (Shadow reach, 1024 envs) runs one workgroup per env for the whole control step:
  // every env starts at once anyway, and its physics steps then need no hand-offs.
  const bool queued = mode == 0 && b->queue && nsub <= 29 && (b->db.defer || b->nenv > b->slots);
  // a mode-0 step builds the next launch's longest-first order, placed by the overflow
  // tier's launch (or, without one, by the order kernel)
  DevBatch& Bo = b->db;
  Bo.onext = (mode == 0 && Bo.order && Bo.defer) ? 1 : 0;
  if (Bo.onext) Bo.opar ^= 1;
  // a queued launch with the mid tier beside it leaves one workgroup slot for it
  const bool mid = queued && b->mid;
  const int grid = queued ? (int)std::min<long>((long)b->nenv * nsub, b->slots - (mid ? 1 : 0)) : b->nenv;
  if (queued) {
    // substep queue: a new progress epoch and zeroed task counters
    DevBatch& B = b->db;
    if (++B.epoch >= (1u << 26)) {  // tags wrap: start over from zeroed progress
      HIPCHK(hipMemsetAsync(B.progress, 0, (size_t)b->nenv * 4, b->stream));
      B.epoch = 1;
    }
    if (!b->qhead_zero) HIPCHK(hipMemsetAsync(B.qhead, 0, DX_QUEUES * DX_QHEAD_STRIDE * 4, b->stream));
    b->qhead_zero = false;
  }
  Bo.mid = mid ? 1 : 0;
  hipEvent_t t0;
  timing_begin(b, &t0);
  hipError_t e = dx_launch_step(b->spec, grid, lds, b->stream, b->dm_dev, b->db, b->model->lds, nsub, queued ? 3 : mode);
  timing_end(b, t0);
  HIPCHK(e);
  // the mid tier, on its own stream, with no stream event in between (dx_step.hip
  // dx_step_mid_kernel: it waits on the device for this launch's workgroups to exit, and
  // the overflow tier below waits for it).  It is submitted after the step kernel: should
  // the two streams share a hardware queue it then runs after the step kernel instead of
  // ahead of it -- the mid tier waits for the step kernel, never the other way round.
  if (mid) {
    b->qdone_target += (unsigned)grid;
    HIPCHK(dx_launch_step_mid(1, (size_t)b->model->lds_mid.total * 4, b->side, b->dm_dev, b->db, b->model->lds_mid,
                              nsub, b->qdone_target));
  }
  // the overflow tier: physics steps whose contacts did not fit the step kernel's pool
  // (nothing to do unless some env deferred one), the next launch's longest-first order,
  // and the queue heads zeroed for the next launch
  if (b->db.defer && mode != 2) {
    HIPCHK(dx_launch_step_hi(b->hi_grid, (size_t)b->model->lds_hi.total * 4, b->stream, b->dm_dev, b->db,
                             b->model->lds_hi, nsub));
    b->qhead_zero = true;
  }
  Bo.mid = 0;
  // torque sensors and contact sensing from the last substep's stash (mode 0 step, mode 1
  // forward), one launch for both (a dx_env's contact forces follow its step: env_observe)
  if ((b->stash_users & (dx_batch::STASH_TORQUE | dx_batch::STASH_CONTACT)) && mode != 2)
    if (int rc = launch_sensor(b, nullptr, nullptr)) return rc;
  // next launch: heaviest environments first (costs just measured) -- for a model without
  // an overflow tier (contacts disabled), by the order kernel, which also zeroes the queue
  // heads the next queued launch claims from
  if (mode == 0 && b->db.order && !b->db.defer && (queued || b->nenv > b->slots)) {
    HIPCHK(dx_launch_order(b->nenv, b->stream, b->db.cost, (int*)b->db.order, b->db.qhead));
    b->qhead_zero = true;
  }
  return 0;
}

// (DX_DIVERGED of a call reports that call only: the step kernel clears an env's flag in
// its first physics-step task)
extern "C" int dx_step(dx_batch* b, int32_t nsubstep) {
  if (!b || nsubstep < 1) return dx_fail(DX_EINVAL, "bad batch or nsubstep");
  return launch_step(b, nsubstep, 0);
}

extern "C" int dx_forward(dx_batch* b) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  return launch_step(b, 1, 1);
}

extern "C" int dx_health(dx_batch* b, uint32_t* out, int32_t n) {
  if (!b || !out || n < 0) return dx_fail(DX_EINVAL, "null batch or output");
  HIPCHK(hipSetDevice(b->device));
  uint32_t h[DX_HEALTH_WORDS + DX_NCON_HIST];
  memset(h, 0, sizeof(h));
  HIPCHK(hipMemcpyAsync(h, b->db.health, DX_HEALTH_WORDS * 4, hipMemcpyDeviceToHost, b->stream));
  if (b->db.ncon_hist)
    HIPCHK(hipMemcpyAsync(h + DX_HEALTH_WORDS, b->db.ncon_hist, DX_NCON_HIST * 4, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  memcpy(out, h, std::min<size_t>(n, DX_HEALTH_WORDS + DX_NCON_HIST) * 4);
  return queue_check(b);
}

extern "C" int dx_health_clear(dx_batch* b) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemsetAsync(b->db.health, 0, DX_HEALTH_WORDS * 4, b->stream));
  if (b->db.ncon_hist) HIPCHK(hipMemsetAsync(b->db.ncon_hist, 0, DX_NCON_HIST * 4, b->stream));
  return 0;
}

extern "C" int dx_ncon_histogram(dx_batch* b, int enable) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (enable && !b->ncon_hist) {
    if (int rc = balloc(b, (void**)&b->ncon_hist, DX_NCON_HIST * 4)) return rc;
  }
  b->db.ncon_hist = enable ? b->ncon_hist : nullptr;
  return 0;
}

extern "C" void* dx_stream(dx_batch* b) { return b ? (void*)b->stream : nullptr; }

extern "C" int dx_sync(dx_batch* b) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  return queue_check(b);
}

extern "C" int dx_set_outputs(dx_batch* b, int bodies) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (b->RA.ncam) {
    // cameras read the body poses: they stay on, and the request is what comes back when
    // the cameras go off
    b->rnd_prev_bodies = bodies != 0;
    b->db.out_bodies = 1;
    return 0;
  }
  b->db.out_bodies = bodies != 0;
  return 0;
}

// The stash's readers: the step kernel writes it while any is on (buffers stay allocated,
// and their fields readable, until destroy).
int stash_use(dx_batch* b, int who, bool on) {
  if (on && !b->sen_stash) {
    const size_t E = b->nenv, words = (size_t)b->dm.nq + 2 * b->dm.nv + 1 + 8 * DX_NCON_HI;
    if (int rc = balloc(b, (void**)&b->sen_stash, E * words * 4)) return rc;
  }
  b->stash_users = on ? (b->stash_users | who) : (b->stash_users & ~who);
  b->db.sen_stash = b->stash_users ? b->sen_stash : nullptr;
  return 0;
}

extern "C" int dx_sensor_enable(dx_batch* b, int enable) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (enable && !b->sensor)
    if (int rc = balloc(b, (void**)&b->sensor, (size_t)b->nenv * 3 * b->dm.nbody * 4)) return rc;
  return stash_use(b, dx_batch::STASH_TORQUE, enable != 0);
}

// ---- contact force sensing (dx_sensor.hip) ----
static int contact_alloc(dx_batch* b) {
  if (b->pads) return 0;
  const size_t E = b->nenv;
  if (int rc = balloc(b, (void**)&b->cfrc_ext, E * 6 * b->dm.nbody * 4)) return rc;
  if (int rc = balloc(b, (void**)&b->pad_force, E * 3 * DX_MAX_PADS * 4)) return rc;
  return balloc(b, (void**)&b->pads, 2 * DX_MAX_PADS * 4);
}

extern "C" int dx_contact_enable(dx_batch* b, int enable) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->device));
  if (enable)
    if (int rc = contact_alloc(b)) return rc;
  return stash_use(b, dx_batch::STASH_CONTACT, enable != 0);
}

static int check_pads(const DevModel& d, const dx_contact_pad* pads, int32_t npad) {
  if (npad < 0 || (npad > 0 && !pads)) return dx_fail(DX_EINVAL, "contact pads: null table or negative count");
  if (npad > DX_MAX_PADS) return dx_fail(DX_ELIMIT, "contact pads: more than 64");
  for (int k = 0; k < npad; k++) {
    if (pads[k].body < 1 || pads[k].body >= d.nbody) return dx_fail(DX_EINVAL, "contact pads: body outside [1, nbody)");
    if (pads[k].partner_body < -1 || pads[k].partner_body >= d.nbody)
      return dx_fail(DX_EINVAL, "contact pads: partner body outside [-1, nbody)");
  }
  return 0;
}

extern "C" int dx_contact_set_pads(dx_batch* b, const dx_contact_pad* pads, int32_t npad) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (int rc = check_pads(b->dm, pads, npad)) return rc;  // (a rejected call changes nothing)
  HIPCHK(hipSetDevice(b->device));
  if (int rc = contact_alloc(b)) return rc;
  // the stream drained: no launch still reads the old table, and the rows of the new
  // pads read zero until the next step / forward
  HIPCHK(hipStreamSynchronize(b->stream));
  if (npad) HIPCHK(hipMemcpy(b->pads, pads, (size_t)npad * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(b->pad_force, 0, (size_t)b->nenv * 3 * DX_MAX_PADS * 4));
  b->npad = npad;
  return 0;
}

extern "C" int dx_contact_npad(const dx_batch* b) { return b ? b->npad : dx_fail(DX_EINVAL, "null batch"); }

extern "C" int dx_debug_enable(dx_batch* b, int enable) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  DevBatch& B = b->db;
  if (enable && !b->debug) {
    size_t E = b->nenv;
    int nv = b->dm.nv;
    int rc = 0;
    rc |= balloc(b, (void**)&B.dbg_qacc_smooth, E * nv * 4);
    rc |= balloc(b, (void**)&B.dbg_qfrc_smooth, E * nv * 4);
    rc |= balloc(b, (void**)&B.dbg_M, E * nv * nv * 4);
    rc |= balloc(b, (void**)&B.dbg_con, E * DX_NCON_HI * 16 * 4);
    rc |= balloc(b, (void**)&B.dbg_nefc, E * 2 * 4);
    if (rc) return rc;
    b->debug = true;
  } else if (!enable) {
    B.dbg_qacc_smooth = nullptr;  // buffers stay allocated until destroy
    B.dbg_qfrc_smooth = nullptr;
    B.dbg_M = nullptr;
    B.dbg_con = nullptr;
    B.dbg_nefc = nullptr;
    b->debug = false;
  }
  return 0;
}

extern "C" int dx_debug_get(dx_batch* b, const char* name, float* dst, size_t nfloats) {
  if (!b || !name || !dst) return dx_fail(DX_EINVAL, "null argument");
  DevBatch& B = b->db;
  if (std::string(name) == "queue_timeouts") {  // int32 bits: 1 if a queued task ever gave up waiting
    if (nfloats < 1) return dx_fail(DX_EINVAL, "destination too small");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(dst, B.qerr, 4, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
  }
  if (std::string(name) == "health") {  // uint32 bits: dx_health's counters (+ histogram)
    return dx_health(b, (uint32_t*)dst, (int32_t)std::min<size_t>(nfloats, DX_HEALTH_WORDS + DX_NCON_HIST));
  }
  if (std::string(name) == "queue_slots") {  // int32 bits: the queued launch's persistent workgroups
    if (nfloats < 1) return dx_fail(DX_EINVAL, "destination too small");
    memcpy(dst, &b->slots, 4);
    return 0;
  }
  // the body-pair cull's host tables (dx_model_load): their sizes {nbitem, nbplane, nbpair}
  // as int32 bits, bp_item [nbitem][8] floats, bp_cull [nbpair][2] int32 bits
  if (std::string(name) == "bp_sizes") {
    if (nfloats < 3) return dx_fail(DX_EINVAL, "destination too small");
    const int v[3] = {b->dm.nbitem, b->dm.nbplane, b->dm.nbpair};
    memcpy(dst, v, sizeof(v));
    return 0;
  }
  if (std::string(name) == "bp_item" || std::string(name) == "bp_cull") {
    const bool item = std::string(name) == "bp_item";
    const size_t n = item ? (size_t)8 * b->dm.nbitem : (size_t)2 * b->dm.nbpair;
    if (nfloats < n) return dx_fail(DX_EINVAL, "destination too small");
    if (n) memcpy(dst, item ? (const void*)b->model->hf.at("bp_item").data() : (const void*)b->model->hi.at("bp_cull").data(), n * 4);
    return 0;
  }
  if (!b->debug) return dx_fail(DX_EINVAL, "debug not enabled");
  size_t E = b->nenv, nv = b->dm.nv;
  const void* src = nullptr;
  size_t n = 0;
  std::string s(name);
  if (s == "qacc_smooth") { src = B.dbg_qacc_smooth; n = E * nv; }
  else if (s == "qfrc_smooth") { src = B.dbg_qfrc_smooth; n = E * nv; }
  else if (s == "M") { src = B.dbg_M; n = E * nv * nv; }
  else if (s == "contact") { src = B.dbg_con; n = E * DX_NCON_HI * 16; }
  else if (s == "efc_count") { src = B.dbg_nefc; n = E * 2; }
  else return dx_fail(DX_EINVAL, "unknown debug field");
  if (nfloats < n) return dx_fail(DX_EINVAL, "destination too small");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// Fills every CU's LDS with NaN bit patterns (test hook: the step kernel must not
// depend on LDS contents left by earlier workgroups).
__global__ void dx_poison_lds_kernel(int nwords) {
  extern __shared__ unsigned int lds_words[];
  for (int k = threadIdx.x; k < nwords; k += blockDim.x) lds_words[k] = 0x7fc00000u | (k & 0xff);
  __syncthreads();
}

extern "C" int dx_debug_poison_lds(int32_t device) {
  HIPCHK(hipSetDevice(device));
  const int bytes = 64 * 1024;
  hipLaunchKernelGGL(dx_poison_lds_kernel, dim3(256 * 16), dim3(256), bytes, nullptr, bytes / 4);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

extern "C" int dx_stage_timing(dx_batch* b, int enable) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->device));
  size_t bytes = (size_t)b->nenv * DX_NSTAGE * 8;  // per-env accumulators: no atomics
  if (enable && !b->db.stage_acc) {
    void* p = nullptr;
    if (int rc = balloc(b, &p, bytes)) return rc;
    HIPCHK(hipMemsetAsync(p, 0, bytes, b->stream));
    b->db.stage_acc = (unsigned long long*)p;
  } else if (!enable) {
    b->db.stage_acc = nullptr;
  }
  // the launches now run the instrumented twins (on) or the production kernels (off): the
  // queue's persistent grid is the occupancy of the kernel it launches
  step_slots(b);
  return 0;
}

extern "C" int dx_stage_read(dx_batch* b, uint64_t* out, int32_t n) {
  if (!b || !out) return dx_fail(DX_EINVAL, "null argument");
  if (!b->db.stage_acc) return dx_fail(DX_EINVAL, "stage timing not enabled");
  HIPCHK(hipSetDevice(b->device));
  size_t cnt = (size_t)b->nenv * DX_NSTAGE;
  std::vector<uint64_t> h(cnt);
  HIPCHK(hipMemcpyAsync(h.data(), b->db.stage_acc, cnt * 8, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipMemsetAsync(b->db.stage_acc, 0, cnt * 8, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  if ((size_t)n >= cnt) {  // per env: out[env][DX_NSTAGE]
    memcpy(out, h.data(), cnt * 8);
    return 0;
  }
  for (int k = 0; k < std::min(n, DX_NSTAGE); k++) {
    uint64_t t = 0;
    for (int e = 0; e < b->nenv; e++) t += h[(size_t)e * DX_NSTAGE + k];
    out[k] = t;
  }
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}
