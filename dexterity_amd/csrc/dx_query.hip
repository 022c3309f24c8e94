// dx_query.hip -- the calls that read a batch through per-call device scratch (CallScratch):
// Jacobians, IK and the velocity mapper, cameras and rays.
#include "dx_host.h"

// ---- site Jacobians and batched IK (dx_ik.hip) ----
static int ik_check_sites(dx_batch* b, const int32_t* sites, int32_t nsite) {
  if (!sites || nsite < 1 || 3 * nsite > 32) return dx_fail(DX_EINVAL, "need 1 <= nsite <= 10 site ids");
  for (int s = 0; s < nsite; s++)
    if (sites[s] < 0 || sites[s] >= b->dm.nsite) return dx_fail(DX_EINVAL, "site id out of range");
  return 0;
}

// The model's LDS layout plus a query kernel's own block of `words`, in bytes.
static int query_lds_bytes(dx_batch* b, int words, const char* who, size_t* bytes) {
  *bytes = ((size_t)b->model->lds.total + words) * 4;
  if (*bytes > 160 * 1024) return dx_fail(DX_ELIMIT, std::string(who) + " LDS footprint exceeds 160 KiB");
  return 0;
}

extern "C" int dx_jac_site(dx_batch* b, const int32_t* sites, int32_t nsite, float* jacp, float* jacr) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (int rc = ik_check_sites(b, sites, nsite)) return rc;
  size_t lds;
  if (int rc = query_lds_bytes(b, dx_ik_lds_words(b->dm, 0), "IK", &lds)) return rc;
  HIPCHK(hipSetDevice(b->device));
  CallScratch S(b->stream);
  IkDev P;
  memset(&P, 0, sizeof(P));
  P.mode = 1;
  P.nsite = nsite;
  P.blk = b->model->lds.total;
  const size_t n = (size_t)b->nenv * 3 * nsite * b->dm.nv;
  int* ds = (int*)S.get(nsite * 4);
  P.jacp = jacp ? (float*)S.get(n * 4) : nullptr;
  P.jacr = jacr ? (float*)S.get(n * 4) : nullptr;
  if (!ds || (jacp && !P.jacp) || (jacr && !P.jacr)) return dx_fail(DX_ENOMEM, "device scratch allocation failed");
  P.sites = ds;
  HIPCHK(hipMemcpyAsync(ds, sites, nsite * 4, hipMemcpyHostToDevice, b->stream));
  HIPCHK(dx_launch_ik(b->nenv, lds, b->stream, b->dm_dev, b->db, b->model->lds, P));
  if (jacp) HIPCHK(hipMemcpyAsync(jacp, P.jacp, n * 4, hipMemcpyDefault, b->stream));
  if (jacr) HIPCHK(hipMemcpyAsync(jacr, P.jacr, n * 4, hipMemcpyDefault, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" int dx_ik_solve(dx_batch* b, const dx_ik_options* opt, const int32_t* sites, int32_t nsite,
                           const int32_t* joints, int32_t njoint, const float* targets, float* qpos_out,
                           int32_t* success, float* linear_err, int32_t* attempt, int32_t* steps) {
  if (!b || !opt || !targets) return dx_fail(DX_EINVAL, "null batch, options or targets");
  if (int rc = ik_check_sites(b, sites, nsite)) return rc;
  if (!joints || njoint < 1 || njoint > DX_MAX_NV) return dx_fail(DX_EINVAL, "need 1 <= njoint <= 64 joint ids");
  const std::vector<int>& jtype = b->model->hi.at("jnt_type");
  for (int k = 0; k < njoint; k++) {
    if (joints[k] < 0 || joints[k] >= b->dm.njnt) return dx_fail(DX_EINVAL, "joint id out of range");
    if (jtype[joints[k]] == DXJ_FREE) return dx_fail(DX_EINVAL, "IK joints must be hinge or slide joints");
  }
  if (opt->max_steps < 1 || opt->num_attempts < 1) return dx_fail(DX_EINVAL, "max_steps and num_attempts must be >= 1");
  if (!(opt->regularization > 0.f)) return dx_fail(DX_EINVAL, "regularization must be positive");
  size_t lds;
  if (int rc = query_lds_bytes(b, dx_ik_lds_words(b->dm, 0), "IK", &lds)) return rc;
  const size_t E = b->nenv, A = opt->num_attempts;
  if (E * A > 0x7fffffffull) return dx_fail(DX_EINVAL, "nenv * num_attempts too large");
  HIPCHK(hipSetDevice(b->device));
  CallScratch S(b->stream);
  IkDev P;
  memset(&P, 0, sizeof(P));
  P.mode = 0;
  P.nsite = nsite;
  P.njoint = njoint;
  P.max_steps = opt->max_steps;
  P.early_stop = opt->early_stop != 0;
  P.nattempt = (int)A;
  P.stop_on_first = opt->stop_on_first != 0;
  P.tol = opt->linear_tol;
  P.reg = opt->regularization;
  P.gain = opt->gain;
  P.progress = opt->progress_threshold;
  P.seed = opt->seed;
  P.blk = b->model->lds.total;
  int* ds = (int*)S.get(nsite * 4);
  int* dj = (int*)S.get(njoint * 4);
  float* dt = (float*)S.get(E * 3 * nsite * 4);
  P.att_qpos = (float*)S.get(E * A * njoint * 4);
  P.att_err = (float*)S.get(E * A * nsite * 4);
  P.att_steps = (int*)S.get(E * A * 4);
  float* oq = (float*)S.get(E * njoint * 4);
  int* os = (int*)S.get(E * 4);
  float* oe = (float*)S.get(E * nsite * 4);
  int* oa = (int*)S.get(E * 4);
  int* ot = (int*)S.get(E * 4);
  if (!ds || !dj || !dt || !P.att_qpos || !P.att_err || !P.att_steps || !oq || !os || !oe || !oa || !ot)
    return dx_fail(DX_ENOMEM, "device scratch allocation failed");
  HIPCHK(hipMemcpyAsync(ds, sites, nsite * 4, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(dj, joints, njoint * 4, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(dt, targets, E * 3 * nsite * 4, hipMemcpyDefault, b->stream));
  P.sites = ds;
  P.joints = dj;
  P.targets = dt;
  P.starts = nullptr;
  if (A > 1) {  // numpy-compatible random restarts (dx_ik.hip dx_ik_starts_kernel)
    auto it = b->model->arr.find("jnt_range");
    if (it == b->model->arr.end() || it->second.dtype != 1) return dx_fail(DX_EMODEL, "model has no fp64 jnt_range");
    std::vector<double> rng(2 * (size_t)njoint);
    for (int k = 0; k < njoint; k++) {
      rng[2 * k] = ((const double*)it->second.p)[2 * joints[k]];
      rng[2 * k + 1] = ((const double*)it->second.p)[2 * joints[k] + 1];
    }
    double* drng = (double*)S.get(rng.size() * 8);
    uint32_t* mt = (uint32_t*)S.get(E * DX_MT_WORDS * 4);
    float* st = (float*)S.get(E * (A - 1) * njoint * 4);
    if (!drng || !mt || !st) return dx_fail(DX_ENOMEM, "device scratch allocation failed");
    HIPCHK(hipMemcpyAsync(drng, rng.data(), rng.size() * 8, hipMemcpyHostToDevice, b->stream));
    HIPCHK(dx_launch_ik_starts((int)E, (int)A - 1, njoint, opt->seed, drng, mt, st, b->stream));
    P.starts = st;
  }
  HIPCHK(dx_launch_ik((int)(E * A), lds, b->stream, b->dm_dev, b->db, b->model->lds, P));
  HIPCHK(dx_launch_ik_select((int)E, b->stream, b->dm, P, oq, os, oe, oa, ot));
  if (qpos_out) HIPCHK(hipMemcpyAsync(qpos_out, oq, E * njoint * 4, hipMemcpyDefault, b->stream));
  if (success) HIPCHK(hipMemcpyAsync(success, os, E * 4, hipMemcpyDefault, b->stream));
  if (linear_err) HIPCHK(hipMemcpyAsync(linear_err, oe, E * nsite * 4, hipMemcpyDefault, b->stream));
  if (attempt) HIPCHK(hipMemcpyAsync(attempt, oa, E * 4, hipMemcpyDefault, b->stream));
  if (steps) HIPCHK(hipMemcpyAsync(steps, ot, E * 4, hipMemcpyDefault, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// dx_jac_object / dx_dls_map: the controlled objects as points (dx_internal.h DlsDev).
// Every argument error returns here, before any launch.
static int dls_points(dx_batch* b, const int32_t* types, const int32_t* ids, int32_t nobj, DlsDev& P) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (!types || !ids || nobj < 1) return dx_fail(DX_EINVAL, "need nobj >= 1 object types and ids");
  const dx_model* m = b->model;
  memset(&P, 0, sizeof(P));
  for (int k = 0; k < nobj; k++) {
    const int t = types[k], id = ids[k];
    const int n = t == DX_OBJ_BODY ? b->dm.nbody : t == DX_OBJ_GEOM ? b->dm.ngeom : t == DX_OBJ_SITE ? b->dm.nsite : -1;
    if (n < 0) return dx_fail(DX_EINVAL, "object type must be DX_OBJ_BODY, DX_OBJ_GEOM or DX_OBJ_SITE");
    if (id < 0 || id >= n) return dx_fail(DX_EINVAL, "object id out of range");
    if (k >= DX_DLS_MAXPT) continue;  // (DX_ELIMIT below, after every object was validated)
    const float* off = nullptr;
    int body = id;
    if (t == DX_OBJ_GEOM) {
      body = m->hi.at("geom_bodyid")[id];
      off = m->hf.at("geom_pos").data() + 3 * id;
    } else if (t == DX_OBJ_SITE) {
      body = m->hi.at("site_bodyid")[id];
      off = m->hf.at("site_pos").data() + 3 * id;
    }
    P.body[k] = body;
    for (int e = 0; e < 3; e++) P.off[3 * k + e] = off ? off[e] : 0.f;
  }
  if (3 * nobj > 32) return dx_fail(DX_ELIMIT, "3 * nobj must be <= 32 (one 32 x 32 matrix-core tile)");
  if (b->dm.nv > DX_MAX_NV) return dx_fail(DX_ELIMIT, "nv must be <= 64");
  P.npoint = nobj;
  P.blk = m->lds.total;
  return 0;
}

// Host or device memory?  (An address HIP does not know is ordinary host memory.)
static bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

// One argument array of a mapper call: device memory is used in place; host memory is
// staged through device scratch (copied in before the launch, or out after it).
struct DlsArg {
  void* user = nullptr;
  void* dev = nullptr;
  size_t bytes = 0;
  bool staged = false;
};
static bool dls_arg(DlsArg& a, const void* user, size_t bytes, std::unique_ptr<CallScratch>& S, hipStream_t stream) {
  a.user = (void*)user;
  a.bytes = bytes;
  if (!user) return true;
  if (is_device_ptr(user)) {
    a.dev = a.user;
    return true;
  }
  if (!S) S.reset(new CallScratch(stream));
  a.dev = S->get(bytes);
  a.staged = true;
  return a.dev != nullptr;
}

extern "C" int dx_jac_object(dx_batch* b, const int32_t* types, const int32_t* ids, int32_t nobj, float* jacp,
                             float* jacr) {
  DlsDev P;
  if (int rc = dls_points(b, types, ids, nobj, P)) return rc;
  size_t lds;
  if (int rc = query_lds_bytes(b, dx_dls_lds_words(b->dm), "mapper", &lds)) return rc;
  HIPCHK(hipSetDevice(b->device));
  const size_t n = (size_t)b->nenv * 3 * nobj * b->dm.nv * 4;
  std::unique_ptr<CallScratch> S;  // (synchronises the stream when it goes)
  DlsArg ap, ar;
  if (!dls_arg(ap, jacp, n, S, b->stream) || !dls_arg(ar, jacr, n, S, b->stream))
    return dx_fail(DX_ENOMEM, "device scratch allocation failed");
  P.mode = 1;
  P.jacp = (float*)ap.dev;
  P.jacr = (float*)ar.dev;
  HIPCHK(dx_launch_dls(b->nenv, lds, b->stream, b->dm_dev, b->db, b->model->lds, P));
  if (ap.staged) HIPCHK(hipMemcpyAsync(ap.user, ap.dev, n, hipMemcpyDeviceToHost, b->stream));
  if (ar.staged) HIPCHK(hipMemcpyAsync(ar.user, ar.dev, n, hipMemcpyDeviceToHost, b->stream));
  if (S) HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" int dx_dls_map(dx_batch* b, const int32_t* types, const int32_t* ids, int32_t nobj, float regularization,
                          const float* target_vel, float* qvel_out, int32_t* status) {
  DlsDev P;
  if (int rc = dls_points(b, types, ids, nobj, P)) return rc;
  if (!(regularization >= 0.f) || std::isinf(regularization))
    return dx_fail(DX_EINVAL, "regularization must be finite and non-negative");
  if (!target_vel || !qvel_out) return dx_fail(DX_EINVAL, "null target_vel or qvel_out");
  size_t lds;
  if (int rc = query_lds_bytes(b, dx_dls_lds_words(b->dm), "mapper", &lds)) return rc;
  HIPCHK(hipSetDevice(b->device));
  const size_t E = b->nenv;
  std::unique_ptr<CallScratch> S;  // (synchronises the stream when it goes)
  DlsArg at, aq, as;
  if (!dls_arg(at, target_vel, E * 3 * nobj * 4, S, b->stream) || !dls_arg(aq, qvel_out, E * b->dm.nv * 4, S, b->stream) ||
      !dls_arg(as, status, E * 4, S, b->stream))
    return dx_fail(DX_ENOMEM, "device scratch allocation failed");
  if (at.staged) HIPCHK(hipMemcpyAsync(at.dev, at.user, at.bytes, hipMemcpyHostToDevice, b->stream));
  P.mode = 0;
  P.reg = regularization;
  P.target = (const float*)at.dev;
  P.qvel = (float*)aq.dev;
  P.status = (int*)as.dev;
  HIPCHK(dx_launch_dls((int)E, lds, b->stream, b->dm_dev, b->db, b->model->lds, P));
  if (aq.staged) HIPCHK(hipMemcpyAsync(aq.user, aq.dev, aq.bytes, hipMemcpyDeviceToHost, b->stream));
  if (as.staged) HIPCHK(hipMemcpyAsync(as.user, as.dev, as.bytes, hipMemcpyDeviceToHost, b->stream));
  if (S) HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// ---- cameras and rays (dx_render.hip) ----
// The model tables and the batch's poses every render / ray launch reads.
static int render_base(dx_batch* b, RenderArgs& A) {
  dx_model::RenderDev T;
  if (int rc = render_tables(b->model, b->device, &T)) return rc;
  const DevModel& d = b->dm;
  A.nenv = b->nenv; A.ngeom = d.ngeom; A.nbody = d.nbody;
  A.xpos = b->db.xpos; A.xquat = b->db.xquat;
  A.geom_type = d.geom_type; A.geom_bodyid = d.geom_bodyid; A.geom_dataid = d.geom_dataid;
  A.geom_size = d.geom_size; A.geom_pos = d.geom_pos; A.geom_mat = d.geom_mat; A.geom_bsphere = d.geom_bsphere;
  A.mesh_planeadr = (decltype(A.mesh_planeadr))T.planeadr;
  A.mesh_planenum = (decltype(A.mesh_planenum))T.planenum;
  A.plane4 = (decltype(A.plane4))T.plane4;
  return 0;
}

// A camera's frame from xyaxes, in fp64: x normalised, y made orthogonal to x and
// normalised, z = x (x) y.  False: degenerate axes.
static bool camera_frame(const dx_camera& c, RenderCam& out, int height) {
  double x[3] = {c.xyaxes[0], c.xyaxes[1], c.xyaxes[2]}, y[3] = {c.xyaxes[3], c.xyaxes[4], c.xyaxes[5]};
  for (int k = 0; k < 6; k++)
    if (!std::isfinite(c.xyaxes[k])) return false;
  const double nx = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (!(nx > 1e-10)) return false;
  for (double& v : x) v /= nx;
  const double dot = x[0] * y[0] + x[1] * y[1] + x[2] * y[2];
  for (int k = 0; k < 3; k++) y[k] -= dot * x[k];
  const double ny = std::sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
  if (!(ny > 1e-10)) return false;
  for (double& v : y) v /= ny;
  const double z[3] = {x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]};
  for (int k = 0; k < 3; k++) {
    out.pos[k] = c.pos[k];
    out.x[k] = (float)x[k]; out.y[k] = (float)y[k]; out.z[k] = (float)z[k];
  }
  out.f = (float)(0.5 * height / std::tan(0.5 * (double)c.fovy * 3.14159265358979323846 / 180.0));
  out.near_ = c.near_;
  out.far_ = c.far_;
  out.body = c.body;
  return true;
}

// A buffer of at least `words` words for a new configuration: the current one when it is
// large enough, else a fresh allocation (*fresh).  Nothing is freed here: the caller swaps
// the fresh buffers in, and frees the ones they replace, only once every step has
// succeeded, so a failed call leaves the active configuration and its images as they were.
static int render_buffer(dx_batch* b, void* cur, size_t cap, size_t words, void** out, bool* fresh) {
  *fresh = false;
  *out = cur;
  if (cap >= words) return 0;
  void* p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(words * 4, 4)) != hipSuccess) {
    (void)hipGetLastError();
    return dx_fail(DX_ENOMEM, "cameras: image allocation failed");
  }
  if (hipMemsetAsync(p, 0, words * 4, b->stream) != hipSuccess) {
    (void)hipFree(p);
    return dx_fail(DX_EHIP, "cameras: image clear failed");
  }
  *out = p;
  *fresh = true;
  return 0;
}
static void render_adopt(dx_batch* b, void** slot, size_t* cap, void* fresh, size_t words) {
  if (*slot) {
    (void)hipFree(*slot);
    b->allocs.erase(std::remove(b->allocs.begin(), b->allocs.end(), *slot), b->allocs.end());
  }
  *slot = fresh;
  *cap = words;
  b->allocs.push_back(fresh);
}

extern "C" int dx_render_set_cameras(dx_batch* b, const dx_camera* cams, int32_t ncam, int32_t width, int32_t height,
                                     int32_t flags) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));  // may be called between steps
  if (ncam == 0) {  // off: nothing is launched, the buffers stay for a later call
    b->RA.ncam = 0;
    b->rnd_flags = 0;
    if (b->rnd_prev_bodies >= 0) b->db.out_bodies = b->rnd_prev_bodies;
    b->rnd_prev_bodies = -1;
    return 0;
  }
  if (!cams || ncam < 0) return dx_fail(DX_EINVAL, "cameras: null camera array or negative count");
  if (width < 1 || height < 1) return dx_fail(DX_EINVAL, "cameras: width and height must be positive");
  if (flags & ~(DX_RENDER_DEPTH | DX_RENDER_SEGMENTATION | DX_RENDER_NO_CULL | DX_RENDER_RGB))
    return dx_fail(DX_EINVAL, "cameras: unknown flag");
  if (!(flags & (DX_RENDER_DEPTH | DX_RENDER_SEGMENTATION | DX_RENDER_RGB)))
    return dx_fail(DX_EINVAL, "cameras: no output flag (DX_RENDER_DEPTH / DX_RENDER_SEGMENTATION / DX_RENDER_RGB)");
  if (ncam > DX_RENDER_MAX_CAMERAS) return dx_fail(DX_ELIMIT, "cameras: more than 8 cameras");
  if (width > DX_RENDER_MAX_SIDE || height > DX_RENDER_MAX_SIDE) return dx_fail(DX_ELIMIT, "cameras: a side above 512 pixels");
  const unsigned long long npix = (unsigned long long)b->nenv * ncam * height * width;
  if (npix >= 0x80000000ull) return dx_fail(DX_ELIMIT, "cameras: nenv * ncam * height * width reaches 2^31");
  RenderArgs A{};
  for (int i = 0; i < ncam; i++) {
    const dx_camera& c = cams[i];
    if (!(c.fovy > 0.f && c.fovy < 180.f)) return dx_fail(DX_EINVAL, "cameras: fovy outside (0, 180) degrees");
    if (!(c.near_ > 0.f) || !(c.far_ > c.near_) || !std::isfinite(c.far_))
      return dx_fail(DX_EINVAL, "cameras: need 0 < near < far (finite)");
    if (c.body < -1 || c.body >= b->dm.nbody) return dx_fail(DX_EINVAL, "cameras: body outside [-1, nbody)");
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(c.pos[k])) return dx_fail(DX_EINVAL, "cameras: a non-finite position");
    if (!camera_frame(c, A.cam[i], height)) return dx_fail(DX_EINVAL, "cameras: degenerate xyaxes");
  }
  if (int rc = render_base(b, A)) return rc;
  // the shading pass reads the cast's depth and geom ids: with RGB on the cast writes both,
  // into the same buffers, whether or not the caller asked for them (rnd_flags says which)
  const bool rgb = (flags & DX_RENDER_RGB) != 0;
  const bool want_d = rgb || (flags & DX_RENDER_DEPTH), want_s = rgb || (flags & DX_RENDER_SEGMENTATION);
  if (rgb && !b->shade_set)  // the documented default shading
    if (int rc = dx_render_set_shading(b, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr)) return rc;
  const size_t rgb_words = (size_t)((npix * 3 + 3) / 4);
  void *nd = b->rnd_depth, *ns = b->rnd_seg, *nc = b->rnd_rgb;
  bool fd = false, fs = false, fc = false;
  int rc = 0;
  if (want_d) rc = render_buffer(b, b->rnd_depth, b->rnd_depth_cap, (size_t)npix, &nd, &fd);
  if (!rc && want_s) rc = render_buffer(b, b->rnd_seg, b->rnd_seg_cap, (size_t)npix, &ns, &fs);
  if (!rc && rgb) rc = render_buffer(b, b->rnd_rgb, b->rnd_rgb_cap, rgb_words, &nc, &fc);
  if (!rc && hipStreamSynchronize(b->stream) != hipSuccess) rc = dx_fail(DX_EHIP, "cameras: stream sync failed");
  if (rc) {
    if (fd) (void)hipFree(nd);
    if (fs) (void)hipFree(ns);
    if (fc) (void)hipFree(nc);
    return rc;
  }
  // every step has succeeded: the new buffers replace the old ones
  if (fd) render_adopt(b, (void**)&b->rnd_depth, &b->rnd_depth_cap, nd, (size_t)npix);
  if (fs) render_adopt(b, (void**)&b->rnd_seg, &b->rnd_seg_cap, ns, (size_t)npix);
  if (fc) render_adopt(b, (void**)&b->rnd_rgb, &b->rnd_rgb_cap, nc, rgb_words);
  A.ncam = ncam; A.W = width; A.H = height;
  A.tiles_x = (width + DX_RENDER_TILE - 1) / DX_RENDER_TILE;
  A.tiles_y = (height + DX_RENDER_TILE - 1) / DX_RENDER_TILE;
  A.no_cull = (flags & DX_RENDER_NO_CULL) ? 1 : 0;
  A.depth = want_d ? b->rnd_depth : nullptr;
  A.seg = want_s ? b->rnd_seg : nullptr;
  b->RA = A;
  b->rnd_flags = flags;
  if (b->rnd_prev_bodies < 0) b->rnd_prev_bodies = b->db.out_bodies;
  b->db.out_bodies = 1;
  return 0;
}

extern "C" int dx_render(dx_batch* b) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (!b->RA.ncam) return dx_fail(DX_EINVAL, "render: no cameras (dx_render_set_cameras)");
  HIPCHK(hipSetDevice(b->device));
  RenderArgs A = b->RA;
  A.stats = b->rnd_stats_on ? b->rnd_stats : nullptr;
  HIPCHK(dx_launch_render(b->stream, A));
  if (b->rnd_flags & DX_RENDER_RGB) {  // the shading pass, over the images the cast just wrote
    ShadeArgs S{};
    S.R = A;
    S.S = b->shade;
    S.geom_rgb = b->shade_tab;
    S.rgb = b->rnd_rgb;
    S.stats = A.stats ? A.stats + 3 : nullptr;
    HIPCHK(dx_launch_shade(b->stream, S));
  }
  return 0;
}

extern "C" int dx_render_output(dx_batch* b, int which, void** devptr) {
  if (!b || !devptr) return dx_fail(DX_EINVAL, "null argument");
  if (!b->RA.ncam) return dx_fail(DX_EINVAL, "render: no cameras (dx_render_set_cameras)");
  // (with RGB on the cast's buffers exist without having been asked for: the flags decide)
  if (which == DX_RENDER_DEPTH && (b->rnd_flags & DX_RENDER_DEPTH)) { *devptr = b->RA.depth; return 0; }
  if (which == DX_RENDER_SEGMENTATION && (b->rnd_flags & DX_RENDER_SEGMENTATION)) { *devptr = b->RA.seg; return 0; }
  if (which == DX_RENDER_RGB && (b->rnd_flags & DX_RENDER_RGB)) { *devptr = b->rnd_rgb; return 0; }
  return dx_fail(DX_EINVAL, "render: that output is not enabled");
}

// The documented default palette (dexterity_amd/cameras.py default_palette mirrors it): the
// world's geoms one colour, each hand's -- a tree whose root has no free joint, in root order --
// one of two, a free-jointed prop's geoms one, and the first such box six face colours.
static const float kPaletteWorld[3] = {0.45f, 0.45f, 0.5f}, kPaletteProp[3] = {0.8f, 0.8f, 0.8f};
static const float kPaletteHands[2][3] = {{0.85f, 0.65f, 0.5f}, {0.5f, 0.65f, 0.85f}};
static const float kPaletteFaces[6][3] = {{0.9f, 0.1f, 0.1f}, {0.1f, 0.8f, 0.1f}, {0.1f, 0.2f, 0.9f},
                                          {0.9f, 0.8f, 0.1f}, {0.9f, 0.1f, 0.9f}, {0.1f, 0.8f, 0.8f}};
static void default_palette(const dx_model* m, std::vector<float>& rgb, int* face_geom) {
  const auto& gb = m->hi.at("geom_bodyid");
  const auto& gt = m->hi.at("geom_type");
  const auto& root = m->hi.at("body_rootid");
  const auto& jt = m->hi.at("jnt_type");
  const auto& jb = m->hi.at("jnt_bodyid");
  std::vector<int> free_root(root.size(), 0), hands;
  for (size_t j = 0; j < jt.size(); j++)
    if (jt[j] == 0) free_root[root[jb[j]]] = 1;
  *face_geom = -1;
  rgb.assign(gb.size() * 3, 0.f);
  for (size_t g = 0; g < gb.size(); g++) {
    const int r = root[gb[g]];
    const float* c = kPaletteWorld;
    if (gb[g] != 0 && free_root[r]) {
      c = kPaletteProp;
      if (gt[g] == DXG_BOX && *face_geom < 0) *face_geom = (int)g;
    } else if (gb[g] != 0) {
      auto it = std::find(hands.begin(), hands.end(), r);
      if (it == hands.end()) it = hands.insert(hands.end(), r);
      c = kPaletteHands[(it - hands.begin()) % 2];
    }
    for (int k = 0; k < 3; k++) rgb[3 * g + k] = c[k];
  }
}

static bool finite_all(const float* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

extern "C" int dx_render_set_shading(dx_batch* b, const float* geom_rgb, const int32_t* face_geom, const float* face_rgb,
                                     int32_t nface, const dx_light* lights, int32_t nlight, const dx_shading* shading) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  const dx_model* m = b->model;
  const int ngeom = b->dm.ngeom;
  if (nface < 0 || nlight < 0) return dx_fail(DX_EINVAL, "shading: a negative count");
  if (nface > DX_RENDER_MAX_FACE_GEOMS) return dx_fail(DX_ELIMIT, "shading: more than 8 face geoms");
  if (nlight > DX_RENDER_MAX_LIGHTS) return dx_fail(DX_ELIMIT, "shading: more than 4 lights");
  if ((nface && (!face_geom || !face_rgb)) || (nlight && !lights))
    return dx_fail(DX_EINVAL, "shading: a null array with a positive count");
  ShadeSet S{};
  std::vector<float> tab;
  int def_face = -1;
  default_palette(m, tab, &def_face);
  if (geom_rgb) {
    if (!finite_all(geom_rgb, (size_t)ngeom * 3)) return dx_fail(DX_EINVAL, "shading: a non-finite geom colour");
    std::copy(geom_rgb, geom_rgb + (size_t)ngeom * 3, tab.begin());
  }
  tab.resize((size_t)ngeom * 3 + DX_RENDER_MAX_FACE_GEOMS * 18, 0.f);
  float* faces = tab.data() + (size_t)ngeom * 3;
  if (!geom_rgb && !face_geom && def_face >= 0) {  // the default palette's prop box
    S.nface = 1;
    S.face_geom[0] = def_face;
    std::copy(&kPaletteFaces[0][0], &kPaletteFaces[0][0] + 18, faces);
  } else {
    const auto& gt = m->hi.at("geom_type");
    for (int i = 0; i < nface; i++) {
      if (face_geom[i] < 0 || face_geom[i] >= ngeom || gt[face_geom[i]] != DXG_BOX)
        return dx_fail(DX_EINVAL, "shading: a face geom that is not a box geom");
      for (int j = 0; j < i; j++)
        if (face_geom[j] == face_geom[i]) return dx_fail(DX_EINVAL, "shading: a repeated face geom");
      S.face_geom[i] = face_geom[i];
    }
    if (nface && !finite_all(face_rgb, (size_t)nface * 18)) return dx_fail(DX_EINVAL, "shading: a non-finite face colour");
    if (nface) std::copy(face_rgb, face_rgb + (size_t)nface * 18, faces);
    S.nface = nface;
  }
  if (!lights) {  // the arena's light: directional, straight down, casting shadows
    S.nlight = 1;
    S.light[0] = ShadeLight{{0.f, 0.f, 1.f}, {0.5f, 0.5f, 0.5f}, 1, 1};
  } else {
    S.nlight = nlight;
    for (int i = 0; i < nlight; i++) {
      const dx_light& l = lights[i];
      if (!finite_all(l.pos, 3) || !finite_all(l.dir, 3) || !finite_all(l.diffuse, 3))
        return dx_fail(DX_EINVAL, "shading: a non-finite light");
      ShadeLight& o = S.light[i];
      o.directional = l.directional != 0;
      o.castshadow = l.castshadow != 0;
      for (int k = 0; k < 3; k++) o.diffuse[k] = l.diffuse[k];
      if (o.directional) {
        const double d[3] = {l.dir[0], l.dir[1], l.dir[2]};
        const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(n > 0.0)) return dx_fail(DX_EINVAL, "shading: a directional light with a zero dir");
        for (int k = 0; k < 3; k++) o.v[k] = (float)(-d[k] / n);
      } else {
        for (int k = 0; k < 3; k++) o.v[k] = l.pos[k];
      }
    }
  }
  if (!shading) {
    for (int k = 0; k < 3; k++) { S.ambient[k] = 0.2f; S.background[k] = 0.f; S.headlight[k] = 0.3f; }
  } else {
    if (!finite_all(shading->ambient, 3) || !finite_all(shading->background, 3) || !finite_all(shading->headlight, 3) ||
        !finite_all(&shading->checker_rgb[0][0], 6) || !finite_all(&shading->checker_cell, 1))
      return dx_fail(DX_EINVAL, "shading: a non-finite value");
    if (shading->checker_cell < 0.f) return dx_fail(DX_EINVAL, "shading: a negative checker_cell");
    for (int k = 0; k < 3; k++) {
      S.ambient[k] = shading->ambient[k]; S.background[k] = shading->background[k]; S.headlight[k] = shading->headlight[k];
      S.checker_rgb[0][k] = shading->checker_rgb[0][k]; S.checker_rgb[1][k] = shading->checker_rgb[1][k];
    }
    S.checker_cell = shading->checker_cell;
  }
  S.headlight_on = S.headlight[0] != 0.f || S.headlight[1] != 0.f || S.headlight[2] != 0.f;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));  // may be called between renders
  if (!b->shade_tab)
    if (int rc = balloc(b, (void**)&b->shade_tab, tab.size() * 4)) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));  // (balloc clears on the stream)
  HIPCHK(hipMemcpy(b->shade_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  b->shade = S;
  b->shade_set = true;
  return 0;
}

extern "C" int dx_render_get(dx_batch* b, int which, void* dst_host, int32_t env0, int32_t n) {
  void* src = nullptr;
  if (int rc = dx_render_output(b, which, &src)) return rc;
  if (!dst_host || env0 < 0 || n < 0 || env0 + n > b->nenv) return dx_fail(DX_EINVAL, "render: bad env range or null destination");
  HIPCHK(hipSetDevice(b->device));
  const size_t per = (size_t)b->RA.ncam * b->RA.H * b->RA.W * (which == DX_RENDER_RGB ? 3 : 4);
  HIPCHK(hipMemcpyAsync(dst_host, (const char*)src + per * env0, per * n, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" int dx_render_stats(dx_batch* b, int enable, uint64_t out[3]) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (!b->rnd_stats)
    if (int rc = balloc(b, (void**)&b->rnd_stats, 6 * 8)) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  if (out) HIPCHK(hipMemcpy(out, b->rnd_stats, 3 * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(b->rnd_stats, 0, 3 * 8));
  b->rnd_stats_on = enable != 0;
  return 0;
}

// the shadow cull's triple (words 3-5 of the same buffer; dx_render_stats switches the counting)
extern "C" int dx_render_stats2(dx_batch* b, uint64_t out[3]) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (!b->rnd_stats) return dx_fail(DX_EINVAL, "render: the statistics were never enabled (dx_render_stats)");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (out) HIPCHK(hipMemcpy(out, b->rnd_stats + 3, 3 * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(b->rnd_stats + 3, 0, 3 * 8));
  return 0;
}

extern "C" int dx_ray(dx_batch* b, const float* origin, const float* dir, int32_t nray, float* dist, int32_t* geom) {
  if (!b) return dx_fail(DX_EINVAL, "null batch");
  if (!origin || !dir || !dist || !geom) return dx_fail(DX_EINVAL, "ray: null origin, dir, dist or geom");
  if (nray < 1) return dx_fail(DX_EINVAL, "ray: nray must be positive");
  if ((unsigned long long)b->nenv * nray >= 0x80000000ull / 4) return dx_fail(DX_ELIMIT, "ray: nenv * nray reaches 2^29");
  HIPCHK(hipSetDevice(b->device));
  RenderArgs A{};
  if (int rc = render_base(b, A)) return rc;
  const size_t E = b->nenv;
  std::unique_ptr<CallScratch> S;  // (synchronises the stream when it goes)
  DlsArg ao, ad, at, ag;
  if (!dls_arg(ao, origin, E * nray * 12, S, b->stream) || !dls_arg(ad, dir, E * nray * 12, S, b->stream) ||
      !dls_arg(at, dist, E * nray * 4, S, b->stream) || !dls_arg(ag, geom, E * nray * 4, S, b->stream))
    return dx_fail(DX_ENOMEM, "device scratch allocation failed");
  if (ao.staged) HIPCHK(hipMemcpyAsync(ao.dev, ao.user, ao.bytes, hipMemcpyHostToDevice, b->stream));
  if (ad.staged) HIPCHK(hipMemcpyAsync(ad.dev, ad.user, ad.bytes, hipMemcpyHostToDevice, b->stream));
  A.nray = nray;
  A.ray_o = (const float*)ao.dev;
  A.ray_d = (const float*)ad.dev;
  A.ray_dist = (float*)at.dev;
  A.ray_geom = (int*)ag.dev;
  HIPCHK(dx_launch_rays(b->stream, A));
  if (at.staged) HIPCHK(hipMemcpyAsync(at.user, at.dev, at.bytes, hipMemcpyDeviceToHost, b->stream));
  if (ag.staged) HIPCHK(hipMemcpyAsync(ag.user, ag.dev, ag.bytes, hipMemcpyDeviceToHost, b->stream));
  if (S) HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}
