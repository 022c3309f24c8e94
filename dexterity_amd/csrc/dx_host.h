// dx_host.h -- what the host units of include/dx.h's implementation share: dx_model.hip
// (the model compiler, no HIP runtime call), dx_batch.hip, dx_query.hip, dx_api.hip (the env)
// and dx_comm.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dx.h"
#include "dx_internal.h"

// sets the calling thread's dx_last_error text and returns `code` (dx_model.hip)
int dx_fail(int code, const std::string& msg);
#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) return dx_fail(DX_EHIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

struct BlobArr { int dtype; long n; const void* p; };  // an array of the blob: 0 int32 / 1 float64

struct dx_model {
  std::vector<unsigned char> blob;
  std::map<std::string, BlobArr> arr;
  // host copies (fp32 / int) of every device array, keyed by name
  std::map<std::string, std::vector<float>> hf;
  std::map<std::string, std::vector<int>> hi;
  std::vector<uint64_t> body_chain;
  DevModel dm;  // host-side scalars; pointers filled per device
  std::map<int, std::vector<void*>> dev_allocs;
  std::map<int, DevModel> dev_models;
  std::map<int, const DevModel*> dev_model_ptrs;  // device copy of dev_models[device]
  Lds lds;     // the step kernel's per-env LDS layout (contact pool DX_NCON_MAX)
  Lds lds_hi;  // the overflow tier's (DX_NCON_HI)
  Lds lds_mid; // the mid tier's (DX_NCON_MID; nefc_max 0: not available for this model)
  int ncon_max, nefc_max;
  // hull face planes (dx_model.hip hull_planes), derived when cameras or rays are first used:
  // plane4 [nplane][4] = (n, d) with n x + d <= 0 inside, hull k's run at planeadr[k],
  // planenum[k]; render_dev: their device copies per device
  bool planes_built = false;
  std::vector<float> plane4;
  std::vector<int> planeadr, planenum;
  struct RenderDev { const float4* plane4; const int *planeadr, *planenum; };
  std::map<int, RenderDev> render_dev;
};

struct dx_batch {
  dx_model* model;
  int device, nenv;
  hipStream_t stream;
  DevModel dm;
  const DevModel* dm_dev;  // the same struct in device memory (kernels read it through this)
  DevBatch db;
  int spec;  // specialized step kernel (dx_specs.inc) or -1 for the generic one
  bool queue;  // mode-0 steps through the substep queue
  bool qhead_zero = false;  // the last kernel on the stream zeroed the queue heads
  int* watch_list = nullptr;  // device copy of DevBatch::watch_pairs
  int slots;   // persistent workgroups of a queued launch
  int hi_grid; // workgroups of the overflow tier's launch
  float* xfrc;
  float* xfrc_env = nullptr;  // [nenv][nbody][6], allocated by the first dx_set_xfrc_env
  std::vector<void*> allocs;
  bool debug;
  float* sensor = nullptr;  // DX_SENSOR_TORQUE [nenv][nbody][3] (allocated by dx_sensor_enable)
  float* sen_stash = nullptr;
  // who reads the stash (DevBatch::sen_stash is set while any does): the torque sensors,
  // contact sensing (dx_contact_enable), the contact forces of a dx_env
  enum { STASH_TORQUE = 1, STASH_CONTACT = 2, STASH_ENV = 4 };
  int stash_users = 0;
  // contact sensing: DX_CFRC_EXT [nenv][nbody][6], DX_PAD_FORCE [nenv][npad][3] (allocated
  // for DX_MAX_PADS), the pad table on the device
  float* cfrc_ext = nullptr;
  float* pad_force = nullptr;
  int* pads = nullptr;
  int npad = 0;
  unsigned* ncon_hist = nullptr;  // dx_ncon_histogram
  // the mid tier beside queued launches (dx_step.hip dx_step_mid_kernel): its stream, the
  // queued workgroups' exit count it waits for (DevBatch::qdone[0])
  bool mid = false;
  hipStream_t side = nullptr;
  unsigned qdone_target = 0;
  // cameras (dx_render_set_cameras): off while RA.ncam == 0; the images are the batch's,
  // grown when a configuration needs more (rnd_cap pixels each); rnd_prev_bodies is the
  // body-pose setting from before the cameras switched it on (-1: not switched)
  RenderArgs RA{};
  int rnd_flags = 0;
  float* rnd_depth = nullptr;
  int* rnd_seg = nullptr;
  size_t rnd_depth_cap = 0, rnd_seg_cap = 0;
  int rnd_prev_bodies = -1;
  unsigned long long* rnd_stats = nullptr;  // the cast's triple, then the shadow cull's
  bool rnd_stats_on = false;
  // shaded RGB (DX_RENDER_RGB): RA.depth / RA.seg are then always set -- the cast writes them
  // for the shading pass -- and rnd_flags says which of them the caller asked for.  The
  // settings (dx_render_set_shading) persist across camera configurations; shade_tab is
  // [ngeom][3] geom colours followed by the face colours, allocated by the first use.
  unsigned char* rnd_rgb = nullptr;
  size_t rnd_rgb_cap = 0;  // in words
  ShadeSet shade{};
  bool shade_set = false;  // (false: the documented defaults, filled in at first use)
  float* shade_tab = nullptr;
};

// Per-call device scratch, released (after the batch stream drains) on every exit path.
struct CallScratch {
  hipStream_t s;
  std::vector<void*> p;
  explicit CallScratch(hipStream_t s_) : s(s_) {}
  ~CallScratch() {
    (void)hipStreamSynchronize(s);
    for (void* q : p) (void)hipFree(q);
  }
  void* get(size_t bytes) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(bytes, 4)) != hipSuccess) return nullptr;
    p.push_back(q);
    return q;
  }
};

struct dx_env {
  dx_batch* batch;
  TaskParams P;
  TaskState S;
  int nsub;
  std::vector<void*> allocs;  // positional: [0] the action buffer, [1] the packed outputs
  // the action pipeline (dx_env_set_action_filter): off while F.flags == 0; its buffers
  // (F.mt != nullptr once allocated) are the batch's
  ActFilter F{};
  // the optional hand observables (dx_env_set_hand_observables): off while H.mask == 0;
  // the output and the fingertip tables are the batch's, sized for every observable of
  // every fingertip at the first call; hobs_prev_bodies is the batch's body-pose setting
  // from before orientations / ego positions switched it on (-1: not switched)
  HandObs H{};
  int hobs_prev_bodies = -1;
  // the observation pipeline (dx_env_set_obs_pipeline): off while O.on == 0; its buffers
  // are sized by the configuration, so they are the env's own (obs_pipe_free), allocated
  // by every accepted call and gone while the pipeline is off
  ObsPipe O{};
  // the contact forces (dx_env_set_contact_forces): the task's pads -- every hand body with
  // a collision pair against the prop body, in body order, the prop their partner (empty
  // for the reach tasks) --, their table on the device and the output (the batch's, from
  // the first enable on); off while cf_on is false
  std::vector<dx_contact_pad> cf_pads;
  ContactSense CF{};
  float* cf_out = nullptr;
  bool cf_on = false;
  // the random pushes (dx_env_set_perturbation): off while PT.nb == 0; the buffers
  // (PT.mt != nullptr once allocated, sized for DX_PERT_MAXB bodies) are the batch's;
  // pt_shared: the batch had a shared xfrc array when the feature went on (restored when
  // it goes off)
  Perturb PT{};
  bool pt_shared = false;
};

// cross-unit helpers of dx_model.hip (the first three) and dx_batch.hip
extern std::recursive_mutex g_render_mu;  // the plane table and its per-device copies
double dx_getd(const dx_model* m, const char* name, double def = 0);
int hull_planes(dx_model* m);
int balloc(dx_batch* b, void** p, size_t bytes);
int render_tables(dx_model* m, int device, dx_model::RenderDev* out);int queue_check(dx_batch* b);
int xfrc_env_mode(dx_batch* b);
int launch_sensor(dx_batch* b, const ContactSense* env_pads, float* env_out);
int launch_step(dx_batch* b, int nsub, int mode);
int stash_use(dx_batch* b, int who, bool on);
