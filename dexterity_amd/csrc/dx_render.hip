// dx_render.hip -- depth and segmentation cameras, and batched rays, by ray casting against
// the compiled geoms (include/dx.h dx_render_set_cameras / dx_render / dx_ray) for CDNA4.
//
// Every input is in the batch arrays once a control step's last launch (or dx_forward) is
// queued: DX_XPOS / DX_XQUAT (DevBatch::out_bodies, which the setter switches on), plus the
// model's geom tables and the hull face planes the library derives on the host
// (dx_model.hip hull_planes).  The step kernels know nothing of this kernel.
//
// Layout.  A workgroup of four waves renders one 16 x 16 pixel tile of one (env, camera);
// a wave's lanes are an 8 x 8 block of the tile, so the rays of a wave stay close and the
// geoms they can hit are few.
//  Stage one: one lane per geom (chunks of DX_RENDER_CHUNK = 256: bimanual has 410 geoms).
//    The lane builds the geom's world pose from its body's, and tests the geom's bounding
//    sphere against the tile's bounding cone (apex the camera, axis the tile centre's ray,
//    half angle that of the farthest corner pixel, widened; the sphere inflated: the cull
//    is conservative, it never removes a geom a pixel's own test would accept).  Survivors
//    are ballot-compacted, in geom order, into an LDS list.  A record carries the camera
//    origin and the three camera axes IN THE GEOM'S FRAME, so a pixel's local ray is one
//    linear combination of them -- no per-pixel rotation.
//  Stage two: every wave walks the list (a wave-uniform trip count, records read by LDS
//    broadcast).  Per record a per-pixel bounding-sphere test gates the geom's own test --
//    hull: a clip against its face planes, whose addresses are wave-uniform (scalar loads);
//    box: slabs; sphere, capsule: closed form; plane: one-sided.  The nearest entry depth in
//    [near, far] wins, the lower geom id on a tie (the list is in geom order).
//  Stores go through a 16 x 16 LDS tile so that 16 consecutive lanes write one row segment.
//
// Exactness.  A pixel's value is a function of (env, camera, pixel) alone: a record's
// contents do not depend on the tile or on the cull, a lane's verdict is masked by its own
// gate (never by the wave's), and the cull only drops geoms no pixel of the tile accepts.
// So DX_RENDER_NO_CULL, another tiling or other cameras beside this one give the same bits.
//
// dx_ray runs the same stage two over caller-given rays (one lane per ray, every geom in
// the list; a record then carries the geom's world pose and the lane rotates its own ray).
#include "../../include/dx.h"
#include "dx_device.h"

#define RINF 3.0e38f

// record words (DX_RENDER_REC = 24)
enum { RR_TYPE = 0, RR_GEOM = 1, RR_PADR = 2, RR_PNUM = 3, RR_SIZE = 4, RR_RG2 = 7, RR_BC = 8, RR_FRAME = 12 };
// Words 0-3 are integers and are only ever touched as integers, through an int view of the
// record: as float bit patterns small integers are denormals, which the build flushes.
__device__ __forceinline__ int rec_int(const float* rec, int k) { return reinterpret_cast<const int*>(rec)[k]; }
__device__ __forceinline__ void rec_set_int(float* rec, int k, int v) { reinterpret_cast<int*>(rec)[k] = v; }

// entry parameter of the line o + t d into the sphere of squared radius r2 about (0, 0, cz);
// RINF: the line misses it.  inv_a = 1 / d.d.  Through the closest approach, not the
// quadratic's c = o.o - r2, which cancels for a small sphere far away.
__device__ __forceinline__ float sphere_entry(const float* o, const float* d, float inv_a, float cz, float r2) {
  const float oz = o[2] - cz;
  const float tc = -(o[0] * d[0] + o[1] * d[1] + oz * d[2]) * inv_a;
  const float px = o[0] + tc * d[0], py = o[1] + tc * d[1], pz = oz + tc * d[2];
  const float perp2 = px * px + py * py + pz * pz;
  return perp2 <= r2 ? tc - sqrtf((r2 - perp2) * inv_a) : RINF;
}

// capsule along z (radius r, half length h): the union of the cylinder's side and the two
// cap spheres; the line's entry into a union is the least of the parts' entries
__device__ __forceinline__ float capsule_entry(const float* o, const float* d, float a, float inv_a, float r, float h) {
  const float r2 = r * r;
  float t = fminf(sphere_entry(o, d, inv_a, h, r2), sphere_entry(o, d, inv_a, -h, r2));
  const float a2 = d[0] * d[0] + d[1] * d[1];
  if (a2 > 1e-12f * a) {
    const float inv_a2 = 1.0f / a2;
    const float tc = -(o[0] * d[0] + o[1] * d[1]) * inv_a2;
    const float px = o[0] + tc * d[0], py = o[1] + tc * d[1];
    const float perp2 = px * px + py * py;
    if (perp2 <= r2) {
      const float ts = tc - sqrtf((r2 - perp2) * inv_a2);
      if (fabsf(o[2] + ts * d[2]) <= h) t = fminf(t, ts);
    }
  }
  return t;
}

__device__ __forceinline__ float box_entry(const float* o, const float* d, const float* s) {
  float tmin = -RINF, tmax = RINF;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (d[k] != 0.f) {
      const float inv = 1.0f / d[k];
      const float t1 = (-s[k] - o[k]) * inv, t2 = (s[k] - o[k]) * inv;
      tmin = fmaxf(tmin, fminf(t1, t2));
      tmax = fminf(tmax, fmaxf(t1, t2));
    } else if (fabsf(o[k]) > s[k]) {
      tmin = RINF;
    }
  }
  return tmin <= tmax ? tmin : RINF;
}

// clip against the hull's half-spaces n x + d <= 0; the plane addresses are wave-uniform
__device__ __forceinline__ float hull_entry(const float* o, const float* d, const DXG float4* pl, int n) {
  float tmin = -RINF, tmax = RINF;
  // Straight-line selects (no exec-mask blocks), the reciprocal by v_rcp (1 ulp); unrolled so
  // that a trip's scalar loads are issued together, one round trip to the cache instead of
  // four.  max / min are exact, so the order of the planes does not touch the result.
#pragma unroll 4
  for (int i = 0; i < n; i++) {
    const float4 p = pl[i];
    const float den = p.x * d[0] + p.y * d[1] + p.z * d[2];
    const float dist = p.x * o[0] + p.y * o[1] + p.z * o[2] + p.w;
    const float t = -dist * __builtin_amdgcn_rcpf(den);  // (inf or nan when den == 0: not selected)
    tmin = den < 0.f ? fmaxf(tmin, t) : tmin;
    tmax = den > 0.f ? fminf(tmax, t) : tmax;
    tmin = (den == 0.f && dist > 0.f) ? RINF : tmin;
  }
  // the chord must be longer than fp32 resolves at that depth (8 ulp): a hull thinner than
  // that along the ray -- the hand's meshes hold flat, 6e-8 m thick pieces -- is not seen,
  // from any side, rather than seen or not by rounding
  return tmax - tmin > 8.0f * 1.1920929e-7f * fmaxf(fabsf(tmin), fabsf(tmax)) ? tmin : RINF;
}

// one record against one local ray: the entry parameter, RINF for a miss.  `rec` is LDS,
// the same address in every lane.
__device__ __forceinline__ float geom_entry(const float* rec, const float* o, const float* d, const RenderArgs& A) {
  const int type = rec_int(rec, RR_TYPE);
  const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  if (type == DXG_PLANE) return (d[2] < 0.f && o[2] > 0.f) ? -o[2] / d[2] : RINF;
  const float inv_a = 1.0f / a;
  // the per-pixel gate: the line against the geom's (slightly inflated) bounding sphere
  const float oc[3] = {o[0] - rec[RR_BC], o[1] - rec[RR_BC + 1], o[2] - rec[RR_BC + 2]};
  const float tc = -(oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2]) * inv_a;
  const float px = oc[0] + tc * d[0], py = oc[1] + tc * d[1], pz = oc[2] + tc * d[2];
  const bool pass = px * px + py * py + pz * pz <= rec[RR_RG2];
  if (!__any(pass)) return RINF;
  float t;
  if (type == DXG_MESH)
    t = hull_entry(o, d, A.plane4 + rec_int(rec, RR_PADR), rec_int(rec, RR_PNUM));
  else if (type == DXG_BOX)
    t = box_entry(o, d, rec + RR_SIZE);
  else if (type == DXG_SPHERE)
    t = sphere_entry(o, d, inv_a, 0.f, rec[RR_SIZE] * rec[RR_SIZE]);
  else if (type == DXG_CAPSULE)
    t = capsule_entry(o, d, a, inv_a, rec[RR_SIZE], rec[RR_SIZE + 1]);
  else
    t = RINF;
  return pass ? t : RINF;
}

// world pose of geom g in env: p, R (row-major).  The world body's pose is the identity.
__device__ __forceinline__ void geom_pose(const RenderArgs& A, int env, int g, float* p, float* R) {
  const int b = A.geom_bodyid[g];
  float xp[3] = {0.f, 0.f, 0.f}, xq[4] = {1.f, 0.f, 0.f, 0.f};
  if (b > 0) {
    const float* bp = A.xpos + ((size_t)env * A.nbody + b) * 3;
    const float* bq = A.xquat + ((size_t)env * A.nbody + b) * 4;
    xp[0] = bp[0]; xp[1] = bp[1]; xp[2] = bp[2];
    xq[0] = bq[0]; xq[1] = bq[1]; xq[2] = bq[2]; xq[3] = bq[3];
  }
  float Rb[9], gm[9], gp[3], t[3];
  quat2mat(Rb, xq);
  for (int k = 0; k < 9; k++) gm[k] = A.geom_mat[9 * g + k];
  for (int k = 0; k < 3; k++) gp[k] = A.geom_pos[3 * g + k];
  matmul3(R, Rb, gm);
  matvec3(t, Rb, gp);
  p[0] = xp[0] + t[0]; p[1] = xp[1] + t[1]; p[2] = xp[2] + t[2];
}

// the part of a record that does not depend on the camera
__device__ __forceinline__ void record_head(const RenderArgs& A, int g, int type, float* rec) {
  rec_set_int(rec, RR_TYPE, type);
  rec_set_int(rec, RR_GEOM, g);
  const int mesh = A.geom_dataid[g];
  const bool hull = type == DXG_MESH && mesh >= 0;
  rec_set_int(rec, RR_PADR, hull ? A.mesh_planeadr[mesh] : 0);
  rec_set_int(rec, RR_PNUM, hull ? A.mesh_planenum[mesh] : 0);
  for (int k = 0; k < 3; k++) rec[RR_SIZE + k] = A.geom_size[3 * g + k];
  const float r = A.geom_bsphere[4 * g + 3], rg = r * 1.001f + 1e-5f;
  rec[RR_RG2] = rg * rg;
  for (int k = 0; k < 3; k++) rec[RR_BC + k] = A.geom_bsphere[4 * g + k];
  rec[11] = 0.f;
}

// Ballot compaction of the workgroup's `keep` lanes, in lane order: the lane's slot (valid
// when keep) and the total.  wcnt: LDS [4].  Two barriers.
__device__ __forceinline__ int compact(bool keep, int* wcnt, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[w] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
  for (int k = 0; k < DX_RENDER_THREADS / 64; k++) {
    const int c = wcnt[k];
    if (k < w) off += c;
    tot += c;
  }
  *total = tot;
  return off + __popcll(m & ((1ull << lane) - 1ull));
}

extern "C" __global__ void __launch_bounds__(DX_RENDER_THREADS) dx_render_kernel(RenderArgs A) {
  __shared__ float rec[DX_RENDER_CHUNK * DX_RENDER_REC];
  __shared__ int wcnt[DX_RENDER_THREADS / 64];
  __shared__ float tdepth[DX_RENDER_TILE * DX_RENDER_TILE];
  __shared__ int tseg[DX_RENDER_TILE * DX_RENDER_TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ntile = A.tiles_x * A.tiles_y;
  const int tile = blockIdx.x % ntile, ec = blockIdx.x / ntile;
  const int cam = ec % A.ncam, env = ec / A.ncam;
  const int tx0 = (tile % A.tiles_x) * DX_RENDER_TILE, ty0 = (tile / A.tiles_x) * DX_RENDER_TILE;
  const RenderCam& C = A.cam[cam];

  // the camera in the world (workgroup-uniform)
  float co[3], cx[3], cy[3], cz[3];
  {
    float xp[3] = {0.f, 0.f, 0.f}, xq[4] = {1.f, 0.f, 0.f, 0.f}, Rb[9], t[3];
    if (C.body > 0) {
      const float* bp = A.xpos + ((size_t)env * A.nbody + C.body) * 3;
      const float* bq = A.xquat + ((size_t)env * A.nbody + C.body) * 4;
      xp[0] = bp[0]; xp[1] = bp[1]; xp[2] = bp[2];
      xq[0] = bq[0]; xq[1] = bq[1]; xq[2] = bq[2]; xq[3] = bq[3];
    }
    quat2mat(Rb, xq);
    matvec3(t, Rb, C.pos);
    co[0] = xp[0] + t[0]; co[1] = xp[1] + t[1]; co[2] = xp[2] + t[2];
    matvec3(cx, Rb, C.x);
    matvec3(cy, Rb, C.y);
    matvec3(cz, Rb, C.z);
  }
  const float inv_f = 1.0f / C.f, hw = 0.5f * (float)A.W, hh = 0.5f * (float)A.H;

  // the tile's bounding cone: axis through the tile centre, half angle to the farthest
  // corner pixel centre, widened (cos lowered by 1e-5)
  float aw[3], cos_t, sin_t;
  bool cone = !A.no_cull;
  {
    const float u0 = ((float)tx0 + 0.5f - hw) * inv_f, u1 = ((float)(tx0 + DX_RENDER_TILE - 1) + 0.5f - hw) * inv_f;
    const float v0 = ((float)ty0 + 0.5f - hh) * inv_f, v1 = ((float)(ty0 + DX_RENDER_TILE - 1) + 0.5f - hh) * inv_f;
    const float uc = 0.5f * (u0 + u1), vc = 0.5f * (v0 + v1);
    const float nc = 1.0f / sqrtf(uc * uc + vc * vc + 1.0f);
    const float ac[3] = {uc * nc, -vc * nc, -nc};
    cos_t = 1.0f;
    const float us[2] = {u0, u1}, vs[2] = {v0, v1};
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 2; j++) {
        const float n = 1.0f / sqrtf(us[i] * us[i] + vs[j] * vs[j] + 1.0f);
        cos_t = fminf(cos_t, (us[i] * ac[0] - vs[j] * ac[1] - ac[2]) * n);
      }
    cos_t -= 1e-5f;
    if (cos_t < 0.05f) cone = false;  // (a cone near a half space: keep every geom)
    sin_t = sqrtf(fmaxf(1.0f - cos_t * cos_t, 0.f));
    for (int k = 0; k < 3; k++) aw[k] = cx[k] * ac[0] + cy[k] * ac[1] + cz[k] * ac[2];
  }

  // this lane's pixel: wave w is the 8 x 8 block (w & 1, w >> 1) of the tile
  const int lx = (w & 1) * 8 + (lane & 7), ly = (w >> 1) * 8 + (lane >> 3);
  const int px = tx0 + lx, py = ty0 + ly;
  const float u = ((float)px + 0.5f - hw) * inv_f, v = ((float)py + 0.5f - hh) * inv_f;
  // a wave whose block lies outside the image skips stage two (wave-uniform)
  const bool wave_on = tx0 + (w & 1) * 8 < A.W && ty0 + (w >> 1) * 8 < A.H;
  float best = RINF;
  int bestg = -1;
  int survivors = 0;

  for (int base = 0; base < A.ngeom; base += DX_RENDER_CHUNK) {
    // stage one
    const int g = base + tid;
    bool keep = false;
    int type = -1;
    float p[3], R[9];
    if (g < A.ngeom) {
      type = A.geom_type[g];
      geom_pose(A, env, g, p, R);
      keep = true;
      if (cone && type != DXG_PLANE) {
        const float bc[3] = {A.geom_bsphere[4 * g], A.geom_bsphere[4 * g + 1], A.geom_bsphere[4 * g + 2]};
        float t[3];
        matvec3(t, R, bc);
        const float vx = p[0] + t[0] - co[0], vy = p[1] + t[1] - co[1], vz = p[2] + t[2] - co[2];
        const float s = vx * aw[0] + vy * aw[1] + vz * aw[2];
        const float v2 = vx * vx + vy * vy + vz * vz;
        const float perp = sqrtf(fmaxf(v2 - s * s, 0.f));
        const float rc = A.geom_bsphere[4 * g + 3] * 1.002f + 2e-4f + 1e-5f * sqrtf(v2);
        keep = perp * cos_t - s * sin_t <= rc;
      }
    }
    int total;
    const int slot = compact(keep, wcnt, &total);
    if (keep) {
      float* r = rec + slot * DX_RENDER_REC;
      record_head(A, g, type, r);
      const float d0[3] = {co[0] - p[0], co[1] - p[1], co[2] - p[2]};
      mattvec3(r + RR_FRAME, R, d0);      // the camera origin in the geom frame
      mattvec3(r + RR_FRAME + 3, R, cx);  // and its axes
      mattvec3(r + RR_FRAME + 6, R, cy);
      mattvec3(r + RR_FRAME + 9, R, cz);
    }
    __syncthreads();
    survivors += total;
    // stage two
    if (wave_on) {
      for (int k = 0; k < total; k++) {
        const float* r = rec + k * DX_RENDER_REC;
        const float* F = r + RR_FRAME;
        const float d[3] = {F[3] * u - F[6] * v - F[9], F[4] * u - F[7] * v - F[10], F[5] * u - F[8] * v - F[11]};
        const float t = geom_entry(r, F, d, A);
        if (t >= C.near_ && t <= C.far_ && t < best) {
          best = t;
          bestg = rec_int(r, RR_GEOM);
        }
      }
    }
    __syncthreads();  // the list and wcnt are reused by the next chunk
  }

  // whole row segments of the tile: 16 consecutive lanes write 64 contiguous bytes
  tdepth[ly * DX_RENDER_TILE + lx] = bestg >= 0 ? best : C.far_;
  tseg[ly * DX_RENDER_TILE + lx] = bestg;
  __syncthreads();
  {
    const int row = tid >> 4, col = tid & 15;
    const int x = tx0 + col, y = ty0 + row;
    if (x < A.W && y < A.H) {
      const size_t at = (((size_t)env * A.ncam + cam) * A.H + y) * A.W + x;
      if (A.depth) A.depth[at] = tdepth[tid];
      if (A.seg) A.seg[at] = tseg[tid];
    }
  }
  if (A.stats && tid == 0) {
    atomicAdd(A.stats, (unsigned long long)survivors);
    atomicMax(A.stats + 1, (unsigned long long)survivors);
    atomicAdd(A.stats + 2, 1ull);
  }
}

// dx_ray: lane = ray, DX_RENDER_THREADS rays of one env per workgroup, every geom listed
extern "C" __global__ void __launch_bounds__(DX_RENDER_THREADS) dx_ray_kernel(RenderArgs A) {
  __shared__ float rec[DX_RENDER_CHUNK * DX_RENDER_REC];
  const int tid = threadIdx.x;
  const int nblk = (A.nray + DX_RENDER_THREADS - 1) / DX_RENDER_THREADS;
  const int env = blockIdx.x / nblk, ray = (blockIdx.x % nblk) * DX_RENDER_THREADS + tid;
  const bool on = ray < A.nray;
  float o[3] = {0.f, 0.f, 0.f}, dw[3] = {0.f, 0.f, 0.f};
  bool ok = false;
  if (on) {
    const size_t at = ((size_t)env * A.nray + ray) * 3;
    for (int k = 0; k < 3; k++) { o[k] = A.ray_o[at + k]; dw[k] = A.ray_d[at + k]; }
    const float n2 = dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2];
    ok = n2 > 0.f && n2 < RINF;
    const float inv = ok ? 1.0f / sqrtf(n2) : 0.f;
    for (int k = 0; k < 3; k++) dw[k] *= inv;
  }
  float best = RINF;
  int bestg = -1;
  for (int base = 0; base < A.ngeom; base += DX_RENDER_CHUNK) {
    const int g = base + tid;
    const int total = min(A.ngeom - base, DX_RENDER_CHUNK);
    if (g < A.ngeom) {
      float* r = rec + tid * DX_RENDER_REC;
      record_head(A, g, A.geom_type[g], r);
      geom_pose(A, env, g, r + RR_FRAME, r + RR_FRAME + 3);
    }
    __syncthreads();
    for (int k = 0; k < total; k++) {
      const float* r = rec + k * DX_RENDER_REC;
      const float* F = r + RR_FRAME;
      const float d0[3] = {o[0] - F[0], o[1] - F[1], o[2] - F[2]};
      float ol[3], dl[3];
      mattvec3(ol, F + 3, d0);
      mattvec3(dl, F + 3, dw);
      const float t = ok ? geom_entry(r, ol, dl, A) : RINF;
      if (t >= 0.f && t < best) {
        best = t;
        bestg = rec_int(r, RR_GEOM);
      }
    }
    __syncthreads();
  }
  if (on) {
    const size_t at = (size_t)env * A.nray + ray;
    A.ray_dist[at] = bestg >= 0 ? best : -1.0f;
    A.ray_geom[at] = bestg;
  }
}

hipError_t dx_launch_render(hipStream_t stream, const RenderArgs& A) {
  const size_t grid = (size_t)A.nenv * A.ncam * A.tiles_x * A.tiles_y;
  hipLaunchKernelGGL(dx_render_kernel, dim3((unsigned)grid), dim3(DX_RENDER_THREADS), 0, stream, A);
  return hipGetLastError();
}

hipError_t dx_launch_rays(hipStream_t stream, const RenderArgs& A) {
  const size_t grid = (size_t)A.nenv * ((A.nray + DX_RENDER_THREADS - 1) / DX_RENDER_THREADS);
  hipLaunchKernelGGL(dx_ray_kernel, dim3((unsigned)grid), dim3(DX_RENDER_THREADS), 0, stream, A);
  return hipGetLastError();
}
