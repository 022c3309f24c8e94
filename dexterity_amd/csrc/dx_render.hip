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
//
// dx_shade_kernel (below, DX_RENDER_RGB) shades the cast's images in a second launch: normals,
// lights, shadows through the same entry tests, per-face colours, uint8 RGB.
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

// ---- the shading pass (DX_RENDER_RGB; the model is stated in include/dx.h "Shaded RGB") ----
// Launched behind dx_render_kernel with the same grid and the same lane-to-pixel map.  A lane
// reads its pixel's depth t and geom g from the cast's images and rebuilds the hit point the
// way the cast built the ray: in g's frame, p = o + t d with o and d from the camera moved
// into that frame.  The normal comes from p alone (per lane: every lane has its own geom, so
// the hull arg-max loads its planes per lane).
//  Shadow pass, once per shadow-casting light: the lanes that face the light reduce their hit
//   points to a bounding sphere (wave shuffles, then LDS).  Stage one culls one geom per lane
//   against that sphere swept towards the light -- along a ray for a directional light, along
//   the segment to a positional one: the distance of the geom's inflated bounding sphere to
//   the ray / segment against the summed radii, which keeps every geom a lane's own test could
//   accept -- and ballot-compacts the survivors into the LDS list, in geom order.  A record is
//   the cast's (the camera in the geom frame, so a lane's hit point there is o + t d again)
//   plus the light in the geom frame.  Stage two walks the list with a wave-uniform trip
//   count through the cast's own geom_entry: hull plane addresses stay wave-uniform.
//  Stores go through an LDS tile of bytes: a row's 16 pixels leave as 48 contiguous bytes in
//   whole dwords (single bytes only where an image row is not dword aligned at its ends).
// Exactness: as the cast's.  A lane's verdict is masked by its own gate and the cull is
// conservative, so the bytes are a function of (env, camera, pixel, settings) alone.
enum { SR_LIGHT = 24 };  // a shadow record's words beyond the cast's (DX_SHADE_REC = 28)

// the unit normal in the geom frame at the surface point p of geom g, and the box face
__device__ __forceinline__ void surface_normal(const RenderArgs& A, int g, int type, const float* p, float* n, int* face) {
  const float s0 = A.geom_size[3 * g], s1 = A.geom_size[3 * g + 1], s2 = A.geom_size[3 * g + 2];
  n[0] = 0.f; n[1] = 0.f; n[2] = 1.f;  // (the plane's)
  *face = 0;
  if (type == DXG_SPHERE) {
    const float inv = 1.0f / sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    n[0] = p[0] * inv; n[1] = p[1] * inv; n[2] = p[2] * inv;
  } else if (type == DXG_CAPSULE) {
    const float qz = p[2] - fminf(fmaxf(p[2], -s1), s1);
    const float inv = 1.0f / sqrtf(p[0] * p[0] + p[1] * p[1] + qz * qz);
    n[0] = p[0] * inv; n[1] = p[1] * inv; n[2] = qz * inv;
  } else if (type == DXG_BOX) {
    const float e0 = fabsf(p[0]) - s0, e1 = fabsf(p[1]) - s1, e2 = fabsf(p[2]) - s2;
    int k = e1 > e0 ? 1 : 0;
    k = e2 > fmaxf(e0, e1) ? 2 : k;
    const float pk = k == 0 ? p[0] : (k == 1 ? p[1] : p[2]);
    const float sg = pk < 0.f ? -1.f : 1.f;
    n[0] = k == 0 ? sg : 0.f; n[1] = k == 1 ? sg : 0.f; n[2] = k == 2 ? sg : 0.f;
    *face = 2 * k + (pk < 0.f ? 1 : 0);
  } else if (type == DXG_MESH) {
    const int mesh = A.geom_dataid[g];
    const int adr = mesh >= 0 ? A.mesh_planeadr[mesh] : 0, num = mesh >= 0 ? A.mesh_planenum[mesh] : 0;
    float bv = -RINF;
    for (int i = 0; i < num; i++) {  // (per-lane loads; straight-line selects)
      const float4 q = A.plane4[adr + i];
      const float v = q.x * p[0] + q.y * p[1] + q.z * p[2] + q.w;
      const bool up = v > bv;
      bv = up ? v : bv;
      n[0] = up ? q.x : n[0]; n[1] = up ? q.y : n[1]; n[2] = up ? q.z : n[2];
    }
  }
}

__device__ __forceinline__ float wave_min(float v) {
  for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

__device__ __forceinline__ int colour_byte(float c) {
  return (int)fminf(fmaxf(floorf(255.0f * c + 0.5f), 0.f), 255.f);
}

extern "C" __global__ void __launch_bounds__(DX_RENDER_THREADS) dx_shade_kernel(ShadeArgs SA) {
  __shared__ float rec[DX_RENDER_CHUNK * DX_SHADE_REC];
  __shared__ int wcnt[DX_RENDER_THREADS / 64];
  __shared__ float wbox[DX_RENDER_THREADS / 64][6];
  __shared__ unsigned char trgb[DX_RENDER_TILE * DX_RENDER_TILE * 3];
  const RenderArgs& A = SA.R;
  const ShadeSet& S = SA.S;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ntile = A.tiles_x * A.tiles_y;
  const int tile = blockIdx.x % ntile, ec = blockIdx.x / ntile;
  const int cam = ec % A.ncam, env = ec / A.ncam;
  const int tx0 = (tile % A.tiles_x) * DX_RENDER_TILE, ty0 = (tile / A.tiles_x) * DX_RENDER_TILE;
  const RenderCam& C = A.cam[cam];

  // the camera in the world (workgroup-uniform), as the cast builds it
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
  const int lx = (w & 1) * 8 + (lane & 7), ly = (w >> 1) * 8 + (lane >> 3);
  const int px = tx0 + lx, py = ty0 + ly;
  const float u = ((float)px + 0.5f - hw) * inv_f, v = ((float)py + 0.5f - hh) * inv_f;
  const bool wave_on = tx0 + (w & 1) * 8 < A.W && ty0 + (w >> 1) * 8 < A.H;
  const bool in_img = px < A.W && py < A.H;

  // the cast's answer for this pixel
  int g = -1;
  float t = 0.f;
  if (in_img) {
    const size_t at = (((size_t)env * A.ncam + cam) * A.H + py) * A.W + px;
    g = A.seg[at];
    t = A.depth[at];
  }
  const bool hit = g >= 0 && g < A.ngeom;
  const int gi = hit ? g : 0;
  const int type = A.geom_type[gi];

  // the hit point in the geom frame, the normal there, both in the world
  float p[3], nw[3], P[3];
  int face;
  {
    float gp[3], gR[9], ol[3], ax[3], ay[3], az[3], nl[3];
    geom_pose(A, env, gi, gp, gR);
    const float d0[3] = {co[0] - gp[0], co[1] - gp[1], co[2] - gp[2]};
    mattvec3(ol, gR, d0);
    mattvec3(ax, gR, cx);
    mattvec3(ay, gR, cy);
    mattvec3(az, gR, cz);
    for (int k = 0; k < 3; k++) p[k] = ol[k] + t * (ax[k] * u - ay[k] * v - az[k]);
    surface_normal(A, gi, type, p, nl, &face);
    matvec3(nw, gR, nl);
    for (int k = 0; k < 3; k++) P[k] = co[k] + t * (cx[k] * u - cy[k] * v - cz[k]);
  }

  // irradiance: ambient, the headlight (along the camera's +z, no shadow), the lights
  float E[3] = {S.ambient[0], S.ambient[1], S.ambient[2]};
  if (S.headlight_on) {
    const float ndl = fmaxf(nw[0] * cz[0] + nw[1] * cz[1] + nw[2] * cz[2], 0.f);
    for (int k = 0; k < 3; k++) E[k] += S.headlight[k] * ndl;
  }
  int survivors = 0, passes = 0;
  for (int li = 0; li < S.nlight; li++) {
    const ShadeLight& L = S.light[li];
    float lw[3] = {L.v[0], L.v[1], L.v[2]};
    if (!L.directional) {
      const float dv[3] = {L.v[0] - P[0], L.v[1] - P[1], L.v[2] - P[2]};
      const float inv = 1.0f / sqrtf(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
      lw[0] = dv[0] * inv; lw[1] = dv[1] * inv; lw[2] = dv[2] * inv;
    }
    const float ndl = nw[0] * lw[0] + nw[1] * lw[1] + nw[2] * lw[2];
    bool occl = false;
    if (L.castshadow) {  // (workgroup-uniform)
      const bool need = hit && ndl > 0.f;
      // the bounding box of the hit points that face the light
      float lo[3], hi[3];
      for (int k = 0; k < 3; k++) {
        lo[k] = wave_min(need ? P[k] : RINF);
        hi[k] = wave_max(need ? P[k] : -RINF);
      }
      if (lane == 0)
        for (int k = 0; k < 3; k++) { wbox[w][k] = lo[k]; wbox[w][3 + k] = hi[k]; }
      __syncthreads();
      for (int k = 0; k < 3; k++) {
        lo[k] = fminf(fminf(wbox[0][k], wbox[1][k]), fminf(wbox[2][k], wbox[3][k]));
        hi[k] = fmaxf(fmaxf(wbox[0][3 + k], wbox[1][3 + k]), fmaxf(wbox[2][3 + k], wbox[3][3 + k]));
      }
      __syncthreads();  // wbox is the next light's too
      if (lo[0] <= hi[0]) {  // some lane needs a verdict (workgroup-uniform)
        passes++;
        const float bcn[3] = {0.5f * (lo[0] + hi[0]), 0.5f * (lo[1] + hi[1]), 0.5f * (lo[2] + hi[2])};
        const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
        const float Rt = 0.5f * sqrtf(ex * ex + ey * ey + ez * ez) * 1.001f + 1e-5f;
        // the sweep's far end relative to the sphere's centre (positional), its length
        const float sv[3] = {L.v[0] - bcn[0], L.v[1] - bcn[1], L.v[2] - bcn[2]};
        const float sl2 = sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2];
        for (int base = 0; base < A.ngeom; base += DX_RENDER_CHUNK) {
          // stage one
          const int gg = base + tid;
          bool keep = false;
          int gtype = -1;
          float gp[3], gR[9];
          if (gg < A.ngeom) {
            gtype = A.geom_type[gg];
            geom_pose(A, env, gg, gp, gR);
            keep = true;
            if (!A.no_cull && gtype != DXG_PLANE) {
              const float bc[3] = {A.geom_bsphere[4 * gg], A.geom_bsphere[4 * gg + 1], A.geom_bsphere[4 * gg + 2]};
              float tb[3];
              matvec3(tb, gR, bc);
              const float vx = gp[0] + tb[0] - bcn[0], vy = gp[1] + tb[1] - bcn[1], vz = gp[2] + tb[2] - bcn[2];
              const float v2 = vx * vx + vy * vy + vz * vz;
              // the parameter of the closest point of the ray (tau >= 0) / segment (0..1)
              float s;
              if (L.directional)
                s = fmaxf(vx * lw[0] + vy * lw[1] + vz * lw[2], 0.f);
              else
                s = sl2 > 0.f ? fminf(fmaxf((vx * sv[0] + vy * sv[1] + vz * sv[2]) / sl2, 0.f), 1.f) : 0.f;
              const float ax_[3] = {L.directional ? lw[0] : sv[0], L.directional ? lw[1] : sv[1], L.directional ? lw[2] : sv[2]};
              const float qx = vx - s * ax_[0], qy = vy - s * ax_[1], qz = vz - s * ax_[2];
              const float dist = sqrtf(qx * qx + qy * qy + qz * qz);
              const float rc = A.geom_bsphere[4 * gg + 3] * 1.002f + 2e-4f + 1e-5f * sqrtf(v2);
              keep = dist <= Rt + rc;
            }
          }
          int total;
          const int slot = compact(keep, wcnt, &total);
          if (keep) {
            float* r = rec + slot * DX_SHADE_REC;
            record_head(A, gg, gtype, r);
            const float d0[3] = {co[0] - gp[0], co[1] - gp[1], co[2] - gp[2]};
            mattvec3(r + RR_FRAME, gR, d0);
            mattvec3(r + RR_FRAME + 3, gR, cx);
            mattvec3(r + RR_FRAME + 6, gR, cy);
            mattvec3(r + RR_FRAME + 9, gR, cz);
            // the light in the geom frame: its direction, or its position
            const float lv[3] = {L.directional ? L.v[0] : L.v[0] - gp[0], L.directional ? L.v[1] : L.v[1] - gp[1],
                                 L.directional ? L.v[2] : L.v[2] - gp[2]};
            mattvec3(r + SR_LIGHT, gR, lv);
            r[SR_LIGHT + 3] = 0.f;
          }
          __syncthreads();
          survivors += total;
          // stage two
          if (wave_on) {
            const float tmax = L.directional ? RINF : 1.0f;  // (a positional light's ray is not normalised)
            for (int k = 0; k < total; k++) {
              const float* r = rec + k * DX_SHADE_REC;
              const float* F = r + RR_FRAME;
              const float o[3] = {F[0] + t * (F[3] * u - F[6] * v - F[9]), F[1] + t * (F[4] * u - F[7] * v - F[10]),
                                  F[2] + t * (F[5] * u - F[8] * v - F[11])};
              const float d[3] = {L.directional ? r[SR_LIGHT] : r[SR_LIGHT] - o[0],
                                  L.directional ? r[SR_LIGHT + 1] : r[SR_LIGHT + 1] - o[1],
                                  L.directional ? r[SR_LIGHT + 2] : r[SR_LIGHT + 2] - o[2]};
              const float tau = geom_entry(r, o, d, A);
              occl = occl || (need && rec_int(r, RR_GEOM) != g && tau > 0.f && tau < tmax);
            }
          }
          __syncthreads();  // the list and wcnt are reused
        }
      }
    }
    const bool lit = ndl > 0.f && !occl;
    for (int k = 0; k < 3; k++) E[k] += lit ? L.diffuse[k] * ndl : 0.f;
  }

  // albedo: the geom's colour, a registered box's face colour, the plane's checker
  float alb[3] = {SA.geom_rgb[3 * gi], SA.geom_rgb[3 * gi + 1], SA.geom_rgb[3 * gi + 2]};
  if (type == DXG_BOX) {
    const float* faces = SA.geom_rgb + 3 * (size_t)A.ngeom;
    for (int k = 0; k < S.nface; k++)
      if (S.face_geom[k] == g)
        for (int c = 0; c < 3; c++) alb[c] = faces[(k * 6 + face) * 3 + c];
  }
  if (type == DXG_PLANE && S.checker_cell > 0.f) {
    const int par = ((int)floorf(p[0] / S.checker_cell) + (int)floorf(p[1] / S.checker_cell)) & 1;
    for (int c = 0; c < 3; c++) alb[c] = S.checker_rgb[par][c];
  }
  for (int c = 0; c < 3; c++)
    trgb[(ly * DX_RENDER_TILE + lx) * 3 + c] =
        (unsigned char)colour_byte(hit ? alb[c] * fminf(1.0f, E[c]) : S.background[c]);
  __syncthreads();

  // a row segment of the tile is up to 48 contiguous bytes of the image: whole dwords where
  // the image's own alignment allows, single bytes at a segment's unaligned ends
  {
    const int row = tid / 13, j = tid % 13, y = ty0 + row;
    if (row < DX_RENDER_TILE && y < A.H) {
      const size_t start = ((((size_t)env * A.ncam + cam) * A.H + y) * A.W + tx0) * 3;
      const size_t end = start + (size_t)min(DX_RENDER_TILE, A.W - tx0) * 3;
      const size_t a = (start & ~(size_t)3) + 4 * (size_t)j;
      const unsigned char* src = trgb + row * DX_RENDER_TILE * 3;
      if (a >= start && a + 4 <= end) {
        const size_t i = a - start;
        const unsigned val = (unsigned)src[i] | ((unsigned)src[i + 1] << 8) | ((unsigned)src[i + 2] << 16) | ((unsigned)src[i + 3] << 24);
        *reinterpret_cast<unsigned*>(SA.rgb + a) = val;
      } else {
        for (int q = 0; q < 4; q++)
          if (a + q >= start && a + q < end) SA.rgb[a + q] = src[a + q - start];
      }
    }
  }
  if (SA.stats && tid == 0 && passes) {
    atomicAdd(SA.stats, (unsigned long long)survivors);
    atomicMax(SA.stats + 1, (unsigned long long)survivors);
    atomicAdd(SA.stats + 2, (unsigned long long)passes);
  }
}

hipError_t dx_launch_shade(hipStream_t stream, const ShadeArgs& A) {
  const size_t grid = (size_t)A.R.nenv * A.R.ncam * A.R.tiles_x * A.R.tiles_y;
  hipLaunchKernelGGL(dx_shade_kernel, dim3((unsigned)grid), dim3(DX_RENDER_THREADS), 0, stream, A);
  return hipGetLastError();
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
