// dx_observe.hip -- the optional hand observables (include/dx.h dx_env_set_hand_observables)
// for CDNA4: the observables of the reference's hand entity that the fixed observation
// does not carry (dexterous_hand.py:245-372), as one gather behind the step.
//
// Every input is already in the batch arrays when a control step's last launch is queued:
// the observation pass of all three contact tiers writes DX_SITE_XPOS / DX_SITE_VEL, and
// (DevBatch::out_bodies, which the setter switches on) DX_XPOS / DX_XQUAT.  The kernel
// reads those and a few model tables and writes [nenv][dim] floats; the step kernels know
// nothing of it.
//
// Layout: one lane per OUTPUT ELEMENT, DX_HOBS_THREADS elements per workgroup, elements in
// the buffer's own order -- a workgroup covers 256 / dim envs (1.7 - 7 at 37 - 148 floats),
// no lane idles but the last workgroup's tail, and a wave's stores are 256 contiguous
// bytes.  The lanes of one quaternion (4) or one ego position (3) repeat its arithmetic;
// their loads are the same few cache lines, and the whole launch moves under 1 KB per env:
// its cost is the launch, not the work.  No LDS.
//
// An element's value does not depend on which other observables are enabled (the mask
// only places it), so a subset's row equals the matching columns of the full row bit for
// bit.
#include "../../include/dx.h"
#include "dx_device.h"

// Element r of hand h's block in env's row.
__device__ __forceinline__ float hand_obs_element(const HandObs& H, int env, int h, int r) {
  // joint_positions (dexterous_hand.py:250-252): qpos at the hand's joints
  if (H.mask & DX_HOBS_JOINT_POSITIONS) {
    if (r < H.hand_nq) return H.qpos[(size_t)env * H.nq + h * H.hand_nq + r];
    r -= H.hand_nq;
  }
  // fingertip_orientations (:286-295): mat_to_quat(site_xmat) [3P], canonical with w >= 0.
  // site_xmat = xmat[body] * site_mat, so its quaternion is xquat[body] (x) site_quat up
  // to sign; normalised, and negated when w < 0 (-0 stays: it compares >= 0).
  if (H.mask & DX_HOBS_TIP_ORIENTATIONS) {
    if (r < 4 * H.ntips) {
      const int tip = h * H.ntips + (r >> 2), k = r & 3;
      const int b = H.site_bodyid[H.tip_site[tip]];
      const float* bq = H.xquat + ((size_t)env * H.nbody + b) * 4;
      const float* sq = H.tip_quat + 4 * tip;
      const float a[4] = {bq[0], bq[1], bq[2], bq[3]}, s[4] = {sq[0], sq[1], sq[2], sq[3]};
      float q[4];
      quatmul(q, a, s);
      quatnorm(q);
      const float v = k == 0 ? q[0] : k == 1 ? q[1] : k == 2 ? q[2] : q[3];
      return q[0] < 0.f ? -v : v;
    }
    r -= 4 * H.ntips;
  }
  // fingertip_angular_velocities (:312-325, utils/mujoco_utils.py:10-35): the world-frame
  // angular part of mj_objectVelocity at the site, words 3-5 of DX_SITE_VEL
  if (H.mask & DX_HOBS_TIP_ANGULAR_VELOCITIES) {
    if (r < 3 * H.ntips) {
      const int tip = h * H.ntips + r / 3, k = r % 3;
      return H.site_vel[((size_t)env * H.nsite + H.tip_site[tip]) * 6 + 3 + k];
    }
    r -= 3 * H.ntips;
  }
  // fingertip_positions_ego (:327-350): framepos of the site in the root body's frame,
  // which for reftype="body" is the body's INERTIAL frame [3P]:
  // ximat^T (site_xpos - xipos), xipos = xpos + xmat ipos, ximat = xmat imat
  {
    const int tip = h * H.ntips + r / 3, k = r % 3;
    const int rb = h ? H.root[1] : H.root[0];
    const float* xq = H.xquat + ((size_t)env * H.nbody + rb) * 4;
    const float* xp = H.xpos + ((size_t)env * H.nbody + rb) * 3;
    const float* sp = H.site_xpos + ((size_t)env * H.nsite + H.tip_site[tip]) * 3;
    const float* ip = H.body_ipos + 3 * rb;
    const float* im = H.body_imat + 9 * rb;
    const float q[4] = {xq[0], xq[1], xq[2], xq[3]}, ipos[3] = {ip[0], ip[1], ip[2]};
    float R[9], t[3], d[3], u[3];
    quat2mat(R, q);
    matvec3(t, R, ipos);
    d[0] = sp[0] - (xp[0] + t[0]); d[1] = sp[1] - (xp[1] + t[1]); d[2] = sp[2] - (xp[2] + t[2]);
    mattvec3(u, R, d);  // into the body frame
    return im[k] * u[0] + im[3 + k] * u[1] + im[6 + k] * u[2];  // row k of imat^T
  }
}

extern "C" __global__ void __launch_bounds__(DX_HOBS_THREADS) dx_hand_obs_kernel(HandObs H) {
  const unsigned t = blockIdx.x * DX_HOBS_THREADS + threadIdx.x;
  if (t >= (unsigned)H.nenv * (unsigned)H.dim) return;  // (nenv * dim < 2^31: checked by the setter)
  const int env = (int)(t / (unsigned)H.dim);
  const int k = (int)t - env * H.dim;
  const int h = k >= H.hand_dim ? 1 : 0;  // nhands <= DX_HOBS_MAX_HANDS = 2
  H.out[t] = hand_obs_element(H, env, h, k - h * H.hand_dim);
}

hipError_t dx_launch_hand_obs(hipStream_t stream, const HandObs& H) {
  const size_t n = (size_t)H.nenv * H.dim;
  hipLaunchKernelGGL(dx_hand_obs_kernel, dim3((unsigned)((n + DX_HOBS_THREADS - 1) / DX_HOBS_THREADS)),
                     dim3(DX_HOBS_THREADS), 0, stream, H);
  return hipGetLastError();
}
