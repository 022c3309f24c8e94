// dx_jac.h -- world positions and Jacobian rows of points fixed to bodies, shared by the
// IK kernel (dx_ik.hip: fingertip sites) and the Cartesian velocity mapper (dx_dls.hip:
// bodies, geoms and sites, resolved on the host to points).
//
// A point is (body id, offset in the body frame).  The accessor P supplies both:
//   int P.body(s)   the body of point s
//   P.off(s)        pointer to its 3 offset components (any address space)
// so the site path keeps reading the model's own site_bodyid / site_pos arrays, with the
// arithmetic the IK kernel has always run, and the mapper reads its launch parameters.
#pragma once
#include "dx_device.h"

// the model's sites, selected by an id list (device memory)
struct SitePoints {
  const DevModel& m;
  const int* sites;
  __device__ __forceinline__ int body(int s) const { return m.site_bodyid[sites[s]]; }
  __device__ __forceinline__ const DXG float* off(int s) const { return m.site_pos + 3 * sites[s]; }
};

// lane t < 3 * npoint: coordinate t % 3 of point t / 3 at the current kinematics
// (site_xpos / geom_xpos / xpos of the object the point stands for)
template <class Ctx, class Pts>
__device__ __forceinline__ void points_to_lds(const Ctx& c, const Pts& P, int npoint, float* pt) {
  if (LANE < 3 * npoint) {
    const int s = LANE / 3, e = LANE - 3 * s;
    const int b = P.body(s);
    const float* xp = c.f(c.L.xpos) + 3 * b;
    const float* xm = c.f(c.L.xmat) + 9 * b;
    const auto sp = P.off(s);
    pt[LANE] = xp[e] + xm[3 * e] * sp[0] + xm[3 * e + 1] * sp[1] + xm[3 * e + 2] * sp[2];
  }
  SYNC();
}

// mj_jac rows [3 * npoint][nv] at the points pt: translational (rot = false) or
// rotational.  Column d of a point on body b is non-zero when dof d is on b's path to
// the root; then jacp = cdof_lin + cdof_ang x (point - subtree_com[root]), jacr = cdof_ang.
template <class Ctx, class Pts>
__device__ __forceinline__ void point_jacobian(const Ctx& c, const Pts& P, int npoint, const float* pt, float* J,
                                               bool rot) {
  const DevModel& m = c.mdl();
  const int nv = c.nv, n = 3 * npoint * nv;
  const float* cdof = c.f(c.L.cdof);
  const float* rcom = c.f(c.L.rcom);
  for (int k = LANE; k < n; k += DX_WAVE) {
    const int r = k / nv, d = k - r * nv, s = r / 3, e = r - 3 * s;
    const int b = P.body(s);
    float v = 0.f;
    if ((m.body_chain[b] >> d) & 1ull) {
      const float* cd = cdof + 6 * d;
      if (rot) {
        v = cd[e];
      } else {
        const float* rc = rcom + 3 * m.body_rootidx[b];
        const float o0 = pt[3 * s] - rc[0], o1 = pt[3 * s + 1] - rc[1], o2 = pt[3 * s + 2] - rc[2];
        const float cr = e == 0 ? cd[1] * o2 - cd[2] * o1 : e == 1 ? cd[2] * o0 - cd[0] * o2 : cd[0] * o1 - cd[1] * o0;
        v = cd[3 + e] + cr;
      }
    }
    J[k] = v;
  }
  SYNC();
}
