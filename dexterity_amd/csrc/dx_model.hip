// dx_model.hip -- the model compiler of include/dx.h, host code only.
//
// dx_model_load parses the compiled-model blob (fp64 arrays from the build-time
// compiler), derives the tables the kernels index (tree levels, dof chain
// bitmasks, friction/limit row maps, dense fixed-tendon Jacobians) and converts to
// fp32; dx_batch.hip uploads it.  Nothing here calls the HIP runtime: this unit and a
// main link without a HIP library (tests/csrc/dx_model_dump.cpp).
#include "dx_host.h"

static thread_local std::string g_err;
int dx_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" const char* dx_last_error(void) { return g_err.c_str(); }
extern "C" int dx_abi_version(void) { return DX_ABI_VERSION; }

// ---- blob parsing ----
static bool parse_blob(const unsigned char* b, size_t nbytes, std::map<std::string, BlobArr>& out) {
  if (nbytes < 16 || memcmp(b, "DXMBLOB1", 8) != 0) return false;
  long n;
  memcpy(&n, b + 8, 8);
  if (n < 0 || 16 + n * 72 > (long)nbytes) return false;
  for (long i = 0; i < n; i++) {
    const unsigned char* e = b + 16 + i * 72;
    char name[49];
    memcpy(name, e, 48);
    name[48] = 0;
    int code;
    long cnt, off;
    memcpy(&code, e + 48, 4);
    memcpy(&cnt, e + 56, 8);
    memcpy(&off, e + 64, 8);
    size_t esz = code == 0 ? 4 : 8;
    if (off < 0 || cnt < 0 || (size_t)off + cnt * esz > nbytes) return false;
    out[name] = BlobArr{code, cnt, b + off};
  }
  return true;
}

static int geti(const dx_model* m, const char* name, int def = -1) {
  auto it = m->arr.find(name);
  if (it == m->arr.end() || it->second.dtype != 0 || it->second.n < 1) return def;
  return ((const int*)it->second.p)[0];
}
double dx_getd(const dx_model* m, const char* name, double def) {
  auto it = m->arr.find(name);
  if (it == m->arr.end() || it->second.dtype != 1 || it->second.n < 1) return def;
  return ((const double*)it->second.p)[0];
}
static bool load_f(dx_model* m, const char* name) {
  auto it = m->arr.find(name);
  if (it == m->arr.end() || it->second.dtype != 1) return false;
  const double* p = (const double*)it->second.p;
  m->hf[name].assign(p, p + it->second.n);
  return true;
}
static bool load_i(dx_model* m, const char* name) {
  auto it = m->arr.find(name);
  if (it == m->arr.end() || it->second.dtype != 0) return false;
  const int* p = (const int*)it->second.p;
  m->hi[name].assign(p, p + it->second.n);
  return true;
}
static void quat2mat_h(float* R, const float* q) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// ---- direction-binned hulls (support-point acceleration, exact) ----
// A hull with more than DX_HULL_K (8) vertices gets a cube map of n x n cells per face
// over the local direction sphere (cell rule: dx_step.hip hull_cell).  Each cell lists
// the vertices that can be a support point for some direction in the cell, sorted by
// vertex index.  A vertex is dropped only if a single other vertex beats it by more
// than 1e-5 R at all four corner directions of the (slightly enlarged) cell, hence at
// every direction of the cell: every maximiser -- ties included -- of every direction
// in the cell is kept, and the lowest-index maximiser over the cell's list is the
// vertex the full scan returns (the oracle's rule).
// Layout: one DX_HULL_K-slot block per cell (x, y, z, vertex index; index -1 pads) -- one
// 128-B line, read by a lane group in one memory round trip of one or two 16-B loads per
// lane.  A cell with more than K candidates (the faces of a hull with many coplanar
// vertices: all of them tie along the face normal) keeps candidates 0..K-2 in its block
// and a header in slot K-1 = (overflow offset in float4s from the hull's first cell,
// candidate count, 0, index -2); candidates K-1.. follow in the hull's overflow run,
// padded to a multiple of K.  n is the smallest of 1, 2, 3, 4, 6, 8, 10, 12 with at most
// 2 % of the cells overflowing.  (Round 6: 8-slot cells on finer maps instead of 16-slot
// cells -- half the loads and candidate tests per support, one line per cell.)
static void cell_corners(int face, int n, int iu, int iv, double eps, double c[4][3]) {
  int ax = face >> 1;
  double sgn = (face & 1) ? -1.0 : 1.0;
  double u0 = -1 + 2.0 * iu / n - eps, u1 = -1 + 2.0 * (iu + 1) / n + eps;
  double v0 = -1 + 2.0 * iv / n - eps, v1 = -1 + 2.0 * (iv + 1) / n + eps;
  double us[4] = {u0, u1, u1, u0}, vs[4] = {v0, v0, v1, v1};
  for (int k = 0; k < 4; k++) {
    c[k][ax] = sgn;
    c[k][(ax + 1) % 3] = us[k];
    c[k][(ax + 2) % 3] = vs[k];
  }
}

static void hull_cell_candidates(const std::vector<double>& V, int nv, double R, const double c[4][3],
                                 std::vector<int>& out) {
  std::vector<double> D(4 * nv), S(nv);
  for (int i = 0; i < nv; i++) {
    for (int k = 0; k < 4; k++)
      D[4 * i + k] = V[3 * i] * c[k][0] + V[3 * i + 1] * c[k][1] + V[3 * i + 2] * c[k][2];
    S[i] = D[4 * i] + D[4 * i + 1] + D[4 * i + 2] + D[4 * i + 3];
  }
  std::vector<int> order(nv);
  for (int i = 0; i < nv; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return S[a] > S[b]; });
  double cn[4];
  for (int k = 0; k < 4; k++) cn[k] = std::sqrt(c[k][0] * c[k][0] + c[k][1] * c[k][1] + c[k][2] * c[k][2]);
  const double tol = 1e-5 * R;
  out.clear();
  for (int v = 0; v < nv; v++) {
    bool dominated = false;
    for (int w : order) {
      if (S[w] <= S[v]) break;  // a dominator beats v at every corner, so also in the sum
      bool all = true;
      for (int k = 0; k < 4 && all; k++) all = D[4 * w + k] - D[4 * v + k] > tol * cn[k];
      if (all) { dominated = true; break; }
    }
    if (!dominated) out.push_back(v);
  }
}

static void build_hull_bins(dx_model* m) {
  auto& mv = m->hf["mesh_vert"];
  auto& adr = m->hi["mesh_vertadr"];
  auto& num = m->hi["mesh_vertnum"];
  int nmesh = (int)num.size();
  std::vector<int> bn(std::max(nmesh, 1), 0), bcap(std::max(nmesh, 1), 0), badr(std::max(nmesh, 1), 0);
  std::vector<float> b4;
  static const int kN[] = {1, 2, 3, 4, 6, 8, 10, 12};
  constexpr int K = DX_HULL_K;
  const char* env_minn = getenv("DX_HULL_BIN_MINN");  // (experiments: finer cube maps)
  const int minn = env_minn ? atoi(env_minn) : 1;
  for (int i = 0; i < nmesh; i++) {
    int nv = num[i];
    if (nv <= K) continue;
    std::vector<double> V(3 * nv);
    double R = 0;
    for (int j = 0; j < nv; j++) {
      for (int k = 0; k < 3; k++) V[3 * j + k] = mv[3 * (adr[i] + j) + k];
      R = std::max(R, std::sqrt(V[3 * j] * V[3 * j] + V[3 * j + 1] * V[3 * j + 1] + V[3 * j + 2] * V[3 * j + 2]));
    }
    std::vector<std::vector<int>> cells;
    int n = 0;
    for (int nn : kN) {
      if (nn < minn && nn != kN[7]) continue;
      cells.assign(6 * nn * nn, {});
      int over = 0;
      for (int f = 0; f < 6; f++)
        for (int iu = 0; iu < nn; iu++)
          for (int iv = 0; iv < nn; iv++) {
            double c[4][3];
            cell_corners(f, nn, iu, iv, 1e-3, c);
            auto& L = cells[(f * nn + iu) * nn + iv];
            hull_cell_candidates(V, nv, R, c, L);
            over += L.size() > K;
          }
      n = nn;
      if (over <= 0.02 * (double)cells.size()) break;
    }
    const size_t base = b4.size() / 4;  // this hull's first cell, in float4s
    const size_t ncell = cells.size();
    b4.resize(4 * (base + K * ncell), 0.f);
    auto put = [&](size_t slot, int idx) {
      float* e = b4.data() + 4 * slot;
      for (int k = 0; k < 3; k++) e[k] = idx >= 0 ? mv[3 * (adr[i] + idx) + k] : 0.f;
      memcpy(e + 3, &idx, 4);
    };
    for (size_t cidx = 0; cidx < ncell; cidx++) {
      const auto& L = cells[cidx];
      const size_t blk = base + K * cidx;
      if (L.size() <= (size_t)K) {
        for (int s = 0; s < K; s++) put(blk + s, s < (int)L.size() ? L[s] : -1);
        continue;
      }
      for (int s = 0; s < K - 1; s++) put(blk + s, L[s]);
      const size_t ov = b4.size() / 4;  // overflow run: candidates K-1.., padded to K
      const int nov = (int)L.size() - (K - 1);
      b4.resize(4 * (ov + (size_t)(nov + K - 1) / K * K), 0.f);
      for (int s = 0; s < (nov + K - 1) / K * K; s++) put(ov + s, s < nov ? L[K - 1 + s] : -1);
      float* h = b4.data() + 4 * (blk + K - 1);
      const int off = (int)(ov - base), cnt = (int)L.size(), tag = -2;
      memcpy(h, &off, 4);
      memcpy(h + 1, &cnt, 4);
      h[2] = 0.f;
      memcpy(h + 3, &tag, 4);
    }
    bn[i] = n;
    bcap[i] = K;
    badr[i] = (int)base;
  }
  if (b4.empty()) b4.assign(4, 0.f);
  m->hf["mesh_bin4"] = b4;
  m->hi["mesh_binn"] = bn;
  m->hi["mesh_bincap"] = bcap;
  m->hi["mesh_binadr"] = badr;
}

static const char* kFloatArrays[] = {
    "body_pos", "body_quat", "body_ipos", "body_iquat", "body_mass", "body_inertia", "body_bsphere",
    "body_invweight0", "jnt_pos", "jnt_axis", "jnt_range", "jnt_margin", "jnt_solref", "jnt_solimp",
    "qpos0", "dof_armature", "dof_damping", "dof_frictionloss", "dof_solref", "dof_solimp",
    "dof_invweight0", "geom_size", "geom_pos", "geom_quat", "geom_center", "geom_bsphere", "geom_aabb", "mesh_vert",
    "site_pos", "site_quat", "tendon_range", "tendon_margin", "tendon_solref", "tendon_solimp",
    "tendon_invweight0", "wrap_coef", "actuator_gear", "actuator_gainprm", "actuator_biasprm",
    "actuator_ctrlrange", "actuator_forcerange", "gpair_friction", "gpair_solref", "gpair_solimp",
    "gpair_margin", "gravity", "bpair_sphere"};
static const char* kIntArrays[] = {
    "body_parent", "body_rootid", "body_jntnum", "body_jntadr", "body_dofnum", "body_dofadr",
    "jnt_type", "jnt_bodyid", "jnt_qposadr", "jnt_dofadr", "jnt_limited", "dof_bodyid",
    "dof_parentid", "dof_jntid", "geom_type", "geom_bodyid", "geom_dataid", "mesh_vertadr",
    "mesh_vertnum", "site_bodyid", "tendon_adr", "tendon_num", "tendon_limited", "wrap_dof",
    "actuator_trntype", "actuator_trnid", "actuator_biastype", "actuator_ctrllimited",
    "actuator_forcelimited", "bpair_body", "bpair_adr", "bpair_num", "bpair_plane", "gpair_geom", "gpair_condim"};

// dx_model_load's steps.  Each reads tables of m->hf / m->hi (the blob's, or an earlier
// step's) and the scalars of m->dm, and writes the tables and scalars it names; one that
// can refuse the model returns its error code.  First the blob's arrays and scalars:
static int load_arrays(dx_model* m) {
  for (const char* n : kFloatArrays)
    if (!load_f(m, n)) return dx_fail(DX_EMODEL, std::string("blob missing float array ") + n);
  for (const char* n : kIntArrays)
    if (!load_i(m, n)) return dx_fail(DX_EMODEL, std::string("blob missing int array ") + n);
  DevModel& d = m->dm;
  memset(&d, 0, sizeof(d));
  d.nq = geti(m, "nq"); d.nv = geti(m, "nv"); d.nbody = geti(m, "nbody"); d.njnt = geti(m, "njnt");
  d.ngeom = geti(m, "ngeom"); d.nsite = geti(m, "nsite"); d.nu = geti(m, "nu");
  d.ntendon = geti(m, "ntendon"); d.nwrap = geti(m, "nwrap"); d.nbpair = geti(m, "nbpair");
  d.ngpair = geti(m, "ngpair"); d.iterations = geti(m, "iterations");
  d.disable_contact = geti(m, "disable_contact");
  d.solver = geti(m, "solver", 2);  // absent in every reference scene: MuJoCo's default, Newton
  if (d.solver < 0 || d.solver > 2) return dx_fail(DX_EMODEL, "unknown solver");
  d.timestep = (float)dx_getd(m, "timestep"); d.tolerance = (float)dx_getd(m, "tolerance");
  d.impratio = (float)dx_getd(m, "impratio"); d.meaninertia = (float)dx_getd(m, "meaninertia");
  for (int k = 0; k < 3; k++) d.gravity[k] = m->hf["gravity"][k];
  if (d.nv < 1 || d.nv > DX_MAX_NV || d.nbody < 1) return dx_fail(DX_ELIMIT, "nv must be in [1, 64]");
  // one lane per actuator / joint (velocity stage, Euler)
  if (d.nu > 64 || d.njnt > 64) return dx_fail(DX_ELIMIT, "nu and njnt must be <= 64");
  return 0;
}

// Roots and tree levels: body_rootidx, root_body, lvl_adr, lvl_body, nlevel, nroot; `depth`
// (a body's level) goes on to tree_records.
static void tree_levels(dx_model* m, std::vector<int>& depth) {
  DevModel& d = m->dm; const int nb = d.nbody;
  auto& parent = m->hi["body_parent"]; auto& rootid = m->hi["body_rootid"];
  std::vector<int> rootidx(nb, 0), roots;
  for (int b = 1; b < nb; b++) {
    if (parent[b] == 0) { rootidx[b] = (int)roots.size(); roots.push_back(b); }
  }
  for (int b = 1; b < nb; b++) rootidx[b] = rootidx[rootid[b]];
  depth.assign(nb, 0);
  int maxd = 0;
  for (int b = 1; b < nb; b++) { depth[b] = depth[parent[b]] + 1; maxd = std::max(maxd, depth[b]); }
  std::vector<int> lvl_adr(maxd + 1, 0), lvl_body;
  for (int lv = 1; lv <= maxd; lv++) {
    lvl_adr[lv - 1] = (int)lvl_body.size();
    for (int b = 1; b < nb; b++)
      if (depth[b] == lv) lvl_body.push_back(b);
  }
  lvl_adr[maxd] = (int)lvl_body.size();
  d.nlevel = maxd;
  d.nroot = (int)roots.size();
  m->hi["body_rootidx"] = rootidx;
  m->hi["root_body"] = roots.empty() ? std::vector<int>{0} : roots;
  m->hi["lvl_adr"] = lvl_adr;
  m->hi["lvl_body"] = lvl_body.empty() ? std::vector<int>{0} : lvl_body;
}

// Dof chain masks: body_chain, the dofs on the path body -> root.
static int dof_chains(dx_model* m) {
  const int nb = m->dm.nbody;
  auto& parent = m->hi["body_parent"]; auto& dofadr = m->hi["body_dofadr"]; auto& dofnum = m->hi["body_dofnum"];
  m->body_chain.assign(nb, 0);
  for (int b = 1; b < nb; b++) {
    uint64_t c = m->body_chain[parent[b]];
    for (int k = 0; k < dofnum[b]; k++) c |= 1ull << (dofadr[b] + k);
    m->body_chain[b] = c;
  }
  // check contact jacobian support limit over all candidate body pairs
  auto& bpair = m->hi["bpair_body"];
  for (int k = 0; k < m->dm.nbpair; k++) {
    uint64_t s = m->body_chain[bpair[2 * k]] ^ m->body_chain[bpair[2 * k + 1]];
    if (__builtin_popcountll(s) > DX_DOFMAX) return dx_fail(DX_ELIMIT, "contact jacobian support exceeds DX_DOFMAX");
  }
  return 0;
}

// Rotation matrices of the blob's quaternions (body_imat, geom_mat, site_mat) and mesh_vert4.
static void rotations_and_verts(dx_model* m) {
  const DevModel& d = m->dm;
  auto mats = [&](const char* qname, const char* out, int n) {
    std::vector<float> R(9 * std::max(n, 1), 0.f);
    auto& q = m->hf[qname];
    for (int i = 0; i < n; i++) quat2mat_h(R.data() + 9 * i, q.data() + 4 * i);
    m->hf[out] = R;
  };
  mats("body_iquat", "body_imat", d.nbody);
  mats("geom_quat", "geom_mat", d.ngeom);
  mats("site_quat", "site_mat", d.nsite);
  {
    // (x, y, z, the vertex's index in its mesh as int bits): a whole-hull scan reads the
    // index from the slot as a cell scan does, so every support load is one 16-B load
    auto& mv = m->hf["mesh_vert"];
    std::vector<float> v4(4 * std::max<size_t>(mv.size() / 3, 1), 0.f);
    for (size_t i = 0; i < mv.size() / 3; i++)
      for (int k = 0; k < 3; k++) v4[4 * i + k] = mv[3 * i + k];
    auto& vadr = m->hi["mesh_vertadr"]; auto& vnum = m->hi["mesh_vertnum"];
    for (size_t g = 0; g < vnum.size(); g++)
      for (int j = 0; j < vnum[g]; j++) memcpy(&v4[4 * ((size_t)vadr[g] + j) + 3], &j, 4);
    m->hf["mesh_vert4"] = v4;
  }
}

// geom_rec, gpair_rec: per-geom shape records and per-pair records for the narrowphase
// setup: one or two memory round trips instead of a chain of dependent table lookups
static void narrowphase_records(dx_model* m) {
  auto& gt = m->hi["geom_type"]; auto& gb = m->hi["geom_bodyid"]; auto& gdid = m->hi["geom_dataid"];
  auto& gs = m->hf["geom_size"]; auto& gp = m->hf["geom_pos"]; auto& gm = m->hf["geom_mat"];
  auto& gc = m->hf["geom_center"];
  auto& vadr = m->hi["mesh_vertadr"]; auto& vnum = m->hi["mesh_vertnum"];
  auto& bn = m->hi["mesh_binn"]; auto& bc = m->hi["mesh_bincap"]; auto& ba = m->hi["mesh_binadr"];
  int ng = (int)gt.size();
  std::vector<float> rec(32 * std::max(ng, 1), 0.f);
  for (int g = 0; g < ng; g++) {
    float* r = rec.data() + 32 * g;
    int iv[8] = {gt[g], gb[g], 0, 0, 0, 0, 0, 0};
    if (gt[g] == DXG_MESH) {
      int mid = gdid[g];
      iv[2] = vnum[mid]; iv[3] = bn[mid]; iv[4] = bc[mid]; iv[5] = vadr[mid]; iv[6] = ba[mid];
    }
    memcpy(r, iv, sizeof(iv));
    for (int k = 0; k < 3; k++) { r[8 + k] = gs[3 * g + k]; r[12 + k] = gp[3 * g + k]; r[25 + k] = gc[3 * g + k]; }
    for (int k = 0; k < 9; k++) r[16 + k] = gm[9 * g + k];
  }
  m->hf["geom_rec"] = rec;
  auto& pg = m->hi["gpair_geom"]; auto& pm = m->hf["gpair_margin"];
  int np = (int)pm.size();
  std::vector<float> prec(4 * std::max(np, 1), 0.f);
  for (int k = 0; k < np; k++) {
    int g1 = pg[2 * k], g2 = pg[2 * k + 1];
    int prim = gt[g1] == DXG_PLANE || (gt[g1] == DXG_CAPSULE && gt[g2] == DXG_CAPSULE);
    int iv[2] = {g1, g2};
    memcpy(&prec[4 * k], iv, 8);
    prec[4 * k + 2] = pm[k];
    memcpy(&prec[4 * k + 3], &prim, 4);
  }
  m->hf["gpair_rec"] = prec;
}

// geom_bsphere_b, geom_obb_b: geom bounding spheres with centres in the body frame (mid-phase cull)
static void bounding_volumes(dx_model* m) {
  const DevModel& d = m->dm;
  std::vector<float> gb(4 * std::max(d.ngeom, 1), 0.f);
  auto& gs = m->hf["geom_bsphere"]; auto& gp = m->hf["geom_pos"]; auto& gm = m->hf["geom_mat"];
  for (int g = 0; g < d.ngeom; g++) {
    const float* R = gm.data() + 9 * g;
    const float* cc = gs.data() + 4 * g;
    for (int k = 0; k < 3; k++)
      gb[4 * g + k] = gp[3 * g + k] + R[3 * k] * cc[0] + R[3 * k + 1] * cc[1] + R[3 * k + 2] * cc[2];
    gb[4 * g + 3] = cc[3];
  }
  m->hf["geom_bsphere_b"] = gb;
  // oriented bounding box in the body frame: centre(3), R(9) body<-box, half extents(3)
  std::vector<float> ob(15 * std::max(d.ngeom, 1), 0.f);
  auto& ga = m->hf["geom_aabb"];
  for (int g = 0; g < d.ngeom; g++) {
    const float* R = gm.data() + 9 * g;
    const float* a = ga.data() + 6 * g;
    for (int k = 0; k < 3; k++)
      ob[15 * g + k] = gp[3 * g + k] + R[3 * k] * a[0] + R[3 * k + 1] * a[1] + R[3 * k + 2] * a[2];
    for (int k = 0; k < 9; k++) ob[15 * g + 3 + k] = R[k];
    for (int k = 0; k < 3; k++) ob[15 * g + 12 + k] = a[3 + k];
  }
  m->hf["geom_obb_b"] = ob;
}

// geom_crec, bpair_rec.
// collision culling records: per geom {type, body}{bsphere (body frame)}{obb centre,
// R (body <- box), half extents; planes: point, normal} and per body pair {b1, b2,
// first geom pair, count}{sphere 1}{sphere 2}{margin, plane geom, plane body, box
// margin}{plane point | box 1 centre, half x}{plane normal | box 1 half y z, box 2
// centre x y}{box 2 centre z, half extents} (body frames) -- one memory round trip
// per culling item
static void cull_records(dx_model* m) {
  auto& gt = m->hi["geom_type"]; auto& gb = m->hi["geom_bodyid"];
  auto& gbs = m->hf["geom_bsphere_b"]; auto& gob = m->hf["geom_obb_b"];
  auto& gp = m->hf["geom_pos"]; auto& gm = m->hf["geom_mat"];
  int ng = (int)gt.size();
  std::vector<float> cr(24 * std::max(ng, 1), 0.f);
  for (int g = 0; g < ng; g++) {
    float* r = cr.data() + 24 * g;
    int iv[2] = {gt[g], gb[g]};
    memcpy(r, iv, 8);
    for (int k = 0; k < 4; k++) r[4 + k] = gbs[4 * g + k];
    if (gt[g] == DXG_PLANE) {
      for (int k = 0; k < 3; k++) { r[8 + k] = gp[3 * g + k]; r[20 + k] = gm[9 * g + 3 * k + 2]; }
    } else {
      for (int k = 0; k < 3; k++) r[8 + k] = gob[15 * g + k];
      for (int k = 0; k < 9; k++) r[11 + k] = gob[15 * g + 3 + k];
      for (int k = 0; k < 3; k++) r[20 + k] = gob[15 * g + 12 + k];
    }
  }
  m->hf["geom_crec"] = cr;
  auto& bb = m->hi["bpair_body"]; auto& ba = m->hi["bpair_adr"]; auto& bnum = m->hi["bpair_num"];
  auto& bpl = m->hi["bpair_plane"]; auto& bs = m->hf["bpair_sphere"]; auto& pm = m->hf["gpair_margin"];
  int nbp = (int)bnum.size();
  auto& gpg = m->hi["gpair_geom"];
  std::vector<float> br(28 * std::max(nbp, 1), 0.f);
  for (int k = 0; k < nbp; k++) {
    float* r = br.data() + 28 * k;
    int iv[4] = {bb[2 * k], bb[2 * k + 1], ba[k], bnum[k]};
    memcpy(r, iv, 16);
    for (int e = 0; e < 8; e++) r[4 + e] = bs[8 * k + e];
    r[12] = pm[ba[k]];
    int pg = bpl[k], pb = pg >= 0 ? gb[pg] : 0;
    memcpy(r + 13, &pg, 4);
    memcpy(r + 14, &pb, 4);
    if (pg >= 0) {
      for (int e = 0; e < 3; e++) { r[16 + e] = gp[3 * pg + e]; r[20 + e] = gm[9 * pg + 3 * e + 2]; }
    } else {
      // Box cull: per side, the body-frame box around the OBBs (geom_obb_b) of that
      // side's geoms in this pair, grown by a little, and the largest geom-pair
      // margin.  Geom pairs whose OBBs overlap have overlapping boxes, so a pair the
      // boxes separate has no geom pair the mid-phase would keep.
      double lo[2][3] = {{1e30, 1e30, 1e30}, {1e30, 1e30, 1e30}};
      double hi[2][3] = {{-1e30, -1e30, -1e30}, {-1e30, -1e30, -1e30}};
      double mmax = 0;
      for (int q = ba[k]; q < ba[k] + bnum[k]; q++) {
        mmax = std::max(mmax, (double)pm[q]);
        for (int t = 0; t < 2; t++) {
          int g = gpg[2 * q + t];
          int side = gb[g] == bb[2 * k] ? 0 : 1;
          const float* o = gob.data() + 15 * g;
          for (int cnr = 0; cnr < 8; cnr++) {
            double sgn[3] = {(cnr & 1) ? 1.0 : -1.0, (cnr & 2) ? 1.0 : -1.0, (cnr & 4) ? 1.0 : -1.0};
            for (int i = 0; i < 3; i++) {
              double v = o[i];
              for (int jj = 0; jj < 3; jj++) v += (double)o[3 + 3 * i + jj] * sgn[jj] * o[12 + jj];
              lo[side][i] = std::min(lo[side][i], v);
              hi[side][i] = std::max(hi[side][i], v);
            }
          }
        }
      }
      float c[2][3], e[2][3];
      for (int side = 0; side < 2; side++)
        for (int i = 0; i < 3; i++) {
          c[side][i] = (float)(0.5 * (lo[side][i] + hi[side][i]));
          e[side][i] = (float)(0.5 * (hi[side][i] - lo[side][i]) * (1.0 + 1e-4) + 1e-5);
        }
      r[15] = (float)mmax;
      const float rec[12] = {c[0][0], c[0][1], c[0][2], e[0][0], e[0][1], e[0][2],
                             c[1][0], c[1][1], c[1][2], e[1][0], e[1][1], e[1][2]};
      for (int i = 0; i < 12; i++) r[16 + i] = rec[i];
    }
  }
  m->hf["bpair_rec"] = br;
}

// Body-pair cull tables.  The units of a scene share a few bounding spheres (a palm
// cluster's ~15 partners meet the same cluster sphere, every cluster the same partner
// spheres) and one ground plane, so the kernel transforms each distinct one once per
// pass (dx_step.hip collision) and a unit only names its two:
//   bp_item [nbitem][2] float4, planes first then spheres, keyed on the float32 bits
//     the per-unit loop used to read: plane {point, geom}{normal, body | 1 << 16}
//     (its body's frame), sphere {centre, radius}{0, 0, 0, body};
//   bp_cull [nbpair] {item 1 | item 2 << 12 | flags, margin}: DX_CULL_PLANE item 1 is
//     a plane (plane test against sphere 2), DX_CULL_KEEP no sphere on a side (kept
//     without a test), neither: sphere test, then the box test of bpair_rec.
static int body_pair_items(dx_model* m) {
  DevModel& d = m->dm;
  auto& gb = m->hi["geom_bodyid"]; auto& gp = m->hf["geom_pos"]; auto& gm = m->hf["geom_mat"];
  auto& bb = m->hi["bpair_body"]; auto& ba = m->hi["bpair_adr"]; auto& bpl = m->hi["bpair_plane"];
  auto& bs = m->hf["bpair_sphere"]; auto& pm = m->hf["gpair_margin"];
  const int nbp = (int)m->hi["bpair_num"].size();
  std::vector<float> items;
  std::vector<int> cull(2 * std::max(nbp, 1), 0);
  std::map<std::array<uint32_t, 5>, int> ids;
  auto item_id = [&](bool plane, int key0, const float* key4, const float* a, const float* b, int body) {
    std::array<uint32_t, 5> key;
    key[0] = (uint32_t)key0 | (plane ? 0x80000000u : 0u);
    memcpy(&key[1], key4, 16);
    auto it = ids.find(key);
    if (it != ids.end()) return it->second;
    const int id = (int)ids.size();
    ids[key] = id;
    float e[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], 0.f};
    const int tag = body | (plane ? 1 << 16 : 0);
    memcpy(e + 7, &tag, 4);
    items.insert(items.end(), e, e + 8);
    return id;
  };
  const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
  int nplane = 0;
  for (int pass = 0; pass < 2; pass++)  // planes take the first ids
    for (int k = 0; k < nbp; k++) {
      const float* s1 = bs.data() + 8 * k;
      const float* s2 = s1 + 4;
      const int pg = bpl[k];
      const bool tested = s2[3] >= 0 && (pg >= 0 || s1[3] >= 0);
      if (pass == 0) {
        if (tested && pg >= 0) {
          float pt[4] = {gp[3 * pg], gp[3 * pg + 1], gp[3 * pg + 2], 0.f};
          const float nl[3] = {gm[9 * pg + 2], gm[9 * pg + 5], gm[9 * pg + 8]};
          memcpy(pt + 3, &pg, 4);
          item_id(true, pg, zero4, pt, nl, gb[pg]);
        }
        nplane = (int)ids.size();
        continue;
      }
      int w = DX_CULL_KEEP;
      if (tested) {
        const int i2 = item_id(false, bb[2 * k + 1], s2, s2, zero4, bb[2 * k + 1]);
        float pt[4] = {0.f, 0.f, 0.f, 0.f};
        const int i1 = pg >= 0 ? item_id(true, pg, zero4, pt, zero4, 0)  // (found: pass 0 made it)
                               : item_id(false, bb[2 * k], s1, s1, zero4, bb[2 * k]);
        w = i1 | (i2 << 12) | (pg >= 0 ? DX_CULL_PLANE : 0);
      }
      cull[2 * k] = w;
      memcpy(&cull[2 * k + 1], &pm[ba[k]], 4);
    }
  d.nbitem = (int)ids.size();
  d.nbplane = nplane;
  // world-space items live in the narrowphase's portal area while the pairs are tested:
  // one float4 per item and a second one per plane
  if (d.nbitem + d.nbplane > DX_NGRP_MAX * 36 / 4)
    return dx_fail(DX_ELIMIT, "distinct broadphase spheres and planes exceed the LDS item area");
  if (items.empty()) items.assign(8, 0.f);
  m->hf["bp_item"] = items;
  m->hi["bp_cull"] = cull;
  return 0;
}

// body_rec, dof_rec: tree records: per body (lane = body in the level loops) and per dof, so
// a stage loads its model data in one memory round trip instead of a chain per tree level
static int tree_records(dx_model* m, const std::vector<int>& depth) {
  const int nb = m->dm.nbody, nv = m->dm.nv;
  if (nb > 64) return dx_fail(DX_ELIMIT, "nbody must be <= 64 (one lane per body)");
  auto& parent = m->hi["body_parent"]; auto& rootidx = m->hi["body_rootidx"];
  auto& dofadr = m->hi["body_dofadr"]; auto& dofnum = m->hi["body_dofnum"];
  auto& bja = m->hi["body_jntadr"]; auto& bjn = m->hi["body_jntnum"];
  auto& jt = m->hi["jnt_type"]; auto& jqa = m->hi["jnt_qposadr"]; auto& jda = m->hi["jnt_dofadr"];
  auto& bpos = m->hf["body_pos"]; auto& bquat = m->hf["body_quat"]; auto& bipos = m->hf["body_ipos"];
  auto& jpos = m->hf["jnt_pos"]; auto& jax = m->hf["jnt_axis"]; auto& q0 = m->hf["qpos0"];
  auto& bmass = m->hf["body_mass"]; auto& binert = m->hf["body_inertia"];
  std::vector<float> br(32 * nb, 0.f);
  for (int b = 0; b < nb; b++) {
    float* r = br.data() + 32 * b;
    int ja = bja[b], jn = bjn[b];
    int iv0[4] = {parent[b], depth[b], ja, jn};
    memcpy(r, iv0, 16);
    int jtp = jn > 0 ? jt[ja] : -1, qa = jn > 0 ? jqa[ja] : 0, jd = jn > 0 ? jda[ja] : 0;
    for (int k = 0; k < 3; k++) { r[4 + k] = bpos[3 * b + k]; r[12 + k] = bipos[3 * b + k]; }
    memcpy(r + 7, &jtp, 4);
    for (int k = 0; k < 4; k++) r[8 + k] = bquat[4 * b + k];
    memcpy(r + 15, &rootidx[b], 4);
    if (jn > 0)
      for (int k = 0; k < 3; k++) { r[16 + k] = jpos[3 * ja + k]; r[20 + k] = jax[3 * ja + k]; }
    memcpy(r + 19, &qa, 4);
    r[23] = jn > 0 ? q0[qa] : 0.f;
    int iv6[2] = {dofadr[b], dofnum[b]};
    memcpy(r + 24, iv6, 8);
    r[26] = bmass[b];
    memcpy(r + 27, &jd, 4);
    for (int k = 0; k < 3; k++) r[28 + k] = binert[3 * b + k];
  }
  m->hf["body_rec"] = br;
  auto& dbody = m->hi["dof_bodyid"]; auto& djnt = m->hi["dof_jntid"];
  auto& arm = m->hf["dof_armature"]; auto& dmp = m->hf["dof_damping"];
  std::vector<float> dr(8 * nv, 0.f);
  for (int d2 = 0; d2 < nv; d2++) {
    float* r = dr.data() + 8 * d2;
    int b = dbody[d2], j = djnt[d2];
    int tk = jt[j] | ((d2 - jda[j]) << 8);
    int iv[4] = {b, j, rootidx[b], tk};
    memcpy(r, iv, 16);
    r[4] = arm[d2];
    r[5] = dmp[d2];
    uint64_t anc = m->body_chain[b] & ((d2 >= 63) ? ~0ull : ((2ull << d2) - 1ull));
    uint32_t lo = (uint32_t)anc, hi = (uint32_t)(anc >> 32);
    memcpy(r + 6, &lo, 4);
    memcpy(r + 7, &hi, 4);
  }
  m->hf["dof_rec"] = dr;
  return 0;
}

// ldl_tab, ldl_nslot, ldl_sync.
// Tree-sparse LDL^T of M (dx_device.h tree_solve): the elimination items (k, i, j)
// -- dof k, a proper ancestor i of k, j = i or an ancestor of i -- grouped by the
// height of k above the leaves (a level's dofs are never ancestors of one another),
// each level padded to whole 64-item slots; bit s of ldl_sync closes a level at
// slot s.  Deeper trees than DX_LDL_SLOTS slots keep the dense solver (nslot 0).
static void ldl_table(dx_model* m) {
  DevModel& d = m->dm; const int nv = d.nv;
  auto& par = m->hi["dof_parentid"];
  std::vector<int> height(nv, 0);
  for (int k = nv - 1; k >= 0; k--)
    if (par[k] >= 0) height[par[k]] = std::max(height[par[k]], height[k] + 1);
  int hmax = 0;
  for (int k = 0; k < nv; k++) hmax = std::max(hmax, height[k]);
  std::vector<int> tab;
  unsigned sync = 0;
  int nslot = 0;
  for (int h = 0; h <= hmax; h++) {
    std::vector<int> items;
    for (int k = 0; k < nv; k++) {
      if (height[k] != h) continue;
      for (int i = par[k]; i >= 0; i = par[i])
        for (int j = i; j >= 0; j = par[j]) items.push_back(k | (i << 8) | (j << 16));
    }
    if (items.empty()) continue;
    const int ns = ((int)items.size() + DX_WAVE - 1) / DX_WAVE;
    items.resize((size_t)ns * DX_WAVE, -1);
    tab.insert(tab.end(), items.begin(), items.end());
    nslot += ns;
    if (nslot <= 32) sync |= 1u << (nslot - 1);
  }
  const char* dense = getenv("DX_DENSE_MSOLVE");  // A/B switch: the matrix-core Cholesky
  if (nslot > DX_LDL_SLOTS || nv > DX_MAX_NV || (dense && dense[0] == '1')) { nslot = 0; sync = 0; tab.clear(); }
  d.ldl_nslot = nslot;
  d.ldl_sync = sync;
  m->hi["ldl_tab"] = tab;
}

// Friction rows / limited joints / limited tendons: fric_dof, dof_fricrow, limj_jnt, limt_ten.
static void row_lists(dx_model* m) {
  DevModel& d = m->dm; const int nv = d.nv;
  std::vector<int> fric_dof, dof_fricrow(nv, -1), limj, limt;
  auto& floss = m->hf["dof_frictionloss"];
  for (int i = 0; i < nv; i++)
    if (floss[i] > 0) { dof_fricrow[i] = (int)fric_dof.size(); fric_dof.push_back(i); }
  auto& jtype = m->hi["jnt_type"];
  auto& jlim = m->hi["jnt_limited"];
  for (int j = 0; j < d.njnt; j++)
    if (jlim[j] && jtype[j] == DXJ_HINGE) limj.push_back(j);
  auto& tlim = m->hi["tendon_limited"];
  for (int t = 0; t < d.ntendon; t++)
    if (tlim[t]) limt.push_back(t);
  d.nfric = (int)fric_dof.size();
  d.nlimj = (int)limj.size();
  d.nlimt = (int)limt.size();
  m->hi["fric_dof"] = fric_dof.empty() ? std::vector<int>{0} : fric_dof;
  m->hi["dof_fricrow"] = dof_fricrow;
  m->hi["limj_jnt"] = limj.empty() ? std::vector<int>{0} : limj;
  m->hi["limt_ten"] = limt.empty() ? std::vector<int>{0} : limt;
}

// Wraps: qpos address (wrap_qadr); dense tendon jacobian (tendon_J).
static void tendon_tables(dx_model* m) {
  const DevModel& d = m->dm; const int nv = d.nv;
  auto& wdof = m->hi["wrap_dof"];
  auto& dofj = m->hi["dof_jntid"];
  auto& jqa = m->hi["jnt_qposadr"];
  std::vector<int> wqadr(std::max(d.nwrap, 1), 0);
  for (int w = 0; w < d.nwrap; w++) wqadr[w] = jqa[dofj[wdof[w]]];
  m->hi["wrap_qadr"] = wqadr;
  std::vector<float> tJ(std::max(d.ntendon, 1) * nv, 0.f);
  auto& tadr = m->hi["tendon_adr"];
  auto& tnum = m->hi["tendon_num"];
  auto& wcoef = m->hf["wrap_coef"];
  for (int t = 0; t < d.ntendon; t++)
    for (int w = tadr[t]; w < tadr[t] + tnum[t]; w++) tJ[t * nv + wdof[w]] += wcoef[w];
  m->hf["tendon_J"] = tJ;
}

// The kernels' compile-time switches: any_damping, solimp_pow2.
static void model_switches(dx_model* m) {
  DevModel& d = m->dm; const int nv = d.nv;
  auto& damp = m->hf["dof_damping"];
  d.any_damping = 0;
  for (int i = 0; i < nv; i++)
    if (damp[i] > 0) d.any_damping = 1;
  // the impedance's power: 2 on every row the model can build?  (each table is [n][5],
  // power last; the geom pairs' solimp is the mixed one)
  d.solimp_pow2 = 1;
  const std::pair<const char*, int> solimp_tabs[] = {
      {"dof_solimp", nv}, {"jnt_solimp", d.njnt}, {"tendon_solimp", d.ntendon}, {"gpair_solimp", d.ngpair}};
  for (const auto& tab : solimp_tabs) {
    const auto it = m->hf.find(tab.first);
    if (it == m->hf.end()) continue;
    for (int i = 0; i < tab.second && 5 * i + 4 < (int)it->second.size(); i++)
      if (it->second[5 * i + 4] != 2.0f) d.solimp_pow2 = 0;
  }
}

// LDS layout (4-byte words) with a contact pool of `cap`.  Persistent arrays first, then a
// union whose contents change with the stage (dx_step.hip forward()):
//   A  kinematic block      xpos xmat xipos rcom cdof   kinematics .. make_constraint
//   B1 com temporaries      cinert cvel cdof_dot scr xanchor xaxis xquat
//                                                       kinematics .. velocity stage
//   B2 smooth-solve transpose (packed nv x nv)          smooth solve
//   B3 candidate lists + hull staging                   collision
//   B4 constraint rows + contact jacobians              make_constraint .. qfrc_constraint
//   H  Newton Hessian / Euler transpose over A          solve, euler
// The union keeps one environment in < 20 KB for the Shadow scene, so eight
// 64-lane workgroups (two waves per SIMD) fit in a CU's 160 KB.
static void lds_layout(dx_model* m, int cap, Lds& L) {
  const DevModel& d = m->dm;
  const int nb = d.nbody, nv = d.nv;
  int off = 0;
  auto take = [&](int n) { int o = off; off += (n + 3) & ~3; return o; };
  auto r4 = [](int n) { return (n + 3) & ~3; };
  const int ntri = nv * (nv + 1) / 2;
  L.ints = take(16);
  L.qpos = take(d.nq); L.qvel = take(nv); L.ctrl = take(std::max(d.nu, 1)); L.qacc = take(nv);
  L.qacc_smooth = take(nv); L.qfrc_smooth = take(nv); L.qfrc_con = take(nv);
  L.v1 = take(nv); L.v2 = take(nv); L.v3 = take(nv); L.v4 = take(nv); L.v5 = take(nv);
  L.M = take(ntri);
  L.ten_len = take(std::max(d.ntendon, 1));  // read by the tendon-limit rows: persistent
  L.con = take((cap + DX_NCON_SPARE) * DX_CON_STRIDE);
  // limit rows: a joint / tendon whose range is wider than twice its margin can have only
  // one side within the margin at a time (q - lo < margin and hi - q < margin need
  // hi - lo < 2 margin), so it holds one row, else two
  int nlimrow = 0;
  {
    auto& jr = m->hf["jnt_range"]; auto& jm = m->hf["jnt_margin"];
    auto& limj = m->hi["limj_jnt"]; auto& limt = m->hi["limt_ten"];  // (row_lists: nlimj, nlimt entries)
    auto rows = [](const float* range, float margin) { return (range[1] - range[0]) > 2.0f * margin + 1e-4f ? 1 : 2; };
    for (int k = 0; k < d.nlimj; k++) nlimrow += rows(&jr[2 * limj[k]], jm[limj[k]]);
    auto& tr = m->hf["tendon_range"]; auto& tm = m->hf["tendon_margin"];
    for (int k = 0; k < d.nlimt; k++) nlimrow += rows(&tr[2 * limt[k]], tm[limt[k]]);
  }
  L.nefc_max = d.nfric + nlimrow + 4 * cap;
  L.efc_fl = take(std::max(d.nfric, 1)); L.efc_Rf = take(std::max(d.nfric, 1));
  L.tri = 0;  // (was the wave Cholesky's index table; n > 32 now factors on the matrix cores)
  const int U0 = off;
  L.xpos = take(3 * nb); L.xmat = take(9 * nb); L.xipos = take(3 * nb);
  L.rcom = take(3 * std::max(d.nroot, 1)); L.cdof = take(6 * nv);
  const int B0 = off;
  L.cinert = take(10 * nb); L.cvel = take(6 * nb); L.cdof_dot = take(6 * nv); L.scr = take(12 * nb);
  L.xanchor = take(3 * std::max(d.njnt, 1)); L.xaxis = take(3 * std::max(d.njnt, 1));
  L.xquat = take(4 * nb);
  // actuator lengths: tendon_lengths -> the velocity stage's actuator forces
  L.act_len = take(std::max(d.nu, 1));
  L.act_force = L.act_len;  // (no longer stored)
  int end = off;
  L.tsm = B0;
  end = std::max(end, B0 + r4(ntri));
  L.cand_max = DX_CAND_MAX;
  L.cand = B0;
  // + MPR portal points of up to DX_NGRP_MAX narrowphase groups (36 words each), then the
  // candidates' pair records (float4 per candidate slot: cand_max - 2 * (cand_max / 3))
  end = std::max(end, L.cand + L.cand_max + DX_NGRP_MAX * 36 + 4 * (L.cand_max - 2 * (L.cand_max / 3)));
  off = std::max(B0, U0 + r4(ntri));
  L.efc_meta = take(L.nefc_max); L.efc_D = take(L.nefc_max); L.efc_aref = take(L.nefc_max);
  L.efc_jar = take(L.nefc_max);
  L.cj_idx = take((cap * DX_DOFMAX + 3) / 4);  // uint8 dof ids
  L.cj_val = take(cap * 3 * DX_DOFMAX);
  // contact-frame scratch: J x in jac_vec, the frame forces in jac_t_force (and the
  // sensor stash right after the last one); never live at the same time
  L.cq = take(3 * cap);
  L.cw = L.cq;
  // The solver's J dir (efc_jv) and CG's M^-1 grad (PGS's M^-1 J_r'): written only from
  // the solve on, when the kinematic block is dead, so they go past the Newton Hessian
  // when it has room
  int spare = U0 + r4(ntri);
  if (spare + r4(L.nefc_max) <= B0) { L.efc_jv = spare; spare += r4(L.nefc_max); }
  else L.efc_jv = take(L.nefc_max);
  if (d.solver == 2) L.cgv = 0;  // Newton: no CG / PGS scratch
  else if (spare + r4(nv) <= B0) L.cgv = spare;
  else L.cgv = take(nv);
  end = std::max(end, off);
  L.H = U0;
  L.total = (end + 3) & ~3;  // the kernels zero it with 16-byte stores
}

extern "C" dx_model* dx_model_load(const void* blob, size_t nbytes) {
  if (!blob) { dx_fail(DX_EINVAL, "null blob"); return nullptr; }
  std::unique_ptr<dx_model> owner(new dx_model());
  dx_model* m = owner.get();
  m->blob.assign((const unsigned char*)blob, (const unsigned char*)blob + nbytes);
  if (!parse_blob(m->blob.data(), nbytes, m->arr)) { dx_fail(DX_EMODEL, "malformed model blob"); return nullptr; }
  if (load_arrays(m)) return nullptr;
  const DevModel& d = m->dm;
  std::vector<int> depth;
  tree_levels(m, depth);
  if (dof_chains(m)) return nullptr;
  rotations_and_verts(m);
  build_hull_bins(m);
  narrowphase_records(m);
  bounding_volumes(m);
  cull_records(m);
  if (body_pair_items(m)) return nullptr;
  if (tree_records(m, depth)) return nullptr;
  ldl_table(m);
  row_lists(m);
  tendon_tables(m);
  model_switches(m);
  // the step kernel's layout (pool DX_NCON_MAX), the overflow tier's and the mid tier's
  lds_layout(m, DX_NCON_MAX, m->lds);
  lds_layout(m, DX_NCON_HI, m->lds_hi);
  lds_layout(m, DX_NCON_MID, m->lds_mid);
  if (m->lds_mid.nefc_max > 5 * 64) m->lds_mid.nefc_max = 0;  // (its line search keeps 5 register slots)
  if (getenv("DX_PRINT_LDS"))
    fprintf(stderr, "dx: LDS per env %d B (step kernel), %d B (mid tier), %d B (overflow tier)\n", m->lds.total * 4,
            m->lds_mid.total * 4, m->lds_hi.total * 4);
  // the contact tiers exist only for a model that can have contacts (dx_batch_create
  // allocates the deferral lists and launches the tiers for those only): a contact-free
  // model is held to the step kernel's layout alone
  const bool tiers = !d.disable_contact && d.ngpair > 0;
  m->ncon_max = tiers ? DX_NCON_HI : DX_NCON_MAX;
  m->nefc_max = tiers ? m->lds_hi.nefc_max : m->lds.nefc_max;
  // line-search register slots (dx_device.h DX_LS_SLOTS: 5 in the generic step kernel and
  // the mid tier, 20 in the overflow tier; a scene specialization keeps CtxT::ls_slots, its
  // own row bound, which a static_assert holds at or below DX_LS_SLOTS).  The literal 5 * 64
  // here and above (lds_mid) and 20 * 64 must stay in step with DX_LS_SLOTS: that assert and
  // the kernels' register arrays rely on this check
  if (m->lds.nefc_max > 5 * 64 || (tiers && m->lds_hi.nefc_max > 20 * 64)) {
    dx_fail(DX_ELIMIT, "constraint row capacity exceeds the line search's register slots");
    return nullptr;
  }
  if (m->lds.total * 4 > 160 * 1024 || (tiers && m->lds_hi.total * 4 > 160 * 1024)) {
    dx_fail(DX_ELIMIT, "per-env LDS footprint exceeds 160 KiB");
    return nullptr;
  }
  return owner.release();
}

extern "C" int dx_model_sizes(const dx_model* m, int32_t out[12]) {
  if (!m || !out) return dx_fail(DX_EINVAL, "null argument");
  const DevModel& d = m->dm;
  int v[12] = {d.nq, d.nv, d.nbody, d.njnt, d.ngeom, d.nsite, d.nu, d.ntendon, d.nbpair, d.ngpair,
               m->ncon_max, m->nefc_max};
  memcpy(out, v, sizeof(v));
  return 0;
}

// Host twin of the device's binned support scan (test hook): the vertex index the
// kernel's support_grp returns for hull `mesh` along local direction dir, plus the
// mesh's cube-map resolution and cell capacity (0, 0 when the hull is not binned).
extern "C" int dx_hull_support(const dx_model* m, int32_t mesh, const float dir[3], int32_t info[3]) {
  if (!m || !dir || !info) return dx_fail(DX_EINVAL, "null argument");
  auto& num = m->hi.at("mesh_vertnum");
  if (mesh < 0 || mesh >= (int)num.size()) return dx_fail(DX_EINVAL, "mesh out of range");
  int n = m->hi.at("mesh_binn")[mesh], cap = m->hi.at("mesh_bincap")[mesh];
  const float* b4 = m->hf.at("mesh_bin4").data() + 4 * (size_t)m->hi.at("mesh_binadr")[mesh];
  const float* mv = m->hf.at("mesh_vert").data() + 3 * (size_t)m->hi.at("mesh_vertadr")[mesh];
  int best = -1;
  float bd = -3.0e38f;
  int cell = -1;
  if (n > 0) {
    float ax0 = std::fabs(dir[0]), ax1 = std::fabs(dir[1]), ax2 = std::fabs(dir[2]);
    int ax = (ax0 >= ax1 && ax0 >= ax2) ? 0 : (ax1 >= ax2 ? 1 : 2);
    float a = dir[ax], u = dir[(ax + 1) % 3], v = dir[(ax + 2) % 3];
    if (std::fabs(a) > 1e-30f) {
      float inv = 1.0f / std::fabs(a);
      int iu = std::min(std::max((int)((u * inv + 1.0f) * 0.5f * (float)n), 0), n - 1);
      int iv = std::min(std::max((int)((v * inv + 1.0f) * 0.5f * (float)n), 0), n - 1);
      cell = ((2 * ax + (a < 0 ? 1 : 0)) * n + iu) * n + iv;
    }
  }
  if (cell >= 0) {
    // the cell's block, then its overflow run when slot K - 1 is a header
    const int K = cap;
    const float* blk = b4 + 4 * (size_t)cell * K;
    int hdr;
    memcpy(&hdr, blk + 4 * (K - 1) + 3, 4);
    int off = 0, cnt = K;
    if (hdr == -2) { memcpy(&off, blk + 4 * (K - 1), 4); memcpy(&cnt, blk + 4 * (K - 1) + 1, 4); }
    for (int s = 0; s < cnt; s++) {
      const float* e = hdr == -2 && s >= K - 1 ? b4 + 4 * ((size_t)off + s - (K - 1)) : blk + 4 * s;
      int idx;
      memcpy(&idx, e + 3, 4);
      if (idx < 0) continue;
      float d = e[0] * dir[0] + e[1] * dir[1] + e[2] * dir[2];
      if (d > bd) { bd = d; best = idx; }
    }
  } else {
    for (int i = 0; i < num[mesh]; i++) {
      float d = mv[3 * i] * dir[0] + mv[3 * i + 1] * dir[1] + mv[3 * i + 2] * dir[2];
      if (d > bd) { bd = d; best = i; }
    }
  }
  info[0] = best;
  info[1] = n;
  info[2] = cap;
  return 0;
}

// Hull face planes for the ray cast (dx_render.hip).  The blob carries a hull's vertices and
// the vertex adjacency, no faces.  For a vertex i and two of its neighbours j, k that are
// neighbours of each other (i < j < k: every triangle once), the plane through the three is
// a face when every hull vertex lies on one side of it, to 1e-9 max|v|; it is oriented
// outward and stored as unit (n, d), n x + d <= 0 inside.  Coplanar triangles (a polygonal
// face's fan) merge into one plane.  fp64 on the blob's fp64 vertices, rounded once.
std::recursive_mutex g_render_mu;
int hull_planes(dx_model* m) {
  std::lock_guard<std::recursive_mutex> lock(g_render_mu);
  if (m->planes_built) return 0;
  const auto& vadr = m->hi.at("mesh_vertadr");
  const auto& vnum = m->hi.at("mesh_vertnum");
  const int nmesh = (int)vnum.size();
  m->planeadr.assign(std::max(nmesh, 1), 0);
  m->planenum.assign(std::max(nmesh, 1), 0);
  m->plane4.clear();
  auto iv = m->arr.find("mesh_vert");
  auto ia = m->arr.find("mesh_vertadj");
  auto ij = m->arr.find("mesh_adj");
  if (nmesh > 0 && (iv == m->arr.end() || ia == m->arr.end() || ij == m->arr.end() || iv->second.dtype != 1 ||
                    ia->second.dtype != 0 || ij->second.dtype != 0))
    return dx_fail(DX_EMODEL, "hull planes: the blob lacks mesh_vert / mesh_vertadj / mesh_adj");
  for (int k = 0; k < nmesh; k++) {
    const int nv = vnum[k], base = vadr[k];
    if (base < 0 || (long)(base + nv) * 3 > iv->second.n || (long)(base + nv) * 2 > ia->second.n)
      return dx_fail(DX_EMODEL, "hull planes: mesh vertex range outside the blob's arrays");
    const double* V = (const double*)iv->second.p + 3 * (size_t)base;
    const int* VA = (const int*)ia->second.p + 2 * (size_t)base;
    const int* ADJ = (const int*)ij->second.p;
    const long nadj = ij->second.n;
    double R = 0;
    for (int i = 0; i < 3 * nv; i++) R = std::max(R, std::fabs(V[i]));
    const double tol = 1e-9 * R;
    // two planes merge when their unit normals agree to kMerge per component and their
    // offsets to kMerge R: the meshes' vertices are float32 data, so a polygonal face's
    // triangles are coplanar only to ~1e-7; the first one met stands for the face (a shift
    // of at most 1e-6 R, below what the fp32 ray cast resolves)
    const double kMerge = 1e-6;
    std::vector<std::array<double, 4>> planes;
    for (int i = 0; i < nv; i++) {
      const int s = VA[2 * i], c = VA[2 * i + 1];
      if (s < 0 || c < 0 || (long)s + c > nadj) return dx_fail(DX_EMODEL, "hull planes: adjacency outside the blob's array");
      for (int a = 0; a < c; a++) {
        const int j = ADJ[s + a];
        if (j <= i || j >= nv) continue;
        const int sj = VA[2 * j], cj = VA[2 * j + 1];
        if (sj < 0 || cj < 0 || (long)sj + cj > nadj) return dx_fail(DX_EMODEL, "hull planes: adjacency outside the blob's array");
        for (int b2 = 0; b2 < c; b2++) {
          const int k2 = ADJ[s + b2];
          if (k2 <= j || k2 >= nv) continue;
          bool adj = false;
          for (int q = 0; q < cj && !adj; q++) adj = ADJ[sj + q] == k2;
          if (!adj) continue;
          const double* p0 = V + 3 * i; const double* p1 = V + 3 * j; const double* p2 = V + 3 * k2;
          const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
          const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
          double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
          const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
          if (!(len > 1e-14 * R * R)) continue;  // a degenerate triple
          for (double& x : n) x /= len;
          double d = -(n[0] * p0[0] + n[1] * p0[1] + n[2] * p0[2]);
          double lo = 0, hi = 0;
          for (int v = 0; v < nv; v++) {
            const double sd = n[0] * V[3 * v] + n[1] * V[3 * v + 1] + n[2] * V[3 * v + 2] + d;
            lo = std::min(lo, sd);
            hi = std::max(hi, sd);
          }
          if (hi > tol && lo < -tol) continue;  // vertices on both sides: not a face
          if (hi > tol) { for (double& x : n) x = -x; d = -d; }
          bool dup = false;
          for (const auto& P : planes)
            if (std::fabs(P[0] - n[0]) < kMerge && std::fabs(P[1] - n[1]) < kMerge && std::fabs(P[2] - n[2]) < kMerge &&
                std::fabs(P[3] - d) < kMerge * std::max(R, 1e-300)) { dup = true; break; }
          if (!dup) planes.push_back({n[0], n[1], n[2], d});
        }
      }
    }
    m->planeadr[k] = (int)(m->plane4.size() / 4);
    m->planenum[k] = (int)planes.size();
    for (const auto& P : planes)
      for (int q = 0; q < 4; q++) m->plane4.push_back((float)P[q]);
  }
  m->planes_built = true;
  return 0;
}

extern "C" int dx_model_hull_planes(const dx_model* mc, int32_t mesh, float* out, int32_t n) {
  dx_model* m = const_cast<dx_model*>(mc);
  if (!m) return dx_fail(DX_EINVAL, "null model");
  if (mesh < 0 || mesh >= (int)m->hi.at("mesh_vertnum").size()) return dx_fail(DX_EINVAL, "mesh out of range");
  if (int rc = hull_planes(m)) return rc;
  const int cnt = m->planenum[mesh];
  if (out && n > 0)
    memcpy(out, m->plane4.data() + 4 * (size_t)m->planeadr[mesh], (size_t)std::min(n, cnt) * 16);
  return cnt;
}

// Layout export for build.py's kernel specialization: the Lds struct (words, in
// declaration order) followed by the 18 dimensions of dx_device.h DX_DIMS.
extern "C" int dx_model_layout(const dx_model* m, int32_t* out, int32_t n) {
  if (!m || !out) return dx_fail(DX_EINVAL, "null argument");
  const int nl = (int)(sizeof(Lds) / sizeof(int));
  const DevModel& d = m->dm;
  int dims[18] = {d.nq, d.nv, d.nbody, d.njnt, d.nu, d.ntendon, d.nsite, d.nlevel, d.nroot,
                  d.nfric, d.nlimj, d.nlimt, d.nbpair, d.any_damping, d.disable_contact, d.iterations, d.solver,
                  d.solimp_pow2};
  if (n < nl + 18) return dx_fail(DX_EINVAL, "output too small");
  memcpy(out, &m->lds, sizeof(Lds));
  memcpy(out + nl, dims, sizeof(dims));
  return nl + 18;
}

extern "C" int dx_model_lds_bytes(const dx_model* m) {
  if (!m) return dx_fail(DX_EINVAL, "null model");
  return m->lds.total * 4;
}

extern "C" int dx_field_width(const dx_model* m, int field) {
  if (!m) return dx_fail(DX_EINVAL, "null model");
  const DevModel& d = m->dm;
  switch (field) {
    case DX_QPOS: return d.nq;
    case DX_QVEL: case DX_QACC_WARMSTART: case DX_QACC: return d.nv;
    case DX_CTRL: return d.nu;
    case DX_TIME: case DX_NCON: case DX_GROUND_CONTACT: case DX_NITER: case DX_NCAND: case DX_STEP_COST:
    case DX_DIVERGED: return 1;
    case DX_SITE_XPOS: return 3 * d.nsite;
    case DX_SITE_VEL: return 6 * d.nsite;
    case DX_XPOS: return 3 * d.nbody;
    case DX_XQUAT: return 4 * d.nbody;
    case DX_SENSOR_TORQUE: return 3 * d.nbody;
    case DX_CFRC_EXT: return 6 * d.nbody;
    case DX_PAD_FORCE: return 0;  // the pads are a batch's (dx_contact_set_pads): a model has none
  }
  return dx_fail(DX_EINVAL, "unknown field");
}

#ifndef DX_BUILD_KEY
#define DX_BUILD_KEY "unkeyed"
#endif
// The hash of the sources this library was built from (dexterity_amd/build.py source_key)
extern "C" const char* dx_build_key(void) { return DX_BUILD_KEY; }
