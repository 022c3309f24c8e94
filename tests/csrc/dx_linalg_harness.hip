// Test harness for the wave-level linear algebra and reductions of dx_device.h
// (tests/test_gpu_linalg.py, built and loaded by tests/linalg_harness.py).
//
// One __global__ kernel per routine; one workgroup is one wave and one case, and every
// block reads its own n, so all cases of a routine go in one launch.  A kernel first fills
// its whole LDS image with the caller's fill word (a NaN pattern, or zero for the
// poison-independence check), then stages the packed triangle A (ti(n) words) and x
// (n words) as the routine's callers do, runs the routine and copies the whole LDS image
// back: the host sees what the routine wrote and what it left alone.
//
// The extern "C" entry points take host pointers, do their own allocation, copies, launch
// and synchronisation, and return the HIP error code (or DXH_EINVAL for an argument that
// could index out of bounds on the device).  Nothing aborts.
//
// Compiled twice with build.py's FLAGS: -DDX_LANE_RANGE_MASK=0 (what dx_ik / dx_dls see)
// and -DDX_LANE_RANGE_MASK=0x3b (what dx_step.hip sees).
#include <hip/hip_runtime.h>

#include <vector>

#include "dx_device.h"

#define DXH_EINVAL (-1)
// LDS image layouts (words): a packed triangle of up to 32 / 64 rows, a 64-word vector
#define DXH_TRI32 528   // ti(32)
#define DXH_TRI64 2080  // ti(64)
#define DXH_VEC 64
#define DXH_W_SWEEP (DXH_TRI32 + DXH_VEC)               // A | x
#define DXH_W_CHOL32 (2 * DXH_TRI32 + DXH_VEC)          // A | x | T
#define DXH_W_CHOL64 (2 * DXH_TRI64 + DXH_VEC)          // A | x | T
#define DXH_W_INV (2 * DXH_TRI32)                       // A | Ainv
#define DXH_W_FACTOR (DXH_TRI32)                        // A
#define DXH_W_TREE (2 * DXH_TRI64 + DXH_VEC)            // A | x | T

namespace {

__device__ __forceinline__ void fill_lds(float* sm, int words, unsigned fill) {
  for (int k = LANE; k < words; k += DX_WAVE) sm[k] = __uint_as_float(fill);
  SYNC();
}
__device__ __forceinline__ void stage(float* dst, const float* src, int words) {
  for (int k = LANE; k < words; k += DX_WAVE) dst[k] = src[k];
}
__device__ __forceinline__ void dump_lds(float* out, const float* sm, int words) {
  SYNC();
  for (int k = LANE; k < words; k += DX_WAVE) out[k] = sm[k];
}
__device__ __forceinline__ const DXG float* as_table(const float* p) { return (const DXG float*)p; }

// A: [ncase][tri] (the first ti(n) words used), d: [ncase][64] diagonal adds, x: [ncase][64]
__global__ __launch_bounds__(64) void k_sweep_solve30(const int* nn, const float* A, const float* d, const float* x,
                                                      unsigned fill, float* out) {
  __shared__ float sm[DXH_W_SWEEP];
  const int b = blockIdx.x, n = nn[b];
  fill_lds(sm, DXH_W_SWEEP, fill);
  float* As = sm;
  float* xs = sm + DXH_TRI32;
  stage(As, A + (size_t)b * DXH_TRI32, ti(n));
  stage(xs, x + (size_t)b * DXH_VEC, n);
  const DiagAdd dd = diag_add(as_table(d + (size_t)b * DXH_VEC), 1.0f, n);
  SYNC();
  mfma_sweep_solve30(As, n, dd.d1, xs);
  dump_lds(out + (size_t)b * DXH_W_SWEEP, sm, DXH_W_SWEEP);
}

__global__ __launch_bounds__(64) void k_chol_solve32(const int* nn, const float* A, const float* d, const float* x,
                                                     int alias, unsigned fill, float* out) {
  __shared__ float sm[DXH_W_CHOL32];
  const int b = blockIdx.x, n = nn[b];
  fill_lds(sm, DXH_W_CHOL32, fill);
  float* As = sm;
  float* xs = sm + DXH_TRI32;
  float* Ts = alias ? As : sm + DXH_TRI32 + DXH_VEC;
  stage(As, A + (size_t)b * DXH_TRI32, ti(n));
  stage(xs, x + (size_t)b * DXH_VEC, n);
  const DiagAdd dd = diag_add(as_table(d + (size_t)b * DXH_VEC), 1.0f, n);
  SYNC();
  mfma_chol_solve32(As, n, dd.d1, xs, Ts);
  dump_lds(out + (size_t)b * DXH_W_CHOL32, sm, DXH_W_CHOL32);
}

__global__ __launch_bounds__(64) void k_chol_solve64(const int* nn, const float* A, const float* d, const float* x,
                                                     int alias, unsigned fill, float* out) {
  __shared__ float sm[DXH_W_CHOL64];
  const int b = blockIdx.x, n = nn[b];
  fill_lds(sm, DXH_W_CHOL64, fill);
  float* As = sm;
  float* xs = sm + DXH_TRI64;
  float* Ts = alias ? As : sm + DXH_TRI64 + DXH_VEC;
  stage(As, A + (size_t)b * DXH_TRI64, ti(n));
  stage(xs, x + (size_t)b * DXH_VEC, n);
  const DiagAdd dd = diag_add(as_table(d + (size_t)b * DXH_VEC), 1.0f, n);
  SYNC();
  mfma_chol_solve64(As, n, dd.d1, dd.d2, xs, Ts);
  dump_lds(out + (size_t)b * DXH_W_CHOL64, sm, DXH_W_CHOL64);
}

__global__ __launch_bounds__(64) void k_sweep_inverse30(const int* nn, const float* A, unsigned fill, float* out) {
  __shared__ float sm[DXH_W_INV];
  const int b = blockIdx.x, n = nn[b];
  fill_lds(sm, DXH_W_INV, fill);
  stage(sm, A + (size_t)b * DXH_TRI32, ti(n));
  SYNC();
  mfma_sweep_inverse30(sm, n, sm + DXH_TRI32);
  dump_lds(out + (size_t)b * DXH_W_INV, sm, DXH_W_INV);
}

__global__ __launch_bounds__(64) void k_chol_factor30(const int* nn, const float* A, unsigned fill, float* out) {
  __shared__ float sm[DXH_W_FACTOR];
  const int b = blockIdx.x, n = nn[b];
  fill_lds(sm, DXH_W_FACTOR, fill);
  stage(sm, A + (size_t)b * DXH_TRI32, ti(n));
  SYNC();
  mfma_chol_factor30(sm, n);
  dump_lds(out + (size_t)b * DXH_W_FACTOR, sm, DXH_W_FACTOR);
}

// tree_solve's context: the dof count and a model of which only the item table is set
struct TreeCtx {
  int nv;
  DevModel m;
  __device__ const DevModel& mdl() const { return m; }
};
// tab: [ncase][DX_LDL_SLOTS][64] items, nslot / sync: [ncase]
__global__ __launch_bounds__(64) void k_tree_solve(const int* nn, const int* nslot, const unsigned* sync, const int* tab,
                                                   const float* A, const float* d, const float* x, unsigned fill,
                                                   float* out) {
  __shared__ float sm[DXH_W_TREE];
  const int b = blockIdx.x, n = nn[b];
  fill_lds(sm, DXH_W_TREE, fill);
  float* As = sm;
  float* xs = sm + DXH_TRI64;
  float* Ts = sm + DXH_TRI64 + DXH_VEC;
  stage(As, A + (size_t)b * DXH_TRI64, ti(n));
  stage(xs, x + (size_t)b * DXH_VEC, n);
  TreeCtx c;
  c.nv = n;
  c.m.ldl_nslot = nslot[b];
  c.m.ldl_sync = sync[b];
  c.m.ldl_tab = (const DXG int*)(tab + (size_t)b * DX_LDL_SLOTS * DX_WAVE);
  // m_solve's per-lane add: lane l carries dof l's (d1 in lanes 0-31, d2 in lanes 32-63)
  const DiagAdd dd = diag_add(as_table(d + (size_t)b * DXH_VEC), 1.0f, n);
  SYNC();
  tree_solve(c, As, LANE < 32 ? dd.d1 : dd.d2, xs, Ts);
  dump_lds(out + (size_t)b * DXH_W_TREE, sm, DXH_W_TREE);
}

// the tile loaded exactly as mfma_chol_solve32 loads it (dj = 0); ok: [ncase]
__global__ __launch_bounds__(64) void k_chol_pivots32(const int* nn, const float* A, const float* thr, unsigned fill,
                                                      int* ok) {
  __shared__ float sm[DXH_TRI32];
  const int b = blockIdx.x, n = nn[b];
  fill_lds(sm, DXH_TRI32, fill);
  stage(sm, A + (size_t)b * DXH_TRI32, ti(n));
  SYNC();
  const int l = LANE;
  const int j = l & 31, hi = l >> 5;
  dx_f16v C;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int i = 8 * (v >> 2) + 4 * hi + (v & 3);
    const int ra = max(i, j), rb = min(i, j);
    const bool in = i < n && j < n;
    C[v] = in ? sm[ti(ra) + rb] : (i == j ? 1.f : 0.f);
  }
  const bool r = mfma_chol_pivots32(C, n, thr[b]);
  ok[(size_t)b * DX_WAVE + l] = r ? 1 : 0;
}

// P: [ncase][64][30] (lane k: row k), diag: [ncase][64], full: [ncase]; out: [ncase][64 lanes][64]
__global__ __launch_bounds__(64) void k_pgs_gram64(const float* P, const float* diag, const int* full, float* out) {
  const int b = blockIdx.x, l = LANE;
  float p[30], o[64];
#pragma unroll
  for (int k = 0; k < 30; k++) p[k] = P[((size_t)b * DX_WAVE + l) * 30 + k];
  pgs_gram64(p, diag[(size_t)b * DX_WAVE + l], full[b] != 0, o);
#pragma unroll
  for (int r = 0; r < 64; r++) out[((size_t)b * DX_WAVE + l) * 64 + r] = o[r];
}

// t: [ncase][64 lanes][32]; out: [ncase][64]
__global__ __launch_bounds__(64) void k_reduce_scatter32(const float* t, float* out) {
  const int b = blockIdx.x, l = LANE;
  float v[32];
#pragma unroll
  for (int k = 0; k < 32; k++) v[k] = t[((size_t)b * DX_WAVE + l) * 32 + k];
  out[(size_t)b * DX_WAVE + l] = wave_reduce_scatter32(v);
}

// iv, fv, bi: [ncase][64]; out: [ncase][8][64] words: wave_sum_i, wave_max_i, wave_min_i,
// wave_incl_scan, wave_excl_scan of iv; wave_sum, wave_max_f of fv; wave_argmax_first(fv, bi)
__global__ __launch_bounds__(64) void k_wave_ops(const int* iv, const float* fv, const int* bi, int* out) {
  const int b = blockIdx.x, l = LANE;
  const int x = iv[(size_t)b * DX_WAVE + l];
  const float f = fv[(size_t)b * DX_WAVE + l];
  const int ix = bi[(size_t)b * DX_WAVE + l];
  int* o = out + (size_t)b * 8 * DX_WAVE + l;
  o[0 * DX_WAVE] = wave_sum_i(x);
  o[1 * DX_WAVE] = wave_max_i(x);
  o[2 * DX_WAVE] = wave_min_i(x);
  o[3 * DX_WAVE] = wave_incl_scan(x);
  o[4 * DX_WAVE] = wave_excl_scan(x);
  o[5 * DX_WAVE] = __float_as_int(wave_sum(f));
  o[6 * DX_WAVE] = __float_as_int(wave_max_f(f));
  o[7 * DX_WAVE] = wave_argmax_first(f, ix);
}

// ---- host side ----
struct Dev {  // device buffers of one call, freed on every path
  std::vector<void*> p;
  hipError_t err = hipSuccess;
  ~Dev() {
    for (void* q : p) (void)hipFree(q);
  }
  template <class T>
  T* in(const T* host, size_t count) {
    T* d = out<T>(count);
    if (err == hipSuccess && count) err = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  T* out(size_t count) {
    void* d = nullptr;
    if (err == hipSuccess) {
      err = hipMalloc(&d, (count ? count : 1) * sizeof(T));
      if (err == hipSuccess) p.push_back(d);
    }
    return (T*)d;
  }
  template <class T>
  int finish(T* host, const T* dev, size_t count) {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost);
    return (int)err;
  }
};
bool sizes_ok(int ncase, const int* n, int lo, int hi) {
  if (ncase < 1 || !n) return false;
  for (int b = 0; b < ncase; b++)
    if (n[b] < lo || n[b] > hi) return false;
  return true;
}

}  // namespace

extern "C" {

#ifndef DXH_BUILD_KEY
#define DXH_BUILD_KEY "unkeyed"
#endif
// hash of the sources and flags this library was built from (tests/linalg_harness.py
// source_key looks for the tagged string in the file, so nothing has to be loaded)
const char* dxh_build_key() {
  static const char tagged[] = "DXH_KEY:" DXH_BUILD_KEY;
  return tagged + 8;
}
int dxh_lane_range_mask() { return DX_LANE_RANGE_MASK; }
int dxh_ldl_slots() { return DX_LDL_SLOTS; }

int dxh_sweep_solve30(int ncase, const int* n, const float* A, const float* d, const float* x, unsigned fill,
                      float* lds) {
  if (!sizes_ok(ncase, n, 1, 30)) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto dn = D.in(n, N);
  auto dA = D.in(A, N * DXH_TRI32);
  auto dd = D.in(d, N * DXH_VEC);
  auto dx = D.in(x, N * DXH_VEC);
  auto dout = D.out<float>(N * DXH_W_SWEEP);
  if (D.err == hipSuccess) hipLaunchKernelGGL(k_sweep_solve30, dim3(ncase), dim3(64), 0, 0, dn, dA, dd, dx, fill, dout);
  return D.finish(lds, dout, N * DXH_W_SWEEP);
}

int dxh_chol_solve32(int ncase, const int* n, const float* A, const float* d, const float* x, int alias,
                     unsigned fill, float* lds) {
  if (!sizes_ok(ncase, n, 1, 32)) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto dn = D.in(n, N);
  auto dA = D.in(A, N * DXH_TRI32);
  auto dd = D.in(d, N * DXH_VEC);
  auto dx = D.in(x, N * DXH_VEC);
  auto dout = D.out<float>(N * DXH_W_CHOL32);
  if (D.err == hipSuccess)
    hipLaunchKernelGGL(k_chol_solve32, dim3(ncase), dim3(64), 0, 0, dn, dA, dd, dx, alias, fill, dout);
  return D.finish(lds, dout, N * DXH_W_CHOL32);
}

int dxh_chol_solve64(int ncase, const int* n, const float* A, const float* d, const float* x, int alias,
                     unsigned fill, float* lds) {
  if (!sizes_ok(ncase, n, 33, 64)) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto dn = D.in(n, N);
  auto dA = D.in(A, N * DXH_TRI64);
  auto dd = D.in(d, N * DXH_VEC);
  auto dx = D.in(x, N * DXH_VEC);
  auto dout = D.out<float>(N * DXH_W_CHOL64);
  if (D.err == hipSuccess)
    hipLaunchKernelGGL(k_chol_solve64, dim3(ncase), dim3(64), 0, 0, dn, dA, dd, dx, alias, fill, dout);
  return D.finish(lds, dout, N * DXH_W_CHOL64);
}

int dxh_sweep_inverse30(int ncase, const int* n, const float* A, unsigned fill, float* lds) {
  if (!sizes_ok(ncase, n, 1, 30)) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto dn = D.in(n, N);
  auto dA = D.in(A, N * DXH_TRI32);
  auto dout = D.out<float>(N * DXH_W_INV);
  if (D.err == hipSuccess) hipLaunchKernelGGL(k_sweep_inverse30, dim3(ncase), dim3(64), 0, 0, dn, dA, fill, dout);
  return D.finish(lds, dout, N * DXH_W_INV);
}

int dxh_chol_factor30(int ncase, const int* n, const float* A, unsigned fill, float* lds) {
  if (!sizes_ok(ncase, n, 1, 30)) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto dn = D.in(n, N);
  auto dA = D.in(A, N * DXH_TRI32);
  auto dout = D.out<float>(N * DXH_W_FACTOR);
  if (D.err == hipSuccess) hipLaunchKernelGGL(k_chol_factor30, dim3(ncase), dim3(64), 0, 0, dn, dA, fill, dout);
  return D.finish(lds, dout, N * DXH_W_FACTOR);
}

int dxh_tree_solve(int ncase, const int* n, const int* nslot, const unsigned* sync, const int* tab, const float* A,
                   const float* d, const float* x, unsigned fill, float* lds) {
  if (!sizes_ok(ncase, n, 1, 64) || !nslot || !tab) return DXH_EINVAL;
  for (int b = 0; b < ncase; b++) {  // every item must index inside the n x n triangle
    if (nslot[b] < 0 || nslot[b] > DX_LDL_SLOTS) return DXH_EINVAL;
    for (int s = 0; s < nslot[b] * DX_WAVE; s++) {
      const int t = tab[(size_t)b * DX_LDL_SLOTS * DX_WAVE + s];
      if (t == -1) continue;
      const int k = t & 255, i = (t >> 8) & 255, j = t >> 16;
      if (t < 0 || k >= n[b] || i >= k || j > i) return DXH_EINVAL;
    }
  }
  Dev D;
  const size_t N = (size_t)ncase;
  auto dn = D.in(n, N);
  auto dns = D.in(nslot, N);
  auto dsy = D.in(sync, N);
  auto dtab = D.in(tab, N * DX_LDL_SLOTS * DX_WAVE);
  auto dA = D.in(A, N * DXH_TRI64);
  auto dd = D.in(d, N * DXH_VEC);
  auto dx = D.in(x, N * DXH_VEC);
  auto dout = D.out<float>(N * DXH_W_TREE);
  if (D.err == hipSuccess)
    hipLaunchKernelGGL(k_tree_solve, dim3(ncase), dim3(64), 0, 0, dn, dns, dsy, dtab, dA, dd, dx, fill, dout);
  return D.finish(lds, dout, N * DXH_W_TREE);
}

int dxh_chol_pivots32(int ncase, const int* n, const float* A, const float* thr, unsigned fill, int* ok) {
  if (!sizes_ok(ncase, n, 1, 32)) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto dn = D.in(n, N);
  auto dA = D.in(A, N * DXH_TRI32);
  auto dt = D.in(thr, N);
  auto dout = D.out<int>(N * DX_WAVE);
  if (D.err == hipSuccess) hipLaunchKernelGGL(k_chol_pivots32, dim3(ncase), dim3(64), 0, 0, dn, dA, dt, fill, dout);
  return D.finish(ok, dout, N * DX_WAVE);
}

int dxh_pgs_gram64(int ncase, const float* P, const float* diag, const int* full, float* out) {
  if (ncase < 1) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto dP = D.in(P, N * DX_WAVE * 30);
  auto dg = D.in(diag, N * DX_WAVE);
  auto df = D.in(full, N);
  auto dout = D.out<float>(N * DX_WAVE * 64);
  if (D.err == hipSuccess) hipLaunchKernelGGL(k_pgs_gram64, dim3(ncase), dim3(64), 0, 0, dP, dg, df, dout);
  return D.finish(out, dout, N * DX_WAVE * 64);
}

int dxh_reduce_scatter32(int ncase, const float* t, float* out) {
  if (ncase < 1) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto dt = D.in(t, N * DX_WAVE * 32);
  auto dout = D.out<float>(N * DX_WAVE);
  if (D.err == hipSuccess) hipLaunchKernelGGL(k_reduce_scatter32, dim3(ncase), dim3(64), 0, 0, dt, dout);
  return D.finish(out, dout, N * DX_WAVE);
}

int dxh_wave_ops(int ncase, const int* iv, const float* fv, const int* bi, int* out) {
  if (ncase < 1) return DXH_EINVAL;
  Dev D;
  const size_t N = (size_t)ncase;
  auto di = D.in(iv, N * DX_WAVE);
  auto df = D.in(fv, N * DX_WAVE);
  auto db = D.in(bi, N * DX_WAVE);
  auto dout = D.out<int>(N * 8 * DX_WAVE);
  if (D.err == hipSuccess) hipLaunchKernelGGL(k_wave_ops, dim3(ncase), dim3(64), 0, 0, di, df, db, dout);
  return D.finish(out, dout, N * 8 * DX_WAVE);
}

}  // extern "C"
