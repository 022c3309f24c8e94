// dx_mtw.h -- wave-cooperative numpy RandomState draws (mtw_*), shared by the step kernel's
// reach sampling pass (dx_step.hip) and the action filter (dx_task.hip).  The including
// translation unit provides LANE (the lane's index in its wave), DX_WAVE, SYNC() (a wave
// barrier) and dx_internal.h; every wave works on LDS of its own.
#pragma once

// numpy RandomState draws for one env, by the whole wave ([3P] numpy legacy MT19937:
// mt19937_gen, legacy_double, legacy_gauss).  The env's 624-word state block is copied
// to LDS scratch (the collision candidate area, free before a pass), outputs pos.. are
// tempered in parallel, and a block that runs out is twisted in place in LDS: chunks
// of 64 in index order, each chunk's loads before its stores, which is the serial
// loop's dependency order (new[k] needs new[k - 227] for k >= 227, new[0] for k = 623).
// The block goes back to HBM only when the draws really consumed past it.
__device__ __forceinline__ void mtw_twist(uint32_t* sm) {
  for (int base = 0; base < 624; base += DX_WAVE) {
    const int k = base + LANE;
    uint32_t a = 0, b = 0, c = 0;
    if (k < 624) { a = sm[k]; b = sm[(k + 1) % 624]; c = sm[(k + 397) % 624]; }
    SYNC();
    if (k < 624) {
      const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
      sm[k] = c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    SYNC();
  }
}
struct MtWave {
  uint32_t* g;   // the env's HBM block (DX_MTW_WORDS)
  uint32_t* sm;  // 624 words of LDS
  int pos;       // read position in the current block (uniform)
  bool twisted;  // LDS holds the next block
};
__device__ __forceinline__ MtWave mtw_begin(uint32_t* g, uint32_t* sm) {
  MtWave w;
  w.g = g;
  w.sm = sm;
  // this wave may have rewritten the block earlier in the launch: invalidate the vector
  // L1 so the reloads see those stores
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  for (int k = LANE; k < 624; k += DX_WAVE) sm[k] = g[k];
  w.pos = (int)g[624];
  w.twisted = false;
  SYNC();
  return w;
}
// Outputs [pos, pos + n) of the stream, lane j gets outputs pos + stride*j + t, t < cnt
// (cnt <= 4, n = stride * 64 at most 624); advances pos by `used` (<= n) afterwards
// through mtw_consume.
__device__ __forceinline__ void mtw_fetch(MtWave& w, int stride, int cnt, uint32_t* out) {
  const int n = stride * DX_WAVE;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int q = w.pos + stride * LANE + t;
    out[t] = (t < cnt && q < 624) ? dx_mt_temper(w.sm[q]) : 0u;
  }
  if (w.pos + n > 624) {  // part of the batch lies in the next block
    SYNC();
    mtw_twist(w.sm);
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int q = w.pos + stride * LANE + t;
      if (t < cnt && q >= 624) out[t] = dx_mt_temper(w.sm[q - 624]);
    }
    w.twisted = true;
  }
}
__device__ __forceinline__ void mtw_consume(MtWave& w, int used) {
  if (w.twisted && w.pos + used >= 624) {
    w.pos = w.pos + used - 624;
    for (int k = LANE; k < 624; k += DX_WAVE) w.g[k] = w.sm[k];
  } else if (w.twisted) {  // speculative twist: the stream is still in the old block
    for (int k = LANE; k < 624; k += DX_WAVE) w.sm[k] = w.g[k];
    w.pos += used;
  } else {
    w.pos += used;
  }
  w.twisted = false;
  if (LANE == 0) w.g[624] = (uint32_t)w.pos;
  SYNC();
}
__device__ __forceinline__ double mt_to_double(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}
// RandomState.uniform(lo, hi) for lanes < n: lo + (hi - lo) * random_sample()
__device__ __forceinline__ double mtw_uniform(MtWave& w, int n, double lo, double hi) {
  uint32_t o[4];
  mtw_fetch(w, 2, 2, o);
  const double u = mt_to_double(o[0], o[1]);
  mtw_consume(w, 2 * n);
  return __dadd_rn(lo, __dmul_rn(hi - lo, u));
}
// RandomState.normal(loc, scale) for lanes < n (legacy_gauss: polar pairs, the second
// value of a pair cached in the state for the next call).  Candidate pairs come 64 at
// a time (lane j: outputs 4j..4j+3); accepted ones are ranked by a ballot.
__device__ __forceinline__ double mtw_normal(MtWave& w, int n, double loc, double scale, double* pairs) {
  int has = (int)w.g[625];
  double cached;
  {
    const uint64_t lo32 = w.g[626], hi32 = w.g[627];
    cached = __longlong_as_double((long long)(lo32 | (hi32 << 32)));
  }
  const int need = n - has;          // gaussians to draw from pairs
  const int npairs = (need + 1) / 2;
  int got = 0;
  while (got < npairs) {
    uint32_t o[4];
    mtw_fetch(w, 4, 4, o);
    const double x1 = 2.0 * mt_to_double(o[0], o[1]) - 1.0;
    const double x2 = 2.0 * mt_to_double(o[2], o[3]) - 1.0;
    const double r2 = __dadd_rn(__dmul_rn(x1, x1), __dmul_rn(x2, x2));
    const bool acc = r2 < 1.0 && r2 != 0.0;
    const uint64_t m = __ballot(acc);
    const int rank = got + __popcll(m & ((1ull << LANE) - 1ull));
    if (acc && rank < npairs) {
      const double f = sqrt(-2.0 * log(r2) / r2);
      pairs[2 * rank] = __dmul_rn(f, x2);      // returned first
      pairs[2 * rank + 1] = __dmul_rn(f, x1);  // cached for the next call
    }
    const int take = min(npairs - got, __popcll(m));
    int used = 4 * DX_WAVE;  // the whole batch unless the last needed pair is in it
    if (take == npairs - got) {
      // lane index of the take-th accepted candidate
      uint64_t mm = m;
      for (int t = 1; t < take; t++) mm &= mm - 1;
      used = 4 * (__ffsll((long long)mm) - 1 + 1);
    }
    got += take;
    mtw_consume(w, used);
  }
  SYNC();
  const int i = LANE;
  double g = 0.0;
  if (i < n) g = (has && i == 0) ? cached : pairs[i - has];
  // state: a leftover second value of the last pair stays cached
  if (LANE == 0 && n > 0) {  // the cached value (if any) was used; an odd count leaves one
    const bool odd = (need & 1) != 0;
    const uint64_t bits = (uint64_t)__double_as_longlong(odd ? pairs[need] : 0.0);
    w.g[625] = odd ? 1u : 0u;
    w.g[626] = (uint32_t)bits;
    w.g[627] = (uint32_t)(bits >> 32);
  }
  SYNC();
  return __dadd_rn(loc, __dmul_rn(scale, g));
}
