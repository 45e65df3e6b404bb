// intra.hip -- AV1 intra prediction for a list of jobs, batched for gfx950.
// All integer, bit-exact:
//   build_intra_predictors[_high]                 av1/common/reconintra.c:1133-1477
//   the dc / v / h / paeth / smooth predictors    aom_dsp/intrapred.c
//   av1_[highbd_]dr_prediction_z{1,2,3}           reconintra.c:519-764
//   av1_filter_intra_predictor, its highbd twin   reconintra.c:847-943
//   intra_edge_filter_strength, filter_intra_edge_corner,
//   av1_filter_intra_edge[_high], av1_upsample_intra_edge[_high]   reconintra.c:979-1131
//
// Layout (as blend.hip / pixel_comp.hip): a job's rows are cut into chunks of
// 16 bytes (a whole row where it is narrower), and a job takes a group of
// min(64, chunks) lanes of one wave: a 4x4 job 4 lanes, a 64x64 job the wave.
// Jobs of any size mix in a call and the list is device memory, so the groups
// are formed on the device: a workgroup of 8 waves owns 16 consecutive jobs.
// Where their groups fit 64 lanes together (16 jobs of 4x4) wave 0 runs them
// all in one pass; otherwise every wave takes two of them and packs them, in
// order, into passes of at most 64 lanes (two 16x16 jobs make one pass, two
// 64x64 two).  Each job owns an LDS slice for the two edges
// (160 entries each, NUM_INTRA_NEIGHBOUR_PIXELS, with room for the in-place
// upsample) and 22 entries per lane of scratch: the copy the edge filter and
// the upsampler read, the DC partial sums, or filter intra's (w + 1) x (h + 1)
// buffer.  Lanes of a group only ever synchronise with each other, and they
// take the same branches, so wave-level ordering is enough; no barrier.
//
// A job loads exactly the pixels its counts declare available, all of them
// before its first store.
#include "intra_tables.h"
#include "lavish_internal.h"

namespace lavish {
namespace {

static_assert(sizeof(LavishIntraJob) == 48, "LavishIntraJob layout");

constexpr int kEdgeLen = 160;  // NUM_INTRA_NEIGHBOUR_PIXELS
constexpr int kEdge0 = 16;     // above_row / left_col start here
constexpr int kJobsPerWg = 16;
constexpr int kWaves = 8;
constexpr int kJobsPerWave = kJobsPerWg / kWaves;  // when the 16 jobs do not fit one wave
// Scratch entries per lane.  Filter intra needs (w + 1)(h + 1) entries from a
// group of min(64, chunks) lanes; the worst ratio is the 8-bit 16x4 job's,
// 85 entries on 4 lanes.  The two edge copies need 2 (w + h + 1) at most,
// which is less for every size.
constexpr int kScratchPerLane = 22;

static const uint8_t kTxWide[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
static const uint8_t kTxHigh[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};

enum { DC_PRED = 0, V_PRED, H_PRED, D45_PRED, D135_PRED, D113_PRED, D157_PRED, D203_PRED,
       D67_PRED, SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, PAETH_PRED, INTRA_MODES };
constexpr int kFilterIntraModes = 5;

enum Kind { K_FILL, K_V, K_H, K_PAETH, K_SMOOTH, K_SMOOTH_V, K_SMOOTH_H, K_Z1, K_Z2, K_Z3, K_BUF };

// what the pixel loop evaluates, the same for every lane of a job
struct Pred {
  int kind, w, h;
  int val;     // K_FILL
  int ua, ul;  // upsample_above / upsample_left
  int dx, dy;
};

struct Grp {
  int q, n;  // this lane's index in its job's group, and the group's size
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// pixels per chunk and lanes per job of a w x h block of T
template <typename T>
__device__ __host__ __forceinline__ int chunk_px(int w) {
  constexpr int n = 16 / (int)sizeof(T);
  return w < n ? w : n;
}
template <typename T>
__device__ __forceinline__ int lanes_of(int w, int h) {
  const int chunks = w * h / chunk_px<T>(w);
  return chunks < 64 ? chunks : 64;
}

// ------------------------------------------------------------ edge filters --
__device__ __forceinline__ int filter_strength(int bs0, int bs1, int delta, int type) {
  const int d = delta < 0 ? -delta : delta, wh = bs0 + bs1;
  if (type == 0) {
    if (wh <= 8) return d >= 56;
    if (wh <= 16) return d >= 40;
    if (wh <= 24) return d >= 32 ? 3 : d >= 16 ? 2 : d >= 8;
    if (wh <= 32) return d >= 32 ? 3 : d >= 4 ? 2 : d >= 1;
    return d >= 1 ? 3 : 0;
  }
  if (wh <= 8) return d >= 64 ? 2 : d >= 40;
  if (wh <= 16) return d >= 48 ? 2 : d >= 20;
  if (wh <= 24) return d >= 4 ? 3 : 0;
  return d >= 1 ? 3 : 0;
}

__device__ __forceinline__ int use_upsample(int bs0, int bs1, int delta, int type) {
  const int d = delta < 0 ? -delta : delta;
  if (d == 0 || d >= 40) return 0;
  return type ? bs0 + bs1 <= 8 : bs0 + bs1 <= 16;
}

// av1_filter_intra_edge on p[0 .. sz): one lane per element, from the copy cp
template <typename T>
__device__ __forceinline__ void filter_edge(T* p, int sz, int strength, T* cp, Grp g) {
  if (!strength) return;
  for (int i = g.q; i < sz; i += g.n) cp[i] = p[i];
  wave_sync();
  for (int i = 1 + g.q; i < sz; i += g.n) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) s += (int)cp[clampi(i - 2 + j, 0, sz - 1)] * kIntraEdgeKernel[strength - 1][j];
    p[i] = (T)((s + 8) >> 4);
  }
  wave_sync();
}

// av1_upsample_intra_edge: reads p[-1 .. sz), writes p[-2 .. 2 sz - 2]
template <typename T>
__device__ __forceinline__ void upsample_edge(T* p, int sz, int maxv, T* cp, Grp g) {
  for (int i = g.q; i < sz + 3; i += g.n) cp[i] = p[i < 2 ? -1 : i - 2 < sz ? i - 2 : sz - 1];
  wave_sync();
  if (g.q == 0) p[-2] = cp[0];
  for (int i = g.q; i < sz; i += g.n) {
    const int s = -(int)cp[i] + 9 * (int)cp[i + 1] + 9 * (int)cp[i + 2] - (int)cp[i + 3];
    p[2 * i - 1] = (T)clampi((s + 8) >> 4, 0, maxv);
    p[2 * i] = cp[i + 2];
  }
  wave_sync();
}

// sum of v over the job's group, through sc[0 .. g.n)
template <typename T>
__device__ __forceinline__ int group_total(int v, int* sc, Grp g) {
  sc[g.q] = v;
  for (int off = g.n >> 1; off > 0; off >>= 1) {
    wave_sync();
    if (g.q < off) sc[g.q] += sc[g.q + off];
  }
  wave_sync();
  const int t = sc[0];
  wave_sync();
  return t;
}

// ----------------------------------------------------------------- pixels --
__device__ __forceinline__ int interp(int a, int b, int shift) {
  return (a * (32 - shift) + b * shift + 16) >> 5;
}

template <typename T>
__device__ __forceinline__ int pixel(const Pred& p, const T* A, const T* L, const T* fb, int x, int y) {
  switch (p.kind) {
    case K_FILL: return p.val;
    case K_V: return A[x];
    case K_H: return L[y];
    case K_PAETH: {
      const int l = L[y], t = A[x], tl = A[-1];
      const int base = t + l - tl;
      const int pl = abs(base - l), pt = abs(base - t), ptl = abs(base - tl);
      return (pl <= pt && pl <= ptl) ? l : (pt <= ptl) ? t : tl;
    }
    case K_SMOOTH: {
      const int wh = kSmoothWeights[p.h - 4 + y], ww = kSmoothWeights[p.w - 4 + x];
      return (wh * A[x] + (256 - wh) * L[p.h - 1] + ww * L[y] + (256 - ww) * A[p.w - 1] + 256) >> 9;
    }
    case K_SMOOTH_V: {
      const int wh = kSmoothWeights[p.h - 4 + y];
      return (wh * A[x] + (256 - wh) * L[p.h - 1] + 128) >> 8;
    }
    case K_SMOOTH_H: {
      const int ww = kSmoothWeights[p.w - 4 + x];
      return (ww * L[y] + (256 - ww) * A[p.w - 1] + 128) >> 8;
    }
    case K_Z1: {
      const int xx = p.dx * (y + 1);
      const int base = (xx >> (6 - p.ua)) + (x << p.ua);
      const int mb = (p.w + p.h - 1) << p.ua;
      return base < mb ? interp(A[base], A[base + 1], ((xx << p.ua) & 0x3F) >> 1) : A[mb];
    }
    case K_Z3: {
      const int yy = p.dy * (x + 1);
      const int base = (yy >> (6 - p.ul)) + (y << p.ul);
      const int mb = (p.w + p.h - 1) << p.ul;
      return base < mb ? interp(L[base], L[base + 1], ((yy << p.ul) & 0x3F) >> 1) : L[mb];
    }
    case K_Z2: {
      const int xx = (x << 6) - (y + 1) * p.dx;
      const int bx = xx >> (6 - p.ua);
      if (bx >= -(1 << p.ua)) return interp(A[bx], A[bx + 1], ((xx * (1 << p.ua)) & 0x3F) >> 1);
      const int yy = (y << 6) - (x + 1) * p.dy;
      const int by = yy >> (6 - p.ul);
      return interp(L[by], L[by + 1], ((yy * (1 << p.ul)) & 0x3F) >> 1);
    }
    default: return fb[(y + 1) * (p.w + 1) + x + 1];  // K_BUF: filter intra's buffer
  }
}

// the block: a lane takes whole chunks, one 4 / 8 / 16-byte store each
template <typename T>
__device__ __forceinline__ void write_block(const Pred& p, const T* A, const T* L, const T* fb,
                                            T* dst, int ds, bool live, Grp g) {
  constexpr int N = 16 / (int)sizeof(T);
  const int pc = chunk_px<T>(p.w);
  const int lcpr = __builtin_ctz(p.w / pc), chunks = p.h << lcpr;  // chunks per row: a power of two
  for (int i = g.q; i < chunks; i += g.n) {
    const int y = i >> lcpr, x = (i & ((1 << lcpr) - 1)) * pc;
    uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const uint32_t v = u < pc ? (uint32_t)pixel(p, A, L, fb, x + u, y) : 0u;
      if constexpr (sizeof(T) == 1) wd[u >> 2] |= v << (8 * (u & 3));
      else wd[u >> 1] |= v << (16 * (u & 1));
    }
    if (!live) continue;
    T* o = dst + (int64_t)y * ds + x;
    const int bytes = pc * (int)sizeof(T);
    if (bytes == 16) {
      u32x4u t;
      t.x = wd[0]; t.y = wd[1]; t.z = wd[2]; t.w = wd[3];
      *(__attribute__((address_space(1))) u32x4u*)o = t;
    } else if (bytes == 8) {
      u32x2u t;
      t.x = wd[0]; t.y = wd[1];
      *(__attribute__((address_space(1))) u32x2u*)o = t;
    } else {
      *(__attribute__((address_space(1))) u32u*)o = wd[0];
    }
  }
}

// av1_filter_intra_predictor into fb, (h + 1) rows of w + 1: the 4x2 units of
// one anti-diagonal depend only on earlier diagonals, so they run together
template <typename T>
__device__ __forceinline__ void filter_intra(const T* A, const T* L, T* fb, int w, int h, int mode,
                                             int maxv, Grp g) {
  const int pitch = w + 1;
  for (int i = g.q; i <= w; i += g.n) fb[i] = A[i - 1];
  for (int i = g.q; i < h; i += g.n) fb[(i + 1) * pitch] = L[i];
  const int uw = w >> 2, uh = h >> 1;
  for (int d = 0; d < uw + uh - 1; ++d) {
    wave_sync();
    const int r0 = d < uw ? 0 : d - uw + 1;         // first unit row of the diagonal
    const int r1 = d < uh ? d : uh - 1;             // last
    for (int ur = r0 + g.q; ur <= r1; ur += g.n) {
      const int r = 1 + 2 * ur, c = 1 + 4 * (d - ur);
      const T* up = fb + (r - 1) * pitch + c - 1;
      const int p0 = up[0], p1 = up[1], p2 = up[2], p3 = up[3], p4 = up[4];
      const int p5 = fb[r * pitch + c - 1], p6 = fb[(r + 1) * pitch + c - 1];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int8_t* t = kFilterIntraTaps[mode][k];
        const int pr = t[0] * p0 + t[1] * p1 + t[2] * p2 + t[3] * p3 + t[4] * p4 + t[5] * p5 + t[6] * p6;
        fb[(r + (k >> 2)) * pitch + c + (k & 3)] = (T)clampi((pr + 8) >> 4, 0, maxv);
      }
    }
  }
  wave_sync();
}

// ------------------------------------------------------------------ a job --
// ae / le: the group's two 160-entry edge buffers; sc: its scratch
template <typename T>
__device__ __forceinline__ void intra_job(const T* ref, int rs, T* dst, int ds,
                                          const LavishIntraJob& jb, int bd, bool live, T* ae,
                                          T* le, T* sc, Grp g) {
  const int w = kTxWide[jb.tx_size], h = kTxHigh[jb.tx_size];
  const int mode = jb.mode, p_angle = jb.p_angle;
  const int base = 128 << (bd - 8), maxv = (1 << bd) - 1;
  const bool use_fi = jb.filter_intra_mode != kFilterIntraModes;
  const bool is_dr = mode >= V_PRED && mode <= D67_PRED;
  for (int i = g.q; i < kEdgeLen; i += g.n) {
    ae[i] = (T)(base - 1);
    le[i] = (T)(base + 1);
  }
  wave_sync();
  T* A = ae + kEdge0;
  T* L = le + kEdge0;
  bool need_left = true, need_above = true, need_al = mode == PAETH_PRED;  // extend_modes
  if (is_dr) {
    need_above = p_angle < 180;
    need_left = p_angle > 90;
    need_al = true;
  }
  if (use_fi) need_left = need_above = need_al = true;
  // counts: never above the dimension; a corner run only next to a full edge
  const int nt = clampi(jb.n_top_px, 0, w), nl = clampi(jb.n_left_px, 0, h);
  int ntr = jb.n_topright_px, nbl = jb.n_bottomleft_px;
  if (ntr > 0) ntr = nt == w ? (ntr < h ? ntr : h) : 0;  // only w + h entries are ever used
  if (nbl > 0) nbl = nl == h ? (nbl < w ? nbl : w) : 0;
  const T* above_ref = ref + jb.ref_off - rs;
  const T* left_ref = ref + jb.ref_off - 1;
  Pred P;
  P.w = w; P.h = h; P.val = 0; P.ua = 0; P.ul = 0; P.dx = 1; P.dy = 1;
  T* d = dst + jb.dst_off;

  if ((!need_above && nl == 0) || (!need_left && nt == 0)) {
    P.kind = K_FILL;
    if (need_left) P.val = nt > 0 ? (int)above_ref[0] : base + 1;
    else P.val = nl > 0 ? (int)left_ref[0] : base - 1;
    write_block<T>(P, A, L, sc, d, ds, live, g);
    return;
  }
  if (need_left) {
    const int need_n = h + (nbl >= 0 ? w : 0);
    if (nl > 0) {
      const int have = nbl > 0 ? h + nbl : nl;  // then the last pixel repeats
      for (int i = g.q; i < need_n; i += g.n) L[i] = left_ref[(int64_t)(i < have ? i : have - 1) * rs];
    } else if (nt > 0) {
      const T v = above_ref[0];
      for (int i = g.q; i < need_n; i += g.n) L[i] = v;
    }
  }
  if (need_above) {
    const int need_n = w + (ntr >= 0 ? h : 0);
    if (nt > 0) {
      const int have = ntr > 0 ? w + ntr : nt;
      for (int i = g.q; i < need_n; i += g.n) A[i] = above_ref[i < have ? i : have - 1];
    } else if (nl > 0) {
      const T v = left_ref[0];
      for (int i = g.q; i < need_n; i += g.n) A[i] = v;
    }
  }
  if (need_al && g.q == 0) {
    const T v = (nt > 0 && nl > 0) ? above_ref[-1] : nt > 0 ? above_ref[0] : nl > 0 ? left_ref[0] : (T)base;
    A[-1] = v;
    L[-1] = v;
  }
  wave_sync();

  if (use_fi) {
    filter_intra<T>(A, L, sc, w, h, jb.filter_intra_mode, maxv, g);
    P.kind = K_BUF;
  } else if (is_dr) {
    if (!jb.disable_edge_filter) {
      const int type = jb.intra_edge_filter_type;
      const bool need_right = p_angle < 90, need_bottom = p_angle > 180;
      if (p_angle != 90 && p_angle != 180) {
        if (need_above && need_left && w + h >= 24) {  // filter_intra_edge_corner
          const int s = ((int)L[0] * 5 + (int)A[-1] * 6 + (int)A[0] * 5 + 8) >> 4;
          wave_sync();
          if (g.q == 0) {
            A[-1] = (T)s;
            L[-1] = (T)s;
          }
          wave_sync();
        }
        if (need_above && nt > 0)
          filter_edge<T>(A - 1, nt + 1 + (need_right ? h : 0), filter_strength(w, h, p_angle - 90, type), sc, g);
        if (need_left && nl > 0)
          filter_edge<T>(L - 1, nl + 1 + (need_bottom ? w : 0), filter_strength(h, w, p_angle - 180, type), sc, g);
      }
      P.ua = use_upsample(w, h, p_angle - 90, type);
      if (need_above && P.ua) upsample_edge<T>(A, w + (need_right ? h : 0), maxv, sc, g);
      P.ul = use_upsample(h, w, p_angle - 180, type);
      if (need_left && P.ul) upsample_edge<T>(L, h + (need_bottom ? w : 0), maxv, sc, g);
    }
    if (p_angle < 90) {
      P.kind = K_Z1;
      P.dx = kDrIntraDerivative[p_angle];
    } else if (p_angle == 90) {
      P.kind = K_V;
    } else if (p_angle < 180) {
      P.kind = K_Z2;
      P.dx = kDrIntraDerivative[180 - p_angle];
      P.dy = kDrIntraDerivative[p_angle - 90];
    } else if (p_angle == 180) {
      P.kind = K_H;
    } else {
      P.kind = K_Z3;
      P.dy = kDrIntraDerivative[270 - p_angle];
    }
  } else if (mode == DC_PRED) {
    P.kind = K_FILL;
    if (nt == 0 && nl == 0) {
      P.val = base;
    } else {
      int s = 0;
      if (nt > 0)
        for (int i = g.q; i < w; i += g.n) s += A[i];
      if (nl > 0)
        for (int i = g.q; i < h; i += g.n) s += L[i];
      s = group_total<T>(s, (int*)sc, g);
      if (nt > 0 && nl > 0) {
        if (w == h) {
          P.val = (s + w) >> __builtin_ctz(2 * w);
        } else {
          // divide_using_multiply_shift: w + h = 3 or 5 times a power of two
          const int shift1 = __builtin_ctz(w + h);
          const bool one_two = (w > h ? w : h) == 2 * (w > h ? h : w);
          const int mult = sizeof(T) == 1 ? (one_two ? 0x5556 : 0x3334) : (one_two ? 0xAAAB : 0x6667);
          P.val = (((s + ((w + h) >> 1)) >> shift1) * mult) >> (sizeof(T) == 1 ? 16 : 17);
        }
      } else {
        const int n = nt > 0 ? w : h;
        P.val = (s + (n >> 1)) >> __builtin_ctz(n);
      }
    }
  } else {
    P.kind = mode == SMOOTH_PRED ? K_SMOOTH : mode == SMOOTH_V_PRED ? K_SMOOTH_V
             : mode == SMOOTH_H_PRED ? K_SMOOTH_H : K_PAETH;
  }
  write_block<T>(P, A, L, sc, d, ds, live, g);
}

__device__ __forceinline__ bool job_ok(const LavishIntraJob& jb) {
  if (jb.tx_size > 18 || jb.mode >= INTRA_MODES || jb.filter_intra_mode > kFilterIntraModes) return false;
  if (jb.filter_intra_mode != kFilterIntraModes && (kTxWide[jb.tx_size] > 32 || kTxHigh[jb.tx_size] > 32))
    return false;
  if (jb.filter_intra_mode == kFilterIntraModes && jb.mode >= V_PRED && jb.mode <= D67_PRED) {
    // one of the 56 angles: the mode's base angle + 3 * delta, delta in -3 .. 3
    // (any other would read a zero dx / dy from the derivative table)
    const int d = jb.p_angle - kModeToAngle[jb.mode];
    if (d < -9 || d > 9 || d % 3 != 0) return false;
  }
  return true;
}

template <typename T>
__global__ __launch_bounds__(64 * kWaves) void intra_kernel(const T* ref, int rs, T* dst, int ds,
                                                            const LavishIntraJob* __restrict__ jobs,
                                                            int njobs, int bd) {
  __shared__ T edges[kJobsPerWg][2][kEdgeLen];  // a slice per job of the workgroup
  __shared__ __attribute__((aligned(4))) T scratch[kWaves][64 * kScratchPerLane];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j0 = blockIdx.x * kJobsPerWg;
  // lane k < 16 looks up the group size of job j0 + k (dead jobs: the last live one)
  int my_n;
  {
    const int j = j0 + (lane & 15);
    const int tx = jobs[j < njobs ? j : njobs - 1].tx_size;
    my_n = tx > 18 ? 4 : lanes_of<T>(kTxWide[tx], kTxHigh[tx]);
  }
  int total = 0;
  for (int k = 0; k < kJobsPerWg; ++k) total += __shfl(my_n, k);
  // 16 small jobs (16 of 4x4: 64 lanes) run as one pass of wave 0; otherwise
  // every wave takes two of them, so that large jobs spread over the waves
  int first = 0, last = kJobsPerWg;
  if (total > 64) {
    first = wave * kJobsPerWave;
    last = first + kJobsPerWave;
  } else if (wave != 0) {
    return;
  }
  if (j0 + first >= njobs) return;
  while (first < last) {
    // the jobs first .. first + cnt - 1 fit into the wave's 64 lanes
    int used = 0, cnt = 0, mine = -1, start = 0, n = 0;
    for (int k = first; k < last; ++k) {
      const int lp = __shfl(my_n, k);
      if (used + lp > 64) break;
      if (lane >= used && lane < used + lp) {
        mine = k;
        start = used;
        n = lp;
      }
      used += lp;
      ++cnt;
    }
    if (mine >= 0) {
      const int j = j0 + mine;
      const bool live = j < njobs;
      const LavishIntraJob jb = jobs[live ? j : njobs - 1];
      if (job_ok(jb))
        intra_job<T>(ref, rs, dst, ds, jb, bd, live, edges[mine][0], edges[mine][1],
                     scratch[wave] + start * kScratchPerLane, Grp{lane - start, n});
    }
    wave_sync();  // the next pass reuses the scratch
    first += cnt;
  }
}

// ------------------------------------------------- single-call kernels ----
// the z1 / z2 / z3 shims: above / left arrive finished, a[i] = above[a_lo + i]
template <typename T>
__global__ __launch_bounds__(64) void dr_single_kernel(T* dst, const T* a, int a_lo, int a_n,
                                                       const T* l, int l_lo, int l_n, Pred P) {
  __shared__ T ae[256 + kEdge0], le[256 + kEdge0];
  const Grp g{(int)threadIdx.x, 64};
  for (int i = g.q; i < a_n; i += 64) ae[kEdge0 + a_lo + i] = a[i];
  for (int i = g.q; i < l_n; i += 64) le[kEdge0 + l_lo + i] = l[i];
  __syncthreads();
  write_block<T>(P, ae + kEdge0, le + kEdge0, ae, dst, P.w, true, g);
}

// av1_filter_intra_edge (upsample = 0) / av1_upsample_intra_edge on p = buf + 2
template <typename T>
__global__ __launch_bounds__(64) void edge_single_kernel(T* buf, int n, int sz, int strength,
                                                         int upsample, int maxv) {
  __shared__ T e[kEdgeLen * 2], cp[kEdgeLen];
  const Grp g{(int)threadIdx.x, 64};
  for (int i = g.q; i < n; i += 64) e[i] = buf[i];
  __syncthreads();
  if (upsample) upsample_edge<T>(e + 2, sz, maxv, cp, g);
  else filter_edge<T>(e + 2, sz, strength, cp, g);
  __syncthreads();
  for (int i = g.q; i < n; i += 64) buf[i] = e[i];
}

#define LCHK() LAVISH_CHECK(hipGetLastError())

}  // namespace

int intra_dr_single(void* dst, const void* above, int a_lo, int a_n, const void* left, int l_lo,
                    int l_n, int zone, int w, int h, int ua, int ul, int dx, int dy, int highbd,
                    hipStream_t s) {
  if (zone < 1 || zone > 3 || w < 4 || h < 4 || w > 64 || h > 64 || (w & (w - 1)) || (h & (h - 1)))
    return -4;
  if ((ua | ul) & ~1) return -2;
  if (dx < 1 || dy < 1 || dx > 1023 || dy > 1023) return -2;
  if (a_lo < -kEdge0 || l_lo < -kEdge0 || a_lo + a_n > 256 || l_lo + l_n > 256) return -4;
  Pred P;
  P.kind = zone == 1 ? K_Z1 : zone == 2 ? K_Z2 : K_Z3;
  P.w = w; P.h = h; P.val = 0; P.ua = ua; P.ul = ul; P.dx = dx; P.dy = dy;
  if (highbd)
    hipLaunchKernelGGL((dr_single_kernel<uint16_t>), dim3(1), dim3(64), 0, s, (uint16_t*)dst,
                       (const uint16_t*)above, a_lo, a_n, (const uint16_t*)left, l_lo, l_n, P);
  else
    hipLaunchKernelGGL((dr_single_kernel<uint8_t>), dim3(1), dim3(64), 0, s, (uint8_t*)dst,
                       (const uint8_t*)above, a_lo, a_n, (const uint8_t*)left, l_lo, l_n, P);
  LCHK();
  return 0;
}

int intra_edge_single(void* buf, int n, int sz, int strength, int upsample, int bd, int highbd,
                      hipStream_t s) {
  if (sz < 1 || (upsample ? sz > 16 : sz > 129) || strength < 0 || strength > 3) return -4;
  if (n < 0 || n > 2 * kEdgeLen) return -4;
  const int maxv = (1 << bd) - 1;
  if (highbd)
    hipLaunchKernelGGL((edge_single_kernel<uint16_t>), dim3(1), dim3(64), 0, s, (uint16_t*)buf, n,
                       sz, strength, upsample, maxv);
  else
    hipLaunchKernelGGL((edge_single_kernel<uint8_t>), dim3(1), dim3(64), 0, s, (uint8_t*)buf, n, sz,
                       strength, upsample, maxv);
  LCHK();
  return 0;
}

// highbd: uint16_t pixels (the highbd shims take them at 8 bits too)
int intra_pred_batch(const void* ref, int ref_stride, void* dst, int dst_stride,
                     const LavishIntraJob* jobs, int njobs, int bd, int highbd, hipStream_t s) {
  if (njobs <= 0) return 0;
  if (!ref || !dst || !jobs) return -1;
  if (!bd_ok(bd, highbd)) return -5;
  const dim3 g((njobs + kJobsPerWg - 1) / kJobsPerWg), b(64 * kWaves);
  if (!highbd)
    hipLaunchKernelGGL((intra_kernel<uint8_t>), g, b, 0, s, (const uint8_t*)ref, ref_stride,
                       (uint8_t*)dst, dst_stride, jobs, njobs, bd);
  else
    hipLaunchKernelGGL((intra_kernel<uint16_t>), g, b, 0, s, (const uint16_t*)ref, ref_stride,
                       (uint16_t*)dst, dst_stride, jobs, njobs, bd);
  LCHK();
  return 0;
}

}  // namespace lavish

using namespace lavish;

extern "C" {

int lavish_intra_pred_batch(const void* ref, int ref_stride, void* dst, int dst_stride,
                            const LavishIntraJob* jobs, int njobs, int bit_depth, void* stream) {
  if (njobs > 0 && bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -5;
  return intra_pred_batch(ref, ref_stride, dst, dst_stride, jobs, njobs, bit_depth, bit_depth > 8,
                          (hipStream_t)stream);
}

int lavish_intra_table(int which, int32_t* out, int cap) {
  const void* p = nullptr;
  int n = 0, sz = 1, sgn = 0;
  switch (which) {
    case 0: p = kSmoothWeights; n = 124; break;
    case 1: p = kDrIntraDerivative; n = 90; sz = 2; sgn = 1; break;
    case 2: p = kFilterIntraTaps; n = 5 * 8 * 8; sgn = 1; break;
    case 3: p = kIntraEdgeKernel; n = 15; break;
    case 4: p = kModeToAngle; n = 13; break;
    default: return 0;
  }
  for (int i = 0; i < n && i < cap && out; ++i)
    out[i] = sz == 2 ? ((const int16_t*)p)[i] : sgn ? ((const int8_t*)p)[i] : ((const uint8_t*)p)[i];
  return n;
}

}  // extern "C"
