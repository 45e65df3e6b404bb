// blend.hip -- the mask-building and blending layer between the first-pass
// convolves and the compound / OBMC searches, batched for gfx950.  All integer,
// bit-exact:
//   aom_[highbd_]blend_a64_{mask,hmask,vmask}    aom_dsp/blend_a64_mask.c:229-349,
//                                                blend_a64_hmask.c:21-70, blend_a64_vmask.c:21-70
//   aom_{lowbd,highbd}_blend_a64_d16_mask        aom_dsp/blend_a64_mask.c:36-223
//   av1_build_compound_diffwtd_mask[_highbd,_d16] av1/common/reconinter.c:296-439
//   calc_target_weighted_pred                    av1/encoder/rdopt.c:6362-6580
//   av1_build_obmc_inter_prediction              av1/common/reconinter.c:844-945
//   av1_wedge_{sse,sign}_from_residuals,
//   av1_wedge_compute_delta_squares              av1/encoder/wedge_utils.c:52-125
//
// Layout (as pixel_comp.hip): a job's rows are cut into chunks of PC pixels, a
// lane takes whole chunks with word-wide byte-addressed loads, and a wave holds
// 64 / LPJ jobs of LPJ = min(64, chunks) lanes each (a 4x4 job takes 4 lanes).
// Dead lanes of the last workgroup read the last live job and write nothing.
// These kernels stream: PC is 16 bytes of the source type (16 u8 or 8 u16 / d16
// samples) wherever the row is that wide, because a lane's 16-byte access moves
// about twice the bytes per request of an 8-byte one; the unpacked pixels of
// three such chunks stay far below the 128 VGPRs of full 256-thread occupancy.
#include "lavish_internal.h"
#include "pixel_dev.h"

namespace lavish {
namespace {

// n elements (a power of two <= N) at p into v[0..n-1]; v[n..] = 0.  n * sizeof(T)
// >= 4 loads 1 / 2 / 4 words at once, the 1- and 2-byte rows of the narrow
// chroma spans load their elements one by one.
template <typename T, int N>
__device__ __forceinline__ void load_vec(const T* p, int n, int (&v)[N]) {
  const int bytes = n * (int)sizeof(T);
  if (bytes >= 4) {
    uint32_t w[4];
    load_words((const uint8_t*)p, bytes >> 2, w);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if constexpr (sizeof(T) == 1) v[i] = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xFF);
      else v[i] = (int)((w[i >> 1] >> (16 * (i & 1))) & 0xFFFF);
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = 0;
    v[0] = p[0];
    if (n == 2) v[1] = p[1];
  }
}

// v[0..n-1] to the n elements at p: one 4 / 8 / 16-byte store, or single elements
template <typename T, int N>
__device__ __forceinline__ void store_vec(T* p, int n, const int (&v)[N]) {
  const int bytes = n * (int)sizeof(T);
  if (bytes < 4) {
    p[0] = (T)v[0];
    if (n == 2) p[1] = (T)v[1];
    return;
  }
  uint32_t w[4] = {0, 0, 0, 0};
  if constexpr (sizeof(T) == 1) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i)
      w[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) |
             ((uint32_t)v[4 * i + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) w[i] = (uint32_t)v[2 * i] | ((uint32_t)v[2 * i + 1] << 16);
  }
  const int c = bytes >> 2;
  if (c == 4) {
    u32x4u t;
    t.x = w[0]; t.y = w[1]; t.z = w[2]; t.w = w[3];
    *(__attribute__((address_space(1))) u32x4u*)p = t;
  } else if (c == 2) {
    u32x2u t;
    t.x = w[0]; t.y = w[1];
    *(__attribute__((address_space(1))) u32x2u*)p = t;
  } else {
    *(__attribute__((address_space(1))) u32u*)p = w[0];
  }
}

// v[0..n-1] (n = 8 or 16) as int32 words: n / 4 16-byte stores
template <int N>
__device__ __forceinline__ void store_i32(int32_t* p, int n, const int (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N / 4; ++i) {
    if (4 * i < n) {
      u32x4u t;
      t.x = (uint32_t)v[4 * i]; t.y = (uint32_t)v[4 * i + 1];
      t.z = (uint32_t)v[4 * i + 2]; t.w = (uint32_t)v[4 * i + 3];
      *(__attribute__((address_space(1))) u32x4u*)(p + 4 * i) = t;
    }
  }
}

// 8 int16 at p (the residual streams of the wedge kernels; any 2-byte offset)
__device__ __forceinline__ void load_s16x8(const int16_t* p, int (&v)[8]) {
  uint32_t w[4];
  load_words((const uint8_t*)p, 4, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (int)(int16_t)(w[i >> 1] >> (16 * (i & 1)));
}

__device__ __forceinline__ int blend_a64(int m, int a, int b) {
  return (m * a + (64 - m) * b + 32) >> 6;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

struct BlendShape {
  int lpc;   // log2(pixels per chunk)
  int lcpr;  // log2(chunks per row)
  int lpj;   // lanes per job (power of two, <= 64)
  int chunks;
};

// ---------------------------------------------------------------- blend ----
struct BlendArgs {
  int kind;        // 0: 2-D mask, 1: hmask (mask[x]), 2: vmask (mask[y])
  int subw, subh;  // 2-D mask: the mask is twice as wide / high as the block
  int d16;         // CONV_BUF_TYPE inputs
  int round_offset, round_bits, maxv;
  int s0s, s1s, ds, ms;  // strides
};

// the PC mask values of row y, columns x .. x + pc - 1 of a job's mask
template <int N>
__device__ __forceinline__ void blend_mask(const uint8_t* mask, const BlendArgs& a, int y, int x,
                                           int pc, int (&m)[N]) {
  if (a.kind == 2) {
    const int v = mask[y];
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = v;
  } else if (a.kind == 1) {
    load_vec(mask + x, pc, m);
  } else if (!a.subw) {
    load_vec(mask + (int64_t)(y << a.subh) * a.ms + x, pc, m);
    if (a.subh) {  // AOM_BLEND_AVG of two rows
      int m1[N];
      load_vec(mask + (int64_t)(2 * y + 1) * a.ms + x, pc, m1);
#pragma unroll
      for (int i = 0; i < N; ++i) m[i] = (m[i] + m1[i] + 1) >> 1;
    }
  } else {
    // 2 * pc mask columns per row: pair sums first, then the row(s)
    const int n2 = 2 * pc, nl = n2 < N ? n2 : N;
    int s[N];
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = 0;
    for (int r = 0; r <= a.subh; ++r) {
      const uint8_t* row = mask + (int64_t)((y << a.subh) + r) * a.ms + 2 * x;
      int lo[N], hi[N];
      load_vec(row, nl, lo);
      if (n2 > N) load_vec(row + N, N, hi);
      else {
#pragma unroll
        for (int i = 0; i < N; ++i) hi[i] = 0;
      }
#pragma unroll
      for (int i = 0; i < N; ++i)
        s[i] += i < N / 2 ? lo[(2 * i) % N] + lo[(2 * i + 1) % N]
                          : hi[(2 * i) % N] + hi[(2 * i + 1) % N];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = a.subh ? (s[i] + 2) >> 2 : (s[i] + 1) >> 1;
  }
}

// dst may be src0 or src1 (equal stride): a lane reads the pixels it writes
// and no others, so no pointer here is __restrict__
template <typename Src, typename Dst>
__global__ __launch_bounds__(256) void blend_kernel(Dst* dst, const Src* src0, const Src* src1,
                                                    const uint8_t* __restrict__ mask,
                                                    BlendShape sh, BlendArgs a,
                                                    const LavishCompJob* __restrict__ jobs,
                                                    int njobs) {
  constexpr int N = 16 / (int)sizeof(Src);
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> __builtin_ctz(sh.lpj);
  const int q = t & (sh.lpj - 1);
  const bool live = j < njobs;
  const LavishCompJob jb = jobs[live ? j : njobs - 1];
  const int pc = 1 << sh.lpc;
  const int rnd = (1 << a.round_bits) >> 1;
  for (int i = q; i < sh.chunks; i += sh.lpj) {
    const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
    int s0[N], s1[N], m[N], o[N];
    load_vec(src0 + jb.ref_off[0] + (int64_t)y * a.s0s + x, pc, s0);
    load_vec(src1 + jb.ref_off[1] + (int64_t)y * a.s1s + x, pc, s1);
    blend_mask(mask + jb.mask_off, a, y, x, pc, m);
    if (a.d16) {
      // a plain >> 6, not a rounding one: the final ROUND_POWER_OF_TWO rounds
      // once (blend_a64_mask.c:25-34)
#pragma unroll
      for (int u = 0; u < N; ++u) {
        const int r = ((m[u] * s0[u] + (64 - m[u]) * s1[u]) >> 6) - a.round_offset;
        o[u] = clampi((r + rnd) >> a.round_bits, 0, a.maxv);
      }
    } else {
#pragma unroll
      for (int u = 0; u < N; ++u) o[u] = blend_a64(m[u], s0[u], s1[u]);
    }
    if (!live) continue;
    store_vec(dst + jb.src_off + (int64_t)y * a.ds + x, pc, o);
  }
}

// ------------------------------------------------- diff-weighted mask ----
// pixel forms: diff = |a - b| >> (bd - 8); d16: ROUND_POWER_OF_TWO(|a - b|, round)
template <typename Src>
__global__ __launch_bounds__(256) void diffwtd_kernel(uint8_t* __restrict__ mask,
                                                      const Src* __restrict__ src0, int s0s,
                                                      const Src* __restrict__ src1, int s1s,
                                                      BlendShape sh, int w, int d16, int shift,
                                                      const LavishCompJob* __restrict__ jobs,
                                                      int njobs) {
  constexpr int N = 16 / (int)sizeof(Src);
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> __builtin_ctz(sh.lpj);
  const int q = t & (sh.lpj - 1);
  const bool live = j < njobs;
  const LavishCompJob jb = jobs[live ? j : njobs - 1];
  const int pc = 1 << sh.lpc;
  const int rnd = d16 ? (1 << shift) >> 1 : 0;
  for (int i = q; i < sh.chunks; i += sh.lpj) {
    const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
    int a[N], b[N], o[N];
    load_vec(src0 + jb.ref_off[0] + (int64_t)y * s0s + x, pc, a);
    load_vec(src1 + jb.ref_off[1] + (int64_t)y * s1s + x, pc, b);
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const int diff = (abs(a[u] - b[u]) + rnd) >> shift;
      const int m = min(38 + (diff >> 4), 64);  // DIFF_FACTOR 16, mask_base 38
      o[u] = jb.invert_mask ? 64 - m : m;
    }
    if (!live) continue;
    store_vec(mask + jb.mask_off + (int64_t)y * w + x, pc, o);
  }
}

// ------------------------------------------------------------- OBMC ----
// The 1-D masks of av1_get_obmc_mask: the caller's 127-byte table holds the
// masks of lengths 1, 2, 4 .. 64 back to back, so length n starts at n - 1.
struct ObmcArgs {
  int ovw, ovh;    // overlap (columns blended with left, rows blended with above)
  int lssx, lssy;  // plane subsampling (the bitmaps are in luma mi units)
  int skip_above;  // av1_skip_u4x4_pred_in_obmc(., ., 0)
};

// bit i of the result: pixel x + i of the plane lies under a visited above
// neighbour (mi column ((x + i) << ssx) >> 2 of the block)
__device__ __forceinline__ uint32_t above_bits(uint32_t above_mask, int x, int lssx, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((above_mask >> (((x + i) << lssx) >> 2)) & 1u) << i;
  return r;
}

// calc_target_weighted_pred, in the reference's order for one pixel:
//   above step   wsrc = (64 - mv[y]) * above, mask = mv[y]   (else 0 and 64)
//   both * 64
//   left step    wsrc = (wsrc >> 6) * mh[x] + (left << 6) * (64 - mh[x]),
//                mask = (mask >> 6) * mh[x]
//   wsrc = src * 4096 - wsrc
// Every value fits int32 at 12 bits: after the above step wsrc <= 64 * 4095 and
// after the scaling <= 4096 * 4095 < 2^24; the left step is a 64-weighted mean
// of two such values, again <= 4096 * 4095; src * 4096 <= 4096 * 4095; so
// |wsrc| < 2^24 and 0 <= mask <= 4096.
template <typename Pix>
__global__ __launch_bounds__(256) void obmc_wsrc_kernel(const Pix* __restrict__ src, int ss,
                                                        const Pix* __restrict__ above, int as,
                                                        const Pix* __restrict__ left, int ls,
                                                        BlendShape sh, int bw, ObmcArgs oa,
                                                        const uint8_t* __restrict__ tab,
                                                        const LavishObmcJob* __restrict__ jobs,
                                                        int njobs, int32_t* __restrict__ wsrc,
                                                        int32_t* __restrict__ mask) {
  constexpr int N = 16 / (int)sizeof(Pix);
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> __builtin_ctz(sh.lpj);
  const int q = t & (sh.lpj - 1);
  const bool live = j < njobs;
  const LavishObmcJob jb = jobs[live ? j : njobs - 1];
  const int pc = 1 << sh.lpc;
  for (int i = q; i < sh.chunks; i += sh.lpj) {
    const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
    int s[N], ws[N], mk[N];
    load_vec(src + jb.src_off + (int64_t)y * ss + x, pc, s);
    const uint32_t ab = y < oa.ovh ? above_bits(jb.above_mask, x, 0, pc) : 0u;
#pragma unroll
    for (int u = 0; u < N; ++u) {
      ws[u] = 0;
      mk[u] = 64 * 64;
    }
    if (ab) {
      int p[N];
      load_vec(above + jb.above_off + (int64_t)y * as + x, pc, p);
      const int mv = tab[oa.ovh - 1 + y];
#pragma unroll
      for (int u = 0; u < N; ++u)
        if ((ab >> u) & 1u) {
          ws[u] = (64 - mv) * p[u] * 64;
          mk[u] = mv * 64;
        }
    }
    if (x < oa.ovw && ((jb.left_mask >> (y >> 2)) & 1u)) {
      int p[N], mh[N];
      load_vec(left + jb.left_off + (int64_t)y * ls + x, pc, p);
      load_vec(tab + oa.ovw - 1 + x, pc, mh);
#pragma unroll
      for (int u = 0; u < N; ++u)
        if (x + u < oa.ovw) {
          ws[u] = (ws[u] >> 6) * mh[u] + (p[u] << 6) * (64 - mh[u]);
          mk[u] = (mk[u] >> 6) * mh[u];
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) ws[u] = s[u] * 4096 - ws[u];
    if (!live) continue;
    store_i32(wsrc + jb.wsrc_off + (int64_t)y * bw + x, pc, ws);
    store_i32(mask + jb.mask_off + (int64_t)y * bw + x, pc, mk);
  }
}

// av1_build_obmc_inter_prediction on one plane, in place: the vmask blend with
// the above predictor, then the hmask blend with the left one reads its
// result, so one lane does both for its pixels
template <typename Pix>
__global__ __launch_bounds__(256) void obmc_blend_kernel(Pix* dst, int ds,
                                                         const Pix* __restrict__ above, int as,
                                                         const Pix* __restrict__ left, int ls,
                                                         BlendShape sh, ObmcArgs oa,
                                                         const uint8_t* __restrict__ tab,
                                                         const LavishObmcJob* __restrict__ jobs,
                                                         int njobs) {
  constexpr int N = 16 / (int)sizeof(Pix);
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> __builtin_ctz(sh.lpj);
  const int q = t & (sh.lpj - 1);
  const bool live = j < njobs;
  const LavishObmcJob jb = jobs[live ? j : njobs - 1];
  const int pc = 1 << sh.lpc;
  for (int i = q; i < sh.chunks; i += sh.lpj) {
    const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
    const uint32_t ab =
        !oa.skip_above && y < oa.ovh ? above_bits(jb.above_mask, x, oa.lssx, pc) : 0u;
    const bool lf = x < oa.ovw && ((jb.left_mask >> ((y << oa.lssy) >> 2)) & 1u);
    if (!ab && !lf) continue;
    int d[N];
    load_vec(dst + jb.src_off + (int64_t)y * ds + x, pc, d);
    if (ab) {
      int p[N];
      load_vec(above + jb.above_off + (int64_t)y * as + x, pc, p);
      const int mv = tab[oa.ovh - 1 + y];
#pragma unroll
      for (int u = 0; u < N; ++u)
        if ((ab >> u) & 1u) d[u] = blend_a64(mv, d[u], p[u]);
    }
    if (lf) {
      int p[N], mh[N];
      load_vec(left + jb.left_off + (int64_t)y * ls + x, pc, p);
      load_vec(tab + oa.ovw - 1 + x, pc, mh);
#pragma unroll
      for (int u = 0; u < N; ++u)
        if (x + u < oa.ovw) d[u] = blend_a64(mh[u], d[u], p[u]);
    }
    if (!live) continue;
    store_vec(dst + jb.src_off + (int64_t)y * ds + x, pc, d);
  }
}

// ------------------------------------------------------------ wedge ----
// One wave per job, a lane takes chunks of 8 elements (16 bytes of int16); n is
// a multiple of 64, so n = 64 keeps 8 lanes busy and n = 16384 gives each lane
// 32 chunks.  kind 0: delta squares, 1: sse, 2: sign.
__global__ __launch_bounds__(256) void wedge_kernel(const int16_t* __restrict__ a,
                                                    const int16_t* __restrict__ b,
                                                    const uint8_t* __restrict__ m,
                                                    const LavishWedgeJob* __restrict__ jobs,
                                                    int njobs, int kind, void* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> 6, q = t & 63;
  const bool live = j < njobs;
  const LavishWedgeJob jb = jobs[live ? j : njobs - 1];
  const int chunks = jb.n >> 3;
  if (kind == 0) {
    for (int i = q; i < chunks; i += 64) {
      int x[8], y[8], o[8];
      load_s16x8(a + jb.a_off + 8 * i, x);
      load_s16x8(b + jb.b_off + 8 * i, y);
#pragma unroll
      for (int u = 0; u < 8; ++u)  // |x^2 - y^2| <= 2^30: int32
        o[u] = clampi(x[u] * x[u] - y[u] * y[u], -32768, 32767) & 0xFFFF;
      if (live) store_vec((uint16_t*)out + jb.out_off + 8 * i, 8, o);
    }
    return;
  }
  int64_t acc = 0;
  for (int i = q; i < chunks; i += 64) {
    int x[8], mk[8];
    load_s16x8(a + jb.a_off + 8 * i, x);
    load_vec(m + jb.m_off + 8 * i, 8, mk);
    if (kind == 1) {
      int y[8];
      load_s16x8(b + jb.b_off + 8 * i, y);
      // t * t <= 2^30 (t = -32768), so a 32-bit sum holds 3 squares and not 4:
      // squares are added in pairs (<= 2^31) and each pair goes to 64 bits
      uint64_t c = 0;
#pragma unroll
      for (int u = 0; u < 8; u += 2) {
        const int t0 = clampi(64 * x[u] + mk[u] * y[u], -32768, 32767);
        const int t1 = clampi(64 * x[u + 1] + mk[u + 1] * y[u + 1], -32768, 32767);
        c += (uint32_t)(t0 * t0) + (uint32_t)(t1 * t1);
      }
      acc += (int64_t)c;
    } else {
      int c = 0;  // 8 products of |ds| <= 2^15 and m <= 255: < 2^26
#pragma unroll
      for (int u = 0; u < 8; ++u) c += x[u] * mk[u];
      acc += c;
    }
  }
  acc = wave_sum64(acc);
  if (!live || q != 0) return;
  if (kind == 1) ((uint64_t*)out)[j] = ((uint64_t)acc + (1ull << 11)) >> 12;
  else ((int8_t*)out)[j] = acc > jb.limit;
}

static bool pow2(int v, int lo, int hi) { return v >= lo && v <= hi && !(v & (v - 1)); }

// the chunk layout of a w x h block (powers of two) with rows of `elem`-byte samples
static void blend_shape(int w, int h, int elem, BlendShape& sh) {
  const int maxpc = 16 / elem;
  const int pc = w < maxpc ? w : maxpc;
  sh.lpc = ilog2(pc);
  sh.lcpr = ilog2(w / pc);
  sh.chunks = h << sh.lcpr;
  sh.lpj = sh.chunks < 64 ? sh.chunks : 64;
}
static int blend_blocks(int njobs, const BlendShape& sh) {
  return (int)(((int64_t)njobs * sh.lpj + 255) / 256);
}

// OBMC runs on the encoder block sizes of at least 8x8
// (is_motion_variation_allowed_bsize, av1/common/blockd.h)
static bool obmc_size_ok(int bw, int bh) {
  bool ok = false;
#define LAVISH_SIZE_OK(w, h) ok |= (bw == w && bh == h);
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_SIZE_OK)
#undef LAVISH_SIZE_OK
  return ok && bw >= 8 && bh >= 8;
}

}  // namespace
}  // namespace lavish

using namespace lavish;

#define LCHK() LAVISH_CHECK(hipGetLastError())

extern "C" {

int lavish_blend_a64_batch(void* dst, int dst_stride, const void* src0, int src0_stride,
                           const void* src1, int src1_stride, const uint8_t* mask,
                           int mask_stride, int w, int h, const LavishCompJob* jobs, int njobs,
                           int kind, int subw, int subh, int d16, int highbd, int bit_depth,
                           const LavishConvolveParams* conv_params, void* stream) {
  if (njobs <= 0) return 0;
  if (kind < 0 || kind > 2 || !dst || !src0 || !src1 || !mask || !jobs) return -1;
  if ((subw | subh) & ~1) return -2;
  if (kind != 0 && (subw || subh || d16)) return -2;
  if (kind == 0 && mask_stride < (w << subw)) return -2;
  if (!pow2(w, d16 ? 4 : 1, 128) || !pow2(h, d16 ? 4 : 1, 128)) return -4;
  if (!bd_ok(bit_depth, highbd)) return -5;
  BlendArgs a = {kind, subw, subh, d16 != 0, 0, 0, (1 << bit_depth) - 1,
                 src0_stride, src1_stride, dst_stride, mask_stride};
  if (d16) {
    if (!conv_params) return -3;
    const int r0 = conv_params->round_0, r1 = conv_params->round_1;
    const int offset_bits = bit_depth + 14 - r0;  // 2 * FILTER_BITS
    a.round_bits = 14 - r0 - r1;
    if (r0 < 0 || r1 < 0 || a.round_bits < 0 || offset_bits - r1 - 1 < 0 || offset_bits > 30)
      return -3;
    a.round_offset = (1 << (offset_bits - r1)) + (1 << (offset_bits - r1 - 1));
  }
  BlendShape sh;
  blend_shape(w, h, d16 || highbd ? 2 : 1, sh);
  const dim3 g(blend_blocks(njobs, sh)), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (d16 && !highbd)
    hipLaunchKernelGGL((blend_kernel<uint16_t, uint8_t>), g, b, 0, s, (uint8_t*)dst,
                       (const uint16_t*)src0, (const uint16_t*)src1, mask, sh, a, jobs, njobs);
  else if (highbd)
    hipLaunchKernelGGL((blend_kernel<uint16_t, uint16_t>), g, b, 0, s, (uint16_t*)dst,
                       (const uint16_t*)src0, (const uint16_t*)src1, mask, sh, a, jobs, njobs);
  else
    hipLaunchKernelGGL((blend_kernel<uint8_t, uint8_t>), g, b, 0, s, (uint8_t*)dst,
                       (const uint8_t*)src0, (const uint8_t*)src1, mask, sh, a, jobs, njobs);
  LCHK();
  return 0;
}

int lavish_diffwtd_mask_batch(uint8_t* mask, const void* src0, int src0_stride, const void* src1,
                              int src1_stride, int w, int h, const LavishCompJob* jobs, int njobs,
                              int d16, int highbd, int bit_depth,
                              const LavishConvolveParams* conv_params, void* stream) {
  if (njobs <= 0) return 0;
  if (!mask || !src0 || !src1 || !jobs) return -1;
  if (!pow2(w, 4, 128) || !pow2(h, 4, 128)) return -4;
  if (!(d16 ? (bit_depth == 8 || bit_depth == 10 || bit_depth == 12) : bd_ok(bit_depth, highbd)))
    return -5;
  int shift = bit_depth - 8;
  if (d16) {
    if (!conv_params) return -3;
    shift = 14 - conv_params->round_0 - conv_params->round_1 + (bit_depth - 8);
    if (conv_params->round_0 < 0 || conv_params->round_1 < 0 || shift < 0) return -3;
  }
  BlendShape sh;
  blend_shape(w, h, d16 || highbd ? 2 : 1, sh);
  const dim3 g(blend_blocks(njobs, sh)), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (d16 || highbd)
    hipLaunchKernelGGL(diffwtd_kernel<uint16_t>, g, b, 0, s, mask, (const uint16_t*)src0,
                       src0_stride, (const uint16_t*)src1, src1_stride, sh, w, d16 != 0, shift,
                       jobs, njobs);
  else
    hipLaunchKernelGGL(diffwtd_kernel<uint8_t>, g, b, 0, s, mask, (const uint8_t*)src0,
                       src0_stride, (const uint8_t*)src1, src1_stride, sh, w, 0, 0, jobs, njobs);
  LCHK();
  return 0;
}

int lavish_obmc_wsrc_batch(const void* src, int src_stride, const void* above, int above_stride,
                           const void* left, int left_stride, int bw, int bh,
                           const LavishObmcJob* jobs, int njobs, const uint8_t* obmc_masks,
                           int highbd, int32_t* wsrc, int32_t* mask, void* stream) {
  if (njobs <= 0) return 0;
  if (!src || !above || !left || !jobs || !wsrc || !mask) return -1;
  if (!obmc_masks) return -2;
  if (!obmc_size_ok(bw, bh)) return -4;
  const ObmcArgs oa = {(bw < 64 ? bw : 64) >> 1, (bh < 64 ? bh : 64) >> 1, 0, 0, 0};
  BlendShape sh;
  blend_shape(bw, bh, highbd ? 2 : 1, sh);
  const dim3 g(blend_blocks(njobs, sh)), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (highbd)
    hipLaunchKernelGGL(obmc_wsrc_kernel<uint16_t>, g, b, 0, s, (const uint16_t*)src, src_stride,
                       (const uint16_t*)above, above_stride, (const uint16_t*)left, left_stride,
                       sh, bw, oa, obmc_masks, jobs, njobs, wsrc, mask);
  else
    hipLaunchKernelGGL(obmc_wsrc_kernel<uint8_t>, g, b, 0, s, (const uint8_t*)src, src_stride,
                       (const uint8_t*)above, above_stride, (const uint8_t*)left, left_stride, sh,
                       bw, oa, obmc_masks, jobs, njobs, wsrc, mask);
  LCHK();
  return 0;
}

int lavish_obmc_blend_batch(void* dst, int dst_stride, const void* above, int above_stride,
                            const void* left, int left_stride, int bw, int bh, int subsampling_x,
                            int subsampling_y, const LavishObmcJob* jobs, int njobs,
                            const uint8_t* obmc_masks, int highbd, void* stream) {
  if (njobs <= 0) return 0;
  if (!dst || !above || !left || !jobs) return -1;
  if (!obmc_masks) return -2;
  if ((subsampling_x | subsampling_y) & ~1) return -3;
  if (!obmc_size_ok(bw, bh)) return -4;
  const int pw = bw >> subsampling_x, ph = bh >> subsampling_y;
  // BLOCK_4X4 / 8X4 / 4X8 planes blend with the left neighbours only
  const int skip = (pw == 4 && ph <= 8) || (pw == 8 && ph == 4);
  const ObmcArgs oa = {((bw < 64 ? bw : 64) >> 1) >> subsampling_x,
                       ((bh < 64 ? bh : 64) >> 1) >> subsampling_y, subsampling_x, subsampling_y,
                       skip};
  BlendShape sh;
  blend_shape(pw, ph, highbd ? 2 : 1, sh);
  const dim3 g(blend_blocks(njobs, sh)), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (highbd)
    hipLaunchKernelGGL(obmc_blend_kernel<uint16_t>, g, b, 0, s, (uint16_t*)dst, dst_stride,
                       (const uint16_t*)above, above_stride, (const uint16_t*)left, left_stride,
                       sh, oa, obmc_masks, jobs, njobs);
  else
    hipLaunchKernelGGL(obmc_blend_kernel<uint8_t>, g, b, 0, s, (uint8_t*)dst, dst_stride,
                       (const uint8_t*)above, above_stride, (const uint8_t*)left, left_stride, sh,
                       oa, obmc_masks, jobs, njobs);
  LCHK();
  return 0;
}

int lavish_wedge_batch(const int16_t* a, const int16_t* b, const uint8_t* m,
                       const LavishWedgeJob* jobs, int njobs, int kind, void* out,
                       void* stream) {
  if (njobs <= 0) return 0;
  if (kind < 0 || kind > 2 || !a || !jobs || !out) return -1;
  if ((kind != 2 && !b) || (kind != 0 && !m)) return -2;
  hipLaunchKernelGGL(wedge_kernel, dim3((njobs + 3) / 4), dim3(256), 0, (hipStream_t)stream, a, b,
                     m, jobs, njobs, kind, out);
  LCHK();
  return 0;
}

}  // extern "C"
