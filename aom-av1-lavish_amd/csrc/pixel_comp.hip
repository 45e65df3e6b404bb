// pixel_comp.hip -- the compound members of the per-block-size function table
// (aom_variance_fn_ptr_t: msdf, msvf, osdf, ovf, osvf, jsdaf, jsvaf) and the
// prediction helpers they reduce to, batched for gfx950.  All integer,
// bit-exact:
//   AOM_BLEND_A64                      aom_dsp/blend.h:23-30
//   masked SAD (+x4d)                  aom_dsp/sad_av1.c:21-67, highbd :95-133
//   masked sub-pixel variance          aom_dsp/variance.c:749-814, highbd :817-929
//   distance-weighted average          aom_dsp/variance.c:300-318, highbd :725-746
//   dist-wtd SAD                       aom_dsp/sad.c:57-64, highbd :290-298
//   dist-wtd sub-pixel avg variance    aom_dsp/variance.c:165-181, highbd to :664
//   OBMC SAD                           aom_dsp/sad_av1.c:163-186, highbd :215-239
//   OBMC (sub-pixel) variance          aom_dsp/variance.c:933-976, highbd :1040-1170
//   comp_avg / dist_wtd / mask pred    aom_dsp/variance.c:285-318,707-767,817-837
//
// Layout (as sad_u8_kernel / var_u8_kernel of pixel.hip): a job's rows are cut
// into chunks of PC = min(w, 8) pixels, a lane takes whole chunks with
// word-wide byte-addressed loads, and a wave holds 64 / LPJ jobs of LPJ =
// min(64, chunks) lanes each (a 4x4 job takes 4 lanes).  Dead lanes of the
// last workgroup read the last live job and write nothing.
#include "lavish_internal.h"
#include "pixel_dev.h"

namespace lavish {

// PC pixels at p into v[0..PC-1] (v[PC..7] = 0); PC is 4 or 8
template <typename Pix>
__device__ __forceinline__ void load_px(const Pix* p, int pc, int (&v)[8]) {
  uint32_t w[4];
  if constexpr (sizeof(Pix) == 1) {
    load_words((const uint8_t*)p, pc >> 2, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xFF);
  } else {
    load_words((const uint8_t*)p, pc >> 1, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (int)((w[i >> 1] >> (16 * (i & 1))) & 0xFFFF);
  }
}

// v[0..PC-1] to the PC pixels at p, as one 4 / 8 / 16-byte store
template <typename Pix>
__device__ __forceinline__ void store_px(Pix* p, int pc, const int (&v)[8]) {
  uint32_t w[4];
  int c;
  if constexpr (sizeof(Pix) == 1) {
    c = pc >> 2;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      w[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) |
             ((uint32_t)v[4 * i + 3] << 24);
    w[2] = w[3] = 0;
  } else {
    c = pc >> 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)v[2 * i] | ((uint32_t)v[2 * i + 1] << 16);
  }
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

// PC int32 words (the OBMC wsrc / mask streams)
__device__ __forceinline__ void load_i32(const int32_t* p, int pc, int (&v)[8]) {
  uint32_t w[4];
  load_words((const uint8_t*)p, 4, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (int)w[i];
  if (pc == 8) {
    load_words((const uint8_t*)(p + 4), 4, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[4 + i] = (int)w[i];
  } else {
#pragma unroll
    for (int i = 4; i < 8; ++i) v[i] = 0;
  }
}

// PC pixels of the two-pass bilinear filter of aom_var_filter_block2d_bil_
// {first,second}_pass (variance.c:73-121) at p (row stride st): reads rows
// y, y + 1 and PC + 1 columns
template <typename Pix>
__device__ __forceinline__ void bilinear_px(const Pix* p, int st, int pc, int xo, int yo,
                                            int (&v)[8]) {
  int r0[8], r1[8];
  load_px(p, pc, r0);
  load_px(p + st, pc, r1);
  const int n0 = p[pc], n1 = p[st + pc];
  const int f0 = bil_tap(xo, 0), f1 = bil_tap(xo, 1);
  const int g0 = bil_tap(yo, 0), g1 = bil_tap(yo, 1);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // the right neighbour: the next pixel of the chunk, or the one past it
    const int a0 = i + 1 < pc ? r0[i < 7 ? i + 1 : 7] : n0;
    const int a1 = i + 1 < pc ? r1[i < 7 ? i + 1 : 7] : n1;
    const int h0 = (r0[i] * f0 + a0 * f1 + 64) >> 7;
    const int h1 = (r1[i] * f0 + a1 * f1 + 64) >> 7;
    v[i] = (h0 * g0 + h1 * g1 + 64) >> 7;
  }
}

__device__ __forceinline__ int blend_a64(int m, int a, int b) {
  return (m * a + (64 - m) * b + 32) >> 6;
}
__device__ __forceinline__ int dist_wtd(int second, int ref, int fwd, int bck) {
  return (second * bck + ref * fwd + 8) >> 4;
}

struct CompArgs {
  const uint8_t* mask;  // u8 blend mask plane (masked modes)
  int mask_stride;
  int fwd, bck;  // distance weights
};

// the compound prediction of PC pixels: `r` (the reference / filtered block)
// combined with second_pred `p`; mode 0 masked, 1 dist-wtd, 2 rounded average
__device__ __forceinline__ void comp_px(int mode, const CompArgs& ca, const LavishCompJob& jb,
                                        int y, int x, int pc, const int (&r)[8],
                                        const int (&p)[8], int (&o)[8]) {
  if (mode == 0) {
    int m[8];
    load_px(ca.mask + jb.mask_off + (int64_t)y * ca.mask_stride + x, pc, m);
    const bool inv = jb.invert_mask != 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = inv ? blend_a64(m[i], p[i], r[i]) : blend_a64(m[i], r[i], p[i]);
  } else if (mode == 1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = dist_wtd(p[i], r[i], ca.fwd, ca.bck);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (p[i] + r[i] + 1) >> 1;
  }
}

struct CompShape {
  int lpc;   // log2(pixels per chunk): 2 or 3
  int lcpr;  // log2(chunks per row)
  int lpj;   // lanes per job (power of two, <= 64)
  int chunks;
};

// ------------------------------------------------------- compound SAD ----
template <typename Pix>
__global__ __launch_bounds__(256) void comp_sad_kernel(const Pix* __restrict__ src, int ss,
                                                       const Pix* __restrict__ ref, int rs,
                                                       CompShape sh, int w,
                                                       const LavishCompJob* __restrict__ jobs,
                                                       int njobs, int nrefs, int mode,
                                                       const Pix* __restrict__ second, CompArgs ca,
                                                       uint32_t* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> __builtin_ctz(sh.lpj);
  const int q = t & (sh.lpj - 1);
  const bool live = j < njobs;
  const LavishCompJob jb = jobs[live ? j : njobs - 1];
  const int pc = 1 << sh.lpc;
  for (int k = 0; k < nrefs; ++k) {
    uint32_t acc = 0;
    for (int i = q; i < sh.chunks; i += sh.lpj) {
      const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
      int s[8], r[8], p[8], o[8];
      load_px(src + jb.src_off + (int64_t)y * ss + x, pc, s);
      load_px(ref + jb.ref_off[k] + (int64_t)y * rs + x, pc, r);
      load_px(second + jb.second_off + (int64_t)y * w + x, pc, p);
      comp_px(mode, ca, jb, y, x, pc, r, p, o);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < pc) acc += (uint32_t)abs(o[u] - s[u]);
    }
    acc = group_sum(acc, sh.lpj);
    if (live && q == 0) out[(int64_t)j * nrefs + k] = acc;
  }
}

// (sum, sse) over the lane group, then the variance rounding of the lowbd /
// highbd 8, 10, 12 forms (variance.c:321-408; OBMC :1063-1123 is the same)
__device__ __forceinline__ void var_finish(int64_t sum, uint64_t sse, int lpj, bool write, int64_t j,
                                           int bd, int wh, uint32_t* __restrict__ var_out,
                                           uint32_t* __restrict__ sse_out) {
  for (int m = 1; m < lpj; m <<= 1) {
    sum += __shfl_xor(sum, m);
    sse += (uint64_t)__shfl_xor((int64_t)sse, m);
  }
  if (!write) return;
  uint32_t s32;
  int sm;
  if (bd == 8) {
    s32 = (uint32_t)sse;
    sm = (int)sum;
  } else {
    const int ss_ = bd == 10 ? 4 : 8, sh2 = bd == 10 ? 2 : 4;
    s32 = (uint32_t)((sse + ((1ull << ss_) >> 1)) >> ss_);
    sm = (int)((sum + ((1ll << sh2) >> 1)) >> sh2);  // arithmetic shift of a signed sum
  }
  if (sse_out) sse_out[j] = s32;
  if (var_out) {
    if (bd == 8) {
      var_out[j] = s32 - (uint32_t)(((int64_t)sm * sm) / wh);
    } else {
      const int64_t v = (int64_t)s32 - (((int64_t)sm * sm) / wh);
      var_out[j] = v >= 0 ? (uint32_t)v : 0;
    }
  }
}

// ----------------------------------------- compound sub-pixel variance ----
// kind 0: masked, 1: distance-weighted average; a is bilinear-filtered
template <typename Pix>
__global__ __launch_bounds__(256) void comp_var_kernel(const Pix* __restrict__ a, int as,
                                                       const Pix* __restrict__ b, int bs,
                                                       CompShape sh, int w, int h,
                                                       const LavishCompJob* __restrict__ jobs,
                                                       int njobs, int kind, int bd,
                                                       const Pix* __restrict__ second, CompArgs ca,
                                                       uint32_t* __restrict__ var_out,
                                                       uint32_t* __restrict__ sse_out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> __builtin_ctz(sh.lpj);
  const int q = t & (sh.lpj - 1);
  const bool live = j < njobs;
  const LavishCompJob jb = jobs[live ? j : njobs - 1];
  const int pc = 1 << sh.lpc;
  int64_t sum = 0;
  uint64_t sse = 0;
  for (int i = q; i < sh.chunks; i += sh.lpj) {
    const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
    int f[8], r[8], p[8], o[8];
    bilinear_px(a + jb.src_off + (int64_t)y * as + x, as, pc, jb.xoff, jb.yoff, f);
    load_px(b + jb.ref_off[0] + (int64_t)y * bs + x, pc, r);
    load_px(second + jb.second_off + (int64_t)y * w + x, pc, p);
    comp_px(kind, ca, jb, y, x, pc, f, p, o);
    int s = 0;
    uint32_t q2 = 0;  // <= 8 squares of 12-bit differences: < 2^28
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int d = u < pc ? o[u] - r[u] : 0;
      s += d;
      q2 += (uint32_t)(d * d);
    }
    sum += s;
    sse += q2;
  }
  var_finish(sum, sse, sh.lpj, live && q == 0, j, bd, w * h, var_out, sse_out);
}

// ---------------------------------------------------------------- OBMC ----
// kind 0: SAD against npre predictors, 1: variance, 2: variance of the
// bilinear-filtered predictor.  wsrc / mask: int32, contiguous w x h.
template <typename Pix>
__global__ __launch_bounds__(256) void obmc_kernel(const Pix* __restrict__ pre, int ps,
                                                   CompShape sh, int w, int h,
                                                   const LavishCompJob* __restrict__ jobs,
                                                   int njobs, int npre, int kind, int bd,
                                                   const int32_t* __restrict__ wsrc,
                                                   const int32_t* __restrict__ mask,
                                                   uint32_t* __restrict__ out,
                                                   uint32_t* __restrict__ sse_out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> __builtin_ctz(sh.lpj);
  const int q = t & (sh.lpj - 1);
  const bool live = j < njobs;
  const LavishCompJob jb = jobs[live ? j : njobs - 1];
  const int pc = 1 << sh.lpc;
  if (kind == 0) {
    for (int k = 0; k < npre; ++k) {
      uint32_t acc = 0;
      for (int i = q; i < sh.chunks; i += sh.lpj) {
        const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
        int p[8], ws[8], m[8];
        load_px(pre + jb.ref_off[k] + (int64_t)y * ps + x, pc, p);
        load_i32(wsrc + jb.second_off + (int64_t)y * w + x, pc, ws);
        load_i32(mask + jb.mask_off + (int64_t)y * w + x, pc, m);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (u < pc) acc += ((uint32_t)abs(ws[u] - p[u] * m[u]) + 2048u) >> 12;
      }
      acc = group_sum(acc, sh.lpj);
      if (live && q == 0) out[(int64_t)j * npre + k] = acc;
    }
    return;
  }
  int64_t sum = 0;
  uint64_t sse = 0;
  for (int i = q; i < sh.chunks; i += sh.lpj) {
    const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
    int p[8], ws[8], m[8];
    const Pix* pp = pre + jb.ref_off[0] + (int64_t)y * ps + x;
    if (kind == 2) bilinear_px(pp, ps, pc, jb.xoff, jb.yoff, p);
    else load_px(pp, pc, p);
    load_i32(wsrc + jb.second_off + (int64_t)y * w + x, pc, ws);
    load_i32(mask + jb.mask_off + (int64_t)y * w + x, pc, m);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < pc) {
        // ROUND_POWER_OF_TWO_SIGNED(v, 12)
        const int v = ws[u] - p[u] * m[u];
        const int r = (int)(((uint32_t)abs(v) + 2048u) >> 12);
        const int d = v < 0 ? -r : r;
        sum += d;
        sse += (uint32_t)(d * d);
      }
    }
  }
  var_finish(sum, sse, sh.lpj, live && q == 0, j, bd, w * h, out, sse_out);
}

// ------------------------------------------------ compound prediction ----
// comp_pred[src_off + y * w + x] from pred (second_off, stride w) and ref
// (ref_off[0], ref_stride); mode 0 avg, 1 dist-wtd, 2 mask
template <typename Pix>
__global__ __launch_bounds__(256) void comp_pred_kernel(Pix* __restrict__ comp_pred,
                                                        const Pix* __restrict__ pred,
                                                        CompShape sh, int w,
                                                        const Pix* __restrict__ ref, int rs,
                                                        const LavishCompJob* __restrict__ jobs,
                                                        int njobs, int mode, CompArgs ca) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t >> __builtin_ctz(sh.lpj);
  const int q = t & (sh.lpj - 1);
  const bool live = j < njobs;
  const LavishCompJob jb = jobs[live ? j : njobs - 1];
  const int pc = 1 << sh.lpc;
  const int cm = mode == 0 ? 2 : mode == 2 ? 0 : 1;  // comp_px's numbering
  for (int i = q; i < sh.chunks; i += sh.lpj) {
    const int y = i >> sh.lcpr, x = (i & ((1 << sh.lcpr) - 1)) << sh.lpc;
    int r[8], p[8], o[8];
    load_px(ref + jb.ref_off[0] + (int64_t)y * rs + x, pc, r);
    load_px(pred + jb.second_off + (int64_t)y * w + x, pc, p);
    comp_px(cm, ca, jb, y, x, pc, r, p, o);
    if (!live) continue;
    store_px(comp_pred + jb.src_off + (int64_t)y * w + x, pc, o);
  }
}

// @encoder_block_sizes (aom_dsp/aom_dsp_rtcd_defs.pl:42-58)
static bool comp_shape(int w, int h, CompShape& sh) {
  bool ok = false;
#define LAVISH_SIZE_OK(bw, bh) ok |= (w == bw && h == bh);
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_SIZE_OK)
#undef LAVISH_SIZE_OK
  if (!ok) return false;
  const int pc = w < 8 ? w : 8;
  sh.lpc = ilog2(pc);
  sh.lcpr = ilog2(w / pc);
  sh.chunks = h << sh.lcpr;
  sh.lpj = sh.chunks < 64 ? sh.chunks : 64;
  return true;
}

static bool dist_offsets_ok(int fwd, int bck) { return fwd >= 0 && bck >= 0 && fwd + bck == 16; }
static bool bit_depth_ok(int bd) { return bd == 8 || bd == 10 || bd == 12; }
static int comp_blocks(int njobs, const CompShape& sh) {
  return (int)(((int64_t)njobs * sh.lpj + 255) / 256);
}

}  // namespace lavish

using namespace lavish;

#define LCHK() LAVISH_CHECK(hipGetLastError())

extern "C" {

int lavish_comp_sad_batch(const void* src, int src_stride, const void* ref, int ref_stride, int w,
                          int h, const LavishCompJob* jobs, int njobs, int nrefs, int mode,
                          const void* second_pred, const uint8_t* mask, int mask_stride,
                          int fwd_offset, int bck_offset, int highbd, uint32_t* sad_out,
                          void* stream) {
  if (njobs <= 0) return 0;
  CompShape sh;
  if (nrefs < 1 || nrefs > 4 || mode < 0 || mode > 1 || !second_pred) return -1;
  if (mode == 0 && (!mask || mask_stride < w)) return -2;
  if (mode == 1 && !dist_offsets_ok(fwd_offset, bck_offset)) return -3;
  if (!comp_shape(w, h, sh)) return -4;
  const CompArgs ca = {mask, mask_stride, fwd_offset, bck_offset};
  hipStream_t s = (hipStream_t)stream;
  if (highbd)
    hipLaunchKernelGGL(comp_sad_kernel<uint16_t>, dim3(comp_blocks(njobs, sh)), dim3(256), 0, s,
                       (const uint16_t*)src, src_stride, (const uint16_t*)ref, ref_stride, sh, w,
                       jobs, njobs, nrefs, mode, (const uint16_t*)second_pred, ca, sad_out);
  else
    hipLaunchKernelGGL(comp_sad_kernel<uint8_t>, dim3(comp_blocks(njobs, sh)), dim3(256), 0, s,
                       (const uint8_t*)src, src_stride, (const uint8_t*)ref, ref_stride, sh, w,
                       jobs, njobs, nrefs, mode, (const uint8_t*)second_pred, ca, sad_out);
  LCHK();
  return 0;
}

int lavish_comp_variance_batch(const void* a, int a_stride, const void* b, int b_stride, int w,
                               int h, const LavishCompJob* jobs, int njobs, int kind,
                               int bit_depth, int highbd, const void* second_pred,
                               const uint8_t* mask, int mask_stride, int fwd_offset,
                               int bck_offset, uint32_t* var_out, uint32_t* sse_out,
                               void* stream) {
  if (njobs <= 0) return 0;
  CompShape sh;
  if (kind < 0 || kind > 1 || !second_pred) return -1;
  if (kind == 0 && (!mask || mask_stride < w)) return -2;
  if (kind == 1 && !dist_offsets_ok(fwd_offset, bck_offset)) return -3;
  if (!comp_shape(w, h, sh)) return -4;
  if (!bit_depth_ok(bit_depth)) return -5;
  const CompArgs ca = {mask, mask_stride, fwd_offset, bck_offset};
  hipStream_t s = (hipStream_t)stream;
  if (highbd)
    hipLaunchKernelGGL(comp_var_kernel<uint16_t>, dim3(comp_blocks(njobs, sh)), dim3(256), 0, s,
                       (const uint16_t*)a, a_stride, (const uint16_t*)b, b_stride, sh, w, h, jobs,
                       njobs, kind, bit_depth, (const uint16_t*)second_pred, ca, var_out, sse_out);
  else
    hipLaunchKernelGGL(comp_var_kernel<uint8_t>, dim3(comp_blocks(njobs, sh)), dim3(256), 0, s,
                       (const uint8_t*)a, a_stride, (const uint8_t*)b, b_stride, sh, w, h, jobs,
                       njobs, kind, 8, (const uint8_t*)second_pred, ca, var_out, sse_out);
  LCHK();
  return 0;
}

int lavish_obmc_batch(const void* pre, int pre_stride, int w, int h, const LavishCompJob* jobs,
                      int njobs, int npre, int kind, int bit_depth, int highbd,
                      const int32_t* wsrc, const int32_t* mask, uint32_t* out, uint32_t* sse_out,
                      void* stream) {
  if (njobs <= 0) return 0;
  CompShape sh;
  if (kind < 0 || kind > 2 || npre < 1 || npre > 4 || (kind != 0 && npre != 1)) return -1;
  if (!wsrc || !mask) return -2;
  if (!comp_shape(w, h, sh)) return -4;
  if (!bit_depth_ok(bit_depth)) return -5;
  hipStream_t s = (hipStream_t)stream;
  if (highbd)
    hipLaunchKernelGGL(obmc_kernel<uint16_t>, dim3(comp_blocks(njobs, sh)), dim3(256), 0, s,
                       (const uint16_t*)pre, pre_stride, sh, w, h, jobs, njobs, npre, kind,
                       bit_depth, wsrc, mask, out, sse_out);
  else
    hipLaunchKernelGGL(obmc_kernel<uint8_t>, dim3(comp_blocks(njobs, sh)), dim3(256), 0, s,
                       (const uint8_t*)pre, pre_stride, sh, w, h, jobs, njobs, npre, kind, 8, wsrc,
                       mask, out, sse_out);
  LCHK();
  return 0;
}

int lavish_comp_pred_batch(void* comp_pred, const void* pred, int w, int h, const void* ref,
                           int ref_stride, const LavishCompJob* jobs, int njobs, int mode,
                           const uint8_t* mask, int mask_stride, int fwd_offset, int bck_offset,
                           int highbd, void* stream) {
  if (njobs <= 0) return 0;
  CompShape sh;
  if (mode < 0 || mode > 2 || !pred || !comp_pred) return -1;
  if (mode == 2 && (!mask || mask_stride < w)) return -2;
  if (mode == 1 && !dist_offsets_ok(fwd_offset, bck_offset)) return -3;
  if (!comp_shape(w, h, sh)) return -4;
  const CompArgs ca = {mask, mask_stride, fwd_offset, bck_offset};
  hipStream_t s = (hipStream_t)stream;
  if (highbd)
    hipLaunchKernelGGL(comp_pred_kernel<uint16_t>, dim3(comp_blocks(njobs, sh)), dim3(256), 0, s,
                       (uint16_t*)comp_pred, (const uint16_t*)pred, sh, w, (const uint16_t*)ref,
                       ref_stride, jobs, njobs, mode, ca);
  else
    hipLaunchKernelGGL(comp_pred_kernel<uint8_t>, dim3(comp_blocks(njobs, sh)), dim3(256), 0, s,
                       (uint8_t*)comp_pred, (const uint8_t*)pred, sh, w, (const uint8_t*)ref,
                       ref_stride, jobs, njobs, mode, ca);
  LCHK();
  return 0;
}

}  // extern "C"
