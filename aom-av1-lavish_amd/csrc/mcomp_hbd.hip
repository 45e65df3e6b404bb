// mcomp_hbd.hip -- the high-bit-depth full-pixel search, one wave per job
// (hbd_fullpel_kernel) and lavish_highbd_full_pixel_search_batch:
//   av1_full_pixel_search (av1/encoder/mcomp.c:1755-1873, no mesh) of
//   DIAMOND / NSTEP / NSTEP_8PT over uint16_t planes with the high-bit-depth
//   members of aom_variance_fn_ptr_t as highbd_set_var_fns binds them
//   (av1/encoder/encoder_utils.h:130-230,572-): sdf / sdx4df / sdsf =
//   aom_highbd_sad{W}x{H}[x4d] / aom_highbd_sad_skip_{W}x{H} under the
//   _bits8 / _bits10 / _bits12 wrappers (the whole block's SAD >> 0 / 2 / 4),
//   vf = aom_highbd_{8,10,12}_variance{W}x{H} (aom_dsp/variance.c:321-408).
// The walk (diamond_walk), the cost list (int_sad_list) and the wave shape are
// mcomp_dev.h's: lane group g = lane / 8 takes one candidate site, lane l of
// the group rows l + 8k.  What this file adds is the SAD source HbdSearch<>:
// a row is W / 2 dwords of two pixels, v_sad_u16 accumulates them, and the
// depth's shift is applied to the group's reduced SAD -- the whole block's --
// before the mv SAD cost is added.  Everything is addressed in bytes inside
// (the Ctx strides are byte strides); the entry point takes elements.
//
// The source stays in VGPRs while it is at most 32 dwords per lane (32x16,
// 16x32 and smaller: half the pixels of the 8-bit search, the same bytes);
// larger blocks re-read it through L2 with the candidate rows, in 32-byte
// chunks (chunk_rows).
//
// What a call reads: the W x H source block of each job, and the W x H
// reference block at every mv inside the job's limits -- rows of exactly
// 2 * W bytes at the pixel's own address (byte-addressed dwordx4 / dwordx2
// loads), nothing before a row's first element or past its last.
#include "mcomp_dev.h"

namespace lavish {
namespace {

template <int W, int H, bool SKIP>
struct HbdSearch {
  using G = Geo<2 * W, H, SKIP>;  // in bytes: DW = W / 2 dwords per row
  static constexpr int DW = G::DW, RPL = G::RPL;
  static constexpr bool kCache = RPL * DW <= 32;
  uint32_t s[kCache ? RPL : 1][kCache ? DW : 1];
  int l, sh;

  __device__ __forceinline__ void load(const Ctx& c, int lane, int shift) {
    l = lane & 7;
    sh = shift;
    if constexpr (kCache) {
#pragma unroll
      for (int k = 0; k < RPL; ++k) {
        const int row = l + 8 * k;
        if (row < G::RH) load_row<DW>(c.src + (int64_t)row * G::YS * c.ss, s[k]);
      }
    }
  }

  // the _bitsN SAD of the candidate at mv (r, cc): the group's 8 lanes reduce
  // the block's SAD (twice the even rows' when SKIP), then the depth's shift;
  // a group whose candidate is not valid reads the block at (sr, sc) instead
  __device__ __forceinline__ uint32_t group_sad(const Ctx& c, int r, int cc, bool valid, int sr,
                                                int sc) const {
    r = valid ? r : sr;
    cc = valid ? cc : sc;
    const uint8_t* base = c.ref + ((int64_t)r * c.rs + 2 * cc);
    uint32_t acc = 0;
    if constexpr (kCache) {
      uint32_t rw[RPL][DW];
#pragma unroll
      for (int k = 0; k < RPL; ++k) {
        const int row = l + 8 * k;
        if (row < G::RH) load_row<DW>(base + (int64_t)row * G::YS * c.rs, rw[k]);
      }
#pragma unroll
      for (int k = 0; k < RPL; ++k) {
        const int row = l + 8 * k;
        if (row < G::RH) {
#pragma unroll
          for (int i = 0; i < DW; ++i) acc = sad2(s[k][i], rw[k][i], acc);
        }
      }
    } else {
      constexpr int CH = kChunk<DW>;
      acc = chunk_rows<DW, RPL, G::YS>(
          base, c.rs, l, [&](const uint32_t (&rw)[CH], int y, int x, uint32_t a) {
            uint32_t q[CH];
            load_row<CH>(c.src + (int64_t)y * c.ss + 4 * x, q);
#pragma unroll
            for (int i = 0; i < CH; ++i) a = sad2(q[i], rw[i], a);
            return a;
          });
    }
    acc = group_sum8(acc);
    return (SKIP ? 2 * acc : acc) >> sh;
  }
};

// one 4-pixel unit (two dwords) of source a and reference b
__device__ __forceinline__ void hbd_acc4(const uint32_t (&a)[2], const uint32_t (&b)[2], int& sum,
                                         uint32_t& sse, uint32_t& sad) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int d0 = (int)(a[j] & 0xFFFFu) - (int)(b[j] & 0xFFFFu);
    const int d1 = (int)(a[j] >> 16) - (int)(b[j] >> 16);
    sum += d0 + d1;
    sse += (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1);
    sad = sad2(a[j], b[j], sad);
  }
}

// get_mvpred_var_cost (vf + mv_err_cost) at a full-pel mv: the whole wave
// walks the block one 4-pixel unit per lane, from global memory.  A lane sees
// at most 256 pixels: its sse stays below 2^32 (256 * 4095^2)
template <int W, int H>
__device__ int hbd_var_cost(const Ctx& c, int lane, int row, int col, int sh) {
  constexpr int UW = W / 4;
  int sum = 0;
  uint32_t sse = 0, sad = 0;
  const uint8_t* rb = c.ref + ((int64_t)row * c.rs + 2 * col);
  for (int i = lane; i < H * UW; i += 64) {
    const int y = i / UW, x = i - y * UW;
    uint32_t a[2], b[2];
    load_row<2>(c.src + (int64_t)y * c.ss + 8 * x, a);
    load_row<2>(rb + (int64_t)y * c.rs + 8 * x, b);
    hbd_acc4(a, b, sum, sse, sad);
  }
  const int ts = (int)groups_sum(group_sum8((uint32_t)sum));  // |.| <= 2^14 * 4095
  const uint64_t tq = groups_sum64(sse);
  return (int)hbd_var_tail(ts, tq, sh, W * H) + mv_cost(c, row, col);
}

// sdf and sdsf under their _bitsN wrappers at a full-pel mv in one pass
template <int W, int H>
__device__ void hbd_sad_and_skip(const Ctx& c, int lane, int row, int col, int sh, int& sad,
                                 int& ssad) {
  constexpr int UW = W / 4;
  uint32_t all = 0, even = 0;
  const uint8_t* rb = c.ref + ((int64_t)row * c.rs + 2 * col);
  for (int i = lane; i < H * UW; i += 64) {
    const int y = i / UW, x = i - y * UW;
    uint32_t a[2], b[2];
    load_row<2>(c.src + (int64_t)y * c.ss + 8 * x, a);
    load_row<2>(rb + (int64_t)y * c.rs + 8 * x, b);
    const uint32_t d = sad2(a[1], b[1], sad2(a[0], b[0], 0));
    all += d;
    even += (y & 1) ? 0u : d;
  }
  const uint32_t ta = groups_sum(group_sum8(all)), te = groups_sum(group_sum8(even));
  sad = (int)(ta >> sh);
  ssad = (int)((2 * te) >> sh);
}

// full_pixel_diamond (mcomp.c:1479-1526) over HbdSearch: every run starts at
// the same clamped start_mv, whose SAD is read once
template <int W, int H, bool SKIP>
__device__ int hbd_full_pixel_diamond(const Ctx& c, int lane, int sh, int srow, int scol,
                                      int step_param, int method, int& brow, int& bcol,
                                      int& steps, int& searches, bool want_cl, int (&cl)[5]) {
  HbdSearch<W, H, SKIP> S;
  S.load(c, lane, sh);
  srow = min(max(srow, c.row_min), c.row_max);
  scol = min(max(scol, c.col_min), c.col_max);
  const uint32_t c0 =
      rdlane(S.group_sad(c, srow, scol, true, srow, scol), 0) + mvsad_cost(c, srow, scol);
  int n, num00 = 0;
  diamond_walk<false, false>(S, c, lane, method, srow, scol, c0, step_param, brow, bcol, n,
                             steps);
  ++searches;
  int bestsme = hbd_var_cost<W, H>(c, lane, brow, bcol, sh);
  const int further = method_steps(method) - 1 - step_param;
  while (n < further) {
    ++n;
    int tr, tc;
    diamond_walk<false, false>(S, c, lane, method, srow, scol, c0, step_param + n, tr, tc, num00,
                               steps);
    ++searches;
    const int sme = hbd_var_cost<W, H>(c, lane, tr, tc, sh);
    if (sme < bestsme) {
      bestsme = sme;
      brow = tr;
      bcol = tc;
    }
    if (num00) {
      n += num00;
      num00 = 0;
    }
  }
  if (want_cl) int_sad_list(S, c, lane, brow, bcol, false, cl);
  return bestsme;
}

template <int W, int H>
__global__ __launch_bounds__(64 * kDkWaves) void hbd_fullpel_kernel(
    const uint16_t* __restrict__ src, int ss, const uint16_t* __restrict__ ref, int rs,
    const Job* __restrict__ jobs, int njobs, int sh, int method, int step_param,
    LavishMvCostParams cost, int skip, LavishDiamondResult* __restrict__ out,
    int32_t* __restrict__ cost_lists) {
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = wg * kDkWaves + wave;
  if (j >= njobs) return;
  Job jb = jobs[j];
  jb.src_off *= 2;  // elements -> bytes
  jb.ref_off *= 2;
  const Ctx c = job_ctx((const uint8_t*)src, 2 * ss, (const uint8_t*)ref, 2 * rs, jb, cost);
  const bool want_cl = cost_lists != nullptr;
  int cl[5] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  int br, bc, steps = 0, searches = 0, sme;
  // use_downsampled_sad applies to blocks at least 16 high (mcomp.c:132-133)
  if (skip && H >= 16) {
    sme = hbd_full_pixel_diamond<W, H, (H >= 16)>(c, lane, sh, jb.start_row, jb.start_col,
                                                  step_param, method, br, bc, steps, searches,
                                                  want_cl, cl);
    // quality check of the row-skipping search (mcomp.c:1840-1867), on the
    // wrapped (shifted) SADs
    int sad, ssad;
    hbd_sad_and_skip<W, H>(c, lane, br, bc, sh, sad, ssad);
    const int thresh = (W >> 2) * (H >> 2);
    if (sad > thresh && abs(ssad - sad) * 10 >= max(sad, 1) * 9)
      sme = hbd_full_pixel_diamond<W, H, false>(c, lane, sh, jb.start_row, jb.start_col,
                                                step_param, method, br, bc, steps, searches,
                                                want_cl, cl);
  } else {
    sme = hbd_full_pixel_diamond<W, H, false>(c, lane, sh, jb.start_row, jb.start_col,
                                              step_param, method, br, bc, steps, searches,
                                              want_cl, cl);
  }
  if (lane == 0) {
    LavishDiamondResult r;
    r.best_row = (int16_t)br;
    r.best_col = (int16_t)bc;
    r.bestsme = sme;
    r.steps = steps;
    r.searches = searches;
    out[j] = r;
  }
  if (want_cl && lane < 5) {
    const int v = lane == 0 ? cl[0] : lane == 1 ? cl[1] : lane == 2 ? cl[2] : lane == 3 ? cl[3] : cl[4];
    cost_lists[5 * (int64_t)j + lane] = v;
  }
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" int lavish_highbd_full_pixel_search_batch(
    const uint16_t* src, int src_stride, const uint16_t* ref, int ref_stride, int w, int h,
    int bit_depth, const LavishDiamondJob* jobs, int njobs, int search_method, int step_param,
    const LavishMvCostParams* cost, int use_downsampled_sad, LavishDiamondResult* out,
    int32_t* cost_lists, void* stream) {
  if (njobs <= 0) return 0;
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      !bd_ok(bit_depth, 1))
    return -7;
  if (!diamond_method(search_method)) return -4;  // (the pattern searches: packed u8 only)
  if (step_param < 0 || step_param >= method_steps(search_method)) return -1;
  if (!mv_cost_ok(cost)) return -2;
  const int nwg = xcd_grid((njobs + kDkWaves - 1) / kDkWaves);
#define LAVISH_HBD_CASE(W, H)                                                                 \
  if (w == W && h == H) {                                                                     \
    hipLaunchKernelGGL((hbd_fullpel_kernel<W, H>), dim3(nwg), dim3(64 * kDkWaves), 0,         \
                       (hipStream_t)stream, src, src_stride, ref, ref_stride,                 \
                       (const Job*)jobs, njobs, bit_depth - 8, search_method, step_param,     \
                       *cost, use_downsampled_sad, out, cost_lists);                          \
    LAVISH_CHECK(hipGetLastError());                                                          \
    return 0;                                                                                 \
  }
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_HBD_CASE)
#undef LAVISH_HBD_CASE
  return -3;
}
