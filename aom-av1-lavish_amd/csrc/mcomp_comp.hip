// mcomp_comp.hip -- the compound, masked and OBMC full-pixel searches, one
// wave per job (comp_kernel) and their lavish_*_batch entry points:
//   av1_full_pixel_search with ms_buffers.second_pred (av1/encoder/mcomp.c:
//     1755-1895): diamond_search_sad's second_pred branch (:1377-1405) under
//     full_pixel_diamond (:1479-1526), DIAMOND / NSTEP / NSTEP_8PT;
//   av1_refining_search_8p_c (:1683-1753);
//   av1_obmc_full_pixel_search (:2328-2342): obmc_full_pixel_diamond
//     (:2293-2326) over obmc_diamond_search_sad (:2235-2291), or
//     obmc_refining_search_sad (:2190-2233).
// The walk (diamond_walk) and the wave shape are
// mcomp_dev.h's: lane group g = lane / 8 takes one candidate site, lane l of
// the group rows l + 8k, and the keyed minimum (cost << 4 | site) over the
// groups is the reference's sequential two-stage strict-< scan.  What this
// file adds is the SAD source CompSearch<> and the refinements: the candidate
// is first combined with a job-invariant block -- the rounded average with
// second_pred (sdaf), the mask blend with it (msdf), or the weighted OBMC
// difference against wsrc (osdf).  Up to 32x32 those invariants are staged
// once per job in a per-wave LDS slice (the source stays in VGPRs); larger
// blocks re-read them through L2 with the candidate rows, in 32-byte chunks.
#include "mcomp_dev.h"

namespace lavish {
namespace {

enum { kPlain = 0, kAvg = 1, kMask = 2, kObmc = 3 };          // FORM
enum { kFullpel = 0, kRefine8 = 1, kObmcFast = 2 };            // what a launch runs

struct CompJob {
  Job base;
  int64_t second_off, mask_off;
  int32_t invert_mask, reserved;
};
static_assert(sizeof(CompJob) == sizeof(LavishCompSearchJob) && sizeof(CompJob) == 56,
              "job layout");
static_assert(sizeof(LavishCompSearchResult) == 16, "result layout");

constexpr int kInvalidMv = -32768;  // MARK_MV_INVALID

// the job-invariant operands of one job
struct Inv {
  const uint8_t* second;  // compact, stride W
  const uint8_t* mask;    // rows ms apart
  int ms, invert;
  const int32_t* wsrc;    // compact int32
  const int32_t* omask;
};

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int j) { return (w >> (8 * j)) & 255u; }

// aom_comp_mask_pred of 4 pixels: m the raw mask bytes
__device__ __forceinline__ uint32_t blend4(uint32_t r, uint32_t s, uint32_t m, int invert) {
  uint32_t p = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t mj = byte_of(m, j), mr = invert ? 64u - mj : mj;
    p |= ((mr * byte_of(r, j) + (64u - mr) * byte_of(s, j) + 32u) >> 6) << (8 * j);
  }
  return p;
}
// the same from the hoisted form: mr the ref multipliers (bytes), c01 / c23
// the 16-bit constants (64 - mr) * second + 32
__device__ __forceinline__ uint32_t blend4_hoisted(uint32_t r, uint32_t mr, uint32_t c01,
                                                   uint32_t c23) {
  const uint32_t p0 = (byte_of(mr, 0) * byte_of(r, 0) + (c01 & 0xFFFFu)) >> 6;
  const uint32_t p1 = (byte_of(mr, 1) * byte_of(r, 1) + (c01 >> 16)) >> 6;
  const uint32_t p2 = (byte_of(mr, 2) * byte_of(r, 2) + (c23 & 0xFFFFu)) >> 6;
  const uint32_t p3 = (byte_of(mr, 3) * byte_of(r, 3) + (c23 >> 16)) >> 6;
  return p0 | (p1 << 8) | (p2 << 16) | (p3 << 24);
}
// comp_avg_pred of 4 pixels: v_lerp_u8 with the rounding bit set per byte
__device__ __forceinline__ uint32_t avg4(uint32_t r, uint32_t s) {
  return __builtin_amdgcn_lerp(r, s, 0x01010101u);
}
// osdf of 4 pixels: sum of ROUND_POWER_OF_TWO(|wsrc - pre * mask|, 12)
__device__ __forceinline__ uint32_t obmc4(uint32_t r, const int32_t (&w)[4],
                                          const int32_t (&m)[4]) {
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    acc += (uint32_t)(abs(w[j] - __mul24((int)byte_of(r, j), m[j])) + 2048) >> 12;
  return acc;
}

__device__ __forceinline__ void load4_i32(const int32_t* p, int32_t (&o)[4]) {
  uint32_t t[4];
  load_row<4>((const uint8_t*)p, t);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (int32_t)t[j];
}

// LDS slice of one wave, in dwords: second_pred (W*H bytes); the hoisted
// blend (W*H multiplier bytes, then W*H 16-bit constants); wsrc and mask
// (W*H int32 each).  Only blocks up to 32x32 stage.
template <int W, int H, int FORM>
struct Slice {
  static constexpr bool kOn = W <= 32 && H <= 32 && FORM != kPlain;
  static constexpr int N = W * H;
  static constexpr int SIZE = !kOn ? 1 : FORM == kAvg ? N / 4 : FORM == kMask ? 3 * N / 4 : 2 * N;
};

template <int W, int H, int FORM>
struct CompSearch {
  using G = Geo<W, H, false>;
  using SL = Slice<W, H, FORM>;
  static constexpr int DW = G::DW, RPL = G::RPL;
  static constexpr bool kCache = W <= 32 && H <= 32;  // source in VGPRs, invariants in LDS
  uint32_t s[(kCache && FORM != kObmc) ? RPL : 1][(kCache && FORM != kObmc) ? DW : 1];
  int l;
  lds_u32 lds;
  Inv iv;

  __device__ __forceinline__ void load(const Ctx& c, int lane, const Inv& inv, lds_u32 slice) {
    l = lane & 7;
    lds = slice;
    iv = inv;
    if constexpr (kCache && FORM != kObmc) {
#pragma unroll
      for (int k = 0; k < RPL; ++k) {
        const int row = l + 8 * k;
        if (row < H) load_row<DW>(c.src + (int64_t)row * c.ss, s[k]);
      }
    }
    if constexpr (SL::kOn) {
      // the whole wave stages the invariants, one word (4 pixels) per lane
      for (int i = lane; i < H * DW; i += 64) {
        const int y = i / DW, x = i - y * DW;
        if constexpr (FORM == kAvg) {
          uint32_t t[1];
          load_row<1>(iv.second + 4 * i, t);
          lds[i] = t[0];
        } else if constexpr (FORM == kMask) {
          uint32_t t[1], m[1];
          load_row<1>(iv.second + 4 * i, t);
          load_row<1>(iv.mask + (int64_t)y * iv.ms + 4 * x, m);
          uint32_t mr = 0, cc[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t mj = byte_of(m[0], j), q = iv.invert ? 64u - mj : mj;
            mr |= q << (8 * j);
            cc[j] = (64u - q) * byte_of(t[0], j) + 32u;
          }
          lds[i] = mr;
          lds[SL::N / 4 + 2 * i] = cc[0] | (cc[1] << 16);
          lds[SL::N / 4 + 2 * i + 1] = cc[2] | (cc[3] << 16);
        } else {
          int32_t w4[4], m4[4];
          load4_i32(iv.wsrc + 4 * i, w4);
          load4_i32(iv.omask + 4 * i, m4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            lds[4 * i + j] = (uint32_t)w4[j];
            lds[SL::N + 4 * i + j] = (uint32_t)m4[j];
          }
        }
      }
      wave_sync();
    }
  }

  // the combined SAD of word wi (= row * DW + i) against candidate word r,
  // invariants from LDS
  __device__ __forceinline__ uint32_t word_lds(uint32_t sw, uint32_t r, int wi, uint32_t acc) const {
    if constexpr (FORM == kPlain) {
      return sad4(sw, r, acc);
    } else if constexpr (FORM == kAvg) {
      return sad4(sw, avg4(r, lds[wi]), acc);
    } else if constexpr (FORM == kMask) {
      return sad4(sw, blend4_hoisted(r, lds[wi], lds[SL::N / 4 + 2 * wi],
                                     lds[SL::N / 4 + 2 * wi + 1]), acc);
    } else {
      int32_t w4[4], m4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w4[j] = (int32_t)lds[4 * wi + j];
        m4[j] = (int32_t)lds[SL::N + 4 * wi + j];
      }
      return acc + obmc4(r, w4, m4);
    }
  }
  // the same with the invariants (and the source) from global memory: word
  // x of row y
  __device__ __forceinline__ uint32_t word_mem(const Ctx& c, uint32_t r, int y, int x,
                                               uint32_t acc) const {
    if constexpr (FORM == kObmc) {
      int32_t w4[4], m4[4];
      load4_i32(iv.wsrc + (y * W + 4 * x), w4);
      load4_i32(iv.omask + (y * W + 4 * x), m4);
      return acc + obmc4(r, w4, m4);
    } else {
      uint32_t sw[1];
      load_row<1>(c.src + (int64_t)y * c.ss + 4 * x, sw);
      return sad4(sw[0], pred_mem(r, y, x), acc);
    }
  }
  // comp_avg_pred / comp_mask_pred word x of row y, invariants from global
  __device__ __forceinline__ uint32_t pred_mem(uint32_t r, int y, int x) const {
    if constexpr (FORM == kAvg) {
      uint32_t t[1];
      load_row<1>(iv.second + (y * W + 4 * x), t);
      return avg4(r, t[0]);
    } else if constexpr (FORM == kMask) {
      uint32_t t[1], m[1];
      load_row<1>(iv.second + (y * W + 4 * x), t);
      load_row<1>(iv.mask + (int64_t)y * iv.ms + 4 * x, m);
      return blend4(r, t[0], m[0], iv.invert);
    } else {
      return r;
    }
  }

  // group SAD of the candidate at mv (r, cc), reduced over the 8 lanes; a
  // group whose candidate is not valid reads the block at (sr, sc) instead
  __device__ __forceinline__ uint32_t group_sad(const Ctx& c, int r, int cc, bool valid, int sr,
                                                int sc) const {
    r = valid ? r : sr;
    cc = valid ? cc : sc;
    const uint8_t* base = c.ref + ((int64_t)__mul24(r, c.rs) + cc);
    uint32_t acc = 0;
    if constexpr (kCache) {
      // every candidate row in flight first, then row by row: the compiler
      // barrier keeps the invariants' LDS reads of one row from being
      // hoisted above the previous row (or out of the step loop) -- all of
      // them live at once cost 464 VGPRs (mask) or spilled (OBMC) at 32x32
      uint32_t rw[RPL][DW];
#pragma unroll
      for (int k = 0; k < RPL; ++k) {
        const int row = l + 8 * k;
        if (row < H) load_row<DW>(base + (int64_t)row * c.rs, rw[k]);
      }
#pragma unroll
      for (int k = 0; k < RPL; ++k) {
        const int row = l + 8 * k;
        if constexpr (FORM != kPlain) asm volatile("" ::: "memory");
        if (row < H) {
#pragma unroll
          for (int i = 0; i < DW; ++i) {
            if constexpr (FORM == kObmc) acc = word_lds(0, rw[k][i], row * DW + i, acc);
            else acc = word_lds(s[k][i], rw[k][i], row * DW + i, acc);
          }
        }
      }
    } else {
      acc = chunk_rows<DW, RPL, 1>(
          base, c.rs, l, [&](const uint32_t (&rw)[kChunk<DW>], int y, int x, uint32_t a) {
#pragma unroll
            for (int i = 0; i < kChunk<DW>; ++i) a = word_mem(c, rw[i], y, x + i, a);
            return a;
          });
    }
    return group_sum8(acc);
  }

  // get_mvpred_compound_var_cost / get_obmc_mvpred_var at (row, col): the
  // whole wave walks the block one word per lane, everything from global
  // memory (once per run)
  __device__ int var_cost_at(const Ctx& c, int lane, int row, int col) const {
    return var_walk<W, H>(
        c, lane, row, col, nullptr,
        [&](const uint8_t* rp, int i, int y, int x, int& sum, uint32_t& sse) {
          uint32_t b[1];
          load_row<1>(rp, b);
          if constexpr (FORM == kObmc) {
            int32_t w4[4], m4[4];
            load4_i32(iv.wsrc + 4 * i, w4);
            load4_i32(iv.omask + 4 * i, m4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              // ROUND_POWER_OF_TWO_SIGNED(wsrc - pre * mask, 12)
              const int v = w4[j] - __mul24((int)byte_of(b[0], j), m4[j]);
              const int rnd = (abs(v) + 2048) >> 12, d = v < 0 ? -rnd : rnd;
              sum += d;
              sse += (uint32_t)(d * d);
            }
          } else {
            uint32_t a[1];
            load_row<1>(c.src + (int64_t)y * c.ss + 4 * x, a);
            var_acc(a[0], pred_mem(b[0], y, x), sum, sse);
          }
        });
  }
};

// neighbour j of av1_refining_search_8p_c: (-1,0) (0,-1) (0,1) (1,0) (-1,-1)
// (1,-1) (-1,1) (1,1); the first four are obmc_refining_search_sad's.
// Packed as 2-bit (d + 1) fields
__device__ __forceinline__ int nb_dr(int j) { return ((0x8894 >> (2 * j)) & 3) - 1; }
__device__ __forceinline__ int nb_dc(int j) { return ((0xA061 >> (2 * j)) & 3) - 1; }

// av1_refining_search_8p_c (GRID: 8 neighbours, 3 rounds, the visited grid)
// or obmc_refining_search_sad (4 neighbours, 8 rounds): returns best_sad
template <bool GRID, class S_t>
__device__ __forceinline__ uint32_t refine(const S_t& S, const Ctx& c, int lane, int srow,
                                           int scol, uint32_t c0, int& brow, int& bcol,
                                           int& steps) {
  const int g = lane >> 3;
  const int dr = nb_dr(g), dc = nb_dc(g);
  int row = srow, col = scol;
  uint32_t best = c0;
  // do_refine_search_grid: 7 x 7 around the start (the centre moves at most
  // 2 before the last round, its neighbours lie within 3)
  auto bit = [&](int r, int cc) { return 1ull << ((r - srow + 3) * 7 + (cc - scol + 3)); };
  uint64_t seen = bit(row, col);
  for (int i = 0; i < (GRID ? 3 : 8); ++i) {
    const int r = row + dr, cc = col + dc;
    bool valid = cc >= c.col_min && cc <= c.col_max && r >= c.row_min && r <= c.row_max;
    if constexpr (GRID) {
      valid = valid && !(seen & bit(r, cc));
#pragma unroll
      for (int j = 0; j < 8; ++j) seen |= bit(row + nb_dr(j), col + nb_dc(j));
    } else {
      valid = valid && g < 4;
    }
    const MvRate mr = mvsad_rate(c, r, cc);
    const uint32_t mine = S.group_sad(c, r, cc, valid, row, col);
    const uint32_t mvs = mvsad_finish(c, mr, r, cc);
    const uint32_t kmin = groups_min((((mine + mvs) << 3) | (uint32_t)g) | (valid ? 0u : ~0u));
    ++steps;
    if (kmin >= (best << 3)) break;
    best = kmin >> 3;
    row += nb_dr((int)(kmin & 7));
    col += nb_dc((int)(kmin & 7));
  }
  brow = row;
  bcol = col;
  return best;
}

template <int W, int H, int FORM>
__global__ __launch_bounds__(64 * kDkWaves) void comp_kernel(
    const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs,
    const CompJob* __restrict__ jobs, int njobs, int what, int method, int step_param,
    LavishMvCostParams cost, const uint8_t* __restrict__ second, const uint8_t* __restrict__ mask,
    int mask_stride, const int32_t* __restrict__ wsrc, const int32_t* __restrict__ omask,
    LavishCompSearchResult* __restrict__ out) {
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = wg * kDkWaves + wave;
  if (j >= njobs) return;
  using SL = Slice<W, H, FORM>;
  __shared__ __attribute__((aligned(16))) uint32_t slice_s[kDkWaves * SL::SIZE];
  const lds_u32 slice = (lds_u32)(slice_s + wave * SL::SIZE);
  const CompJob jb = jobs[j];
  // (an OBMC job has no source: its Ctx source is the reference, never read)
  const Ctx c = job_ctx(FORM == kObmc ? ref : src, ss, ref, rs, jb.base, cost);
  Inv iv;
  iv.second = second + jb.second_off;
  iv.mask = mask + jb.mask_off;
  iv.ms = mask_stride;
  iv.invert = jb.invert_mask;
  iv.wsrc = wsrc + jb.second_off;
  iv.omask = omask + jb.mask_off;
  CompSearch<W, H, FORM> S;
  S.load(c, lane, iv, slice);

  // clamp_fullmv; every run starts here, its cost is read once
  const int srow = min(max((int)jb.base.start_row, c.row_min), c.row_max);
  const int scol = min(max((int)jb.base.start_col, c.col_min), c.col_max);
  const uint32_t c0 = rdlane(S.group_sad(c, srow, scol, true, srow, scol), 0) +
                      mvsad_cost(c, srow, scol);
  int br = srow, bc = scol, steps = 0, sme;
  int sec_r = kInvalidMv, sec_c = kInvalidMv;
  if (what == kRefine8) {
    sme = (int)refine<true>(S, c, lane, srow, scol, c0, br, bc, steps);
    sec_r = br;
    sec_c = bc;
  } else if (what == kObmcFast) {
    refine<false>(S, c, lane, srow, scol, c0, br, bc, steps);
    sme = S.var_cost_at(c, lane, br, bc);
  } else {
    // full_pixel_diamond / obmc_full_pixel_diamond
    constexpr bool OB = FORM == kObmc;
    int n, num00 = 0;
    diamond_walk<true, OB>(S, c, lane, method, srow, scol, c0, step_param, br, bc, n, steps,
                           &sec_r, &sec_c);
    sme = S.var_cost_at(c, lane, br, bc);
    const int further = method_steps(method) - 1 - step_param;
    while (n < further) {
      ++n;
      if (OB && num00) {
        --num00;
        continue;
      }
      int tr, tc;
      diamond_walk<true, OB>(S, c, lane, method, srow, scol, c0, step_param + n, tr, tc, num00,
                             steps, &sec_r, &sec_c);
      const int t = S.var_cost_at(c, lane, tr, tc);
      if (t < sme) {
        sme = t;
        br = tr;
        bc = tc;
      }
      if (!OB && num00) {
        n += num00;
        num00 = 0;
      }
    }
    if (OB) sec_r = sec_c = kInvalidMv;
  }
  if (lane == 0) {
    LavishCompSearchResult r;
    r.best_row = (int16_t)br;
    r.best_col = (int16_t)bc;
    r.second_row = (int16_t)sec_r;
    r.second_col = (int16_t)sec_c;
    r.bestsme = sme;
    r.steps = steps;
    out[j] = r;
  }
}

template <int W, int H, int FORM>
void launch_comp(const uint8_t* src, int ss, const uint8_t* ref, int rs,
                 const LavishCompSearchJob* jobs, int njobs, int what, int method,
                 int step_param, const LavishMvCostParams& cost, const uint8_t* second,
                 const uint8_t* mask, int mask_stride, const int32_t* wsrc,
                 const int32_t* omask, LavishCompSearchResult* out, hipStream_t s) {
  const int nwg = xcd_grid((njobs + kDkWaves - 1) / kDkWaves);
  hipLaunchKernelGGL((comp_kernel<W, H, FORM>), dim3(nwg), dim3(64 * kDkWaves), 0, s, src, ss,
                     ref, rs, (const CompJob*)jobs, njobs, what, method, step_param, cost, second,
                     mask, mask_stride, wsrc, omask, out);
}

// the checks the step-taking entry points share; with the NULL checks and
// comp_batch's size dispatch (-3) everything is refused before any device work
int comp_args_ok(int method, int step_param, const LavishMvCostParams* cost) {
  if (!diamond_method(method)) return -4;
  if (step_param < 0 || step_param >= method_steps(method)) return -1;
  if (!mv_cost_ok(cost)) return -2;
  return 0;
}

int comp_batch(const uint8_t* src, int ss, const uint8_t* ref, int rs, int w, int h,
               const LavishCompSearchJob* jobs, int njobs, int what, int form, int method,
               int step_param, const LavishMvCostParams* cost, const uint8_t* second,
               const uint8_t* mask, int mask_stride, const int32_t* wsrc, const int32_t* omask,
               LavishCompSearchResult* out, hipStream_t s) {
#define LAVISH_COMP_CASE(W, H)                                                                \
  if (w == W && h == H) {                                                                     \
    if (form == kObmc)                                                                        \
      launch_comp<W, H, kObmc>(src, ss, ref, rs, jobs, njobs, what, method, step_param,       \
                               *cost, second, mask, mask_stride, wsrc, omask, out, s);        \
    else if (form == kMask)                                                                   \
      launch_comp<W, H, kMask>(src, ss, ref, rs, jobs, njobs, what, method, step_param,       \
                               *cost, second, mask, mask_stride, wsrc, omask, out, s);        \
    else if (form == kAvg)                                                                    \
      launch_comp<W, H, kAvg>(src, ss, ref, rs, jobs, njobs, what, method, step_param, *cost, \
                              second, mask, mask_stride, wsrc, omask, out, s);                \
    else                                                                                      \
      launch_comp<W, H, kPlain>(src, ss, ref, rs, jobs, njobs, what, method, step_param,      \
                                *cost, second, mask, mask_stride, wsrc, omask, out, s);       \
    LAVISH_CHECK(hipGetLastError());                                                          \
    return 0;                                                                                 \
  }
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_COMP_CASE)
#undef LAVISH_COMP_CASE
  return -3;
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" int lavish_comp_full_pixel_search_batch(
    const uint8_t* src, int src_stride, const uint8_t* ref, int ref_stride, int w, int h,
    const LavishCompSearchJob* jobs, int njobs, int search_method, int step_param,
    const LavishMvCostParams* cost, const uint8_t* second_pred, const uint8_t* mask,
    int mask_stride, LavishCompSearchResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = comp_args_ok(search_method, step_param, cost)) return rc;
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      second_pred == nullptr || (mask != nullptr && mask_stride < w))
    return -7;
  return comp_batch(src, src_stride, ref, ref_stride, w, h, jobs, njobs, kFullpel,
                    mask ? kMask : kAvg, search_method, step_param, cost, second_pred, mask,
                    mask_stride, nullptr, nullptr, out, (hipStream_t)stream);
}

extern "C" int lavish_refining_search_8p_batch(
    const uint8_t* src, int src_stride, const uint8_t* ref, int ref_stride, int w, int h,
    const LavishCompSearchJob* jobs, int njobs, const LavishMvCostParams* cost,
    const uint8_t* second_pred, const uint8_t* mask, int mask_stride,
    LavishCompSearchResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (!mv_cost_ok(cost)) return -2;
  // (a mask without second_pred has nothing to blend with)
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      (mask != nullptr && (second_pred == nullptr || mask_stride < w)))
    return -7;
  const int form = mask ? kMask : second_pred ? kAvg : kPlain;
  return comp_batch(src, src_stride, ref, ref_stride, w, h, jobs, njobs, kRefine8, form, kDiamond,
                    0, cost, second_pred, mask, mask_stride, nullptr, nullptr, out,
                    (hipStream_t)stream);
}

extern "C" int lavish_obmc_full_pixel_search_batch(
    const uint8_t* ref, int ref_stride, int w, int h, const LavishCompSearchJob* jobs, int njobs,
    int search_method, int step_param, const LavishMvCostParams* cost, int fast_obmc_search,
    const int32_t* wsrc, const int32_t* obmc_mask, LavishCompSearchResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = comp_args_ok(search_method, step_param, cost)) return rc;
  if (ref == nullptr || jobs == nullptr || out == nullptr || wsrc == nullptr ||
      obmc_mask == nullptr)
    return -7;
  return comp_batch(nullptr, ref_stride, ref, ref_stride, w, h, jobs, njobs,
                    fast_obmc_search ? kObmcFast : kFullpel, kObmc, search_method, step_param,
                    cost, nullptr, nullptr, 0, wsrc, obmc_mask, out, (hipStream_t)stream);
}
