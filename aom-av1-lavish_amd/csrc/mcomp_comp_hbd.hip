// mcomp_comp_hbd.hip -- the high-bit-depth compound, masked and OBMC
// full-pixel searches, one wave per job (hbd_csearch_kernel) and their
// lavish_highbd_*_batch entry points: mcomp_comp.hip's three searches
//   av1_full_pixel_search with ms_buffers.second_pred (av1/encoder/mcomp.c:
//     1755-1895), DIAMOND / NSTEP / NSTEP_8PT;
//   av1_refining_search_8p_c (:1683-1753);
//   av1_obmc_full_pixel_search (:2328-2342), both fast_obmc_search branches
// over uint16_t planes with the members highbd_set_var_fns binds
// (av1/encoder/encoder_utils.h): sdaf = aom_highbd_sad{W}x{H}_avg, msdf =
// aom_highbd_masked_sad{W}x{H}, osdf = aom_highbd_obmc_sad{W}x{H} under their
// _bits8 / _bits10 / _bits12 wrappers (the whole block's SAD >> 0 / 2 / 4,
// before the mv SAD cost is added), svaf / msvf at offset (0, 0) and ovf =
// aom_highbd_{8,10,12}_... (aom_dsp/variance.c; 8 bits truncate the sums,
// 10 / 12 round them and clamp the variance at 0: hbd_var_tail).
//
// The walk (diamond_walk) and the wave shape are mcomp_dev.h's: lane group
// g = lane / 8 takes one candidate site, lane l of the group rows l + 8k.
// What this file adds is the SAD source HbdCompSearch<>: a row is W / 2 dwords
// of two pixels; the candidate is combined with the job-invariant block --
// the rounded average with second_pred, the A64 blend with it (its 12-bit
// sum m * a + (64 - m) * b + 32 needs 18 bits: computed per pixel in 32, no
// hoisted 16-bit constant), or the weighted OBMC difference against wsrc
// (pre * mask and wsrc stay below 2^24: v_mul_i32_i24) -- and v_sad_u16
// accumulates the packed pairs.
//
// Where the invariants live: blocks of at most 512 pixels (32x16, 16x32 and
// smaller) keep the source in VGPRs (32 dwords per lane, as HbdSearch) and
// stage second_pred / the folded mask / wsrc and obmc_mask once per job in a
// per-wave LDS slice (2, 3 and 8 bytes per pixel: at most 16 KB per
// workgroup of four waves); larger blocks re-read them through L2 with the
// candidate rows, in 32-byte chunks.  Everything is addressed in bytes
// inside; the entry points take elements.
//
// What a call reads: the W x H source, second_pred, mask, wsrc and obmc_mask
// blocks of each job, and the W x H reference block at every mv inside the
// job's limits -- rows of exactly 2 * W bytes at the pixel's own address.
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

constexpr int kInvalidMv = -32768;  // MARK_MV_INVALID

// the job-invariant operands of one job (byte pointers)
struct Inv {
  const uint8_t* second;  // u16, compact, stride W
  const uint8_t* mask;    // u8, rows ms apart
  int ms, invert;
  const uint8_t* wsrc;    // int32, compact
  const uint8_t* omask;
};

__device__ __forceinline__ uint32_t lo16(uint32_t w) { return w & 0xFFFFu; }
__device__ __forceinline__ uint32_t hi16(uint32_t w) { return w >> 16; }

// aom_highbd_comp_avg_pred of 2 pixels
__device__ __forceinline__ uint32_t avg2(uint32_t r, uint32_t s) {
  return ((lo16(r) + lo16(s) + 1u) >> 1) | (((hi16(r) + hi16(s) + 1u) >> 1) << 16);
}
// aom_highbd_comp_mask_pred of 2 pixels: m0 / m1 the candidate's weights
// (invert_mask folded in)
__device__ __forceinline__ uint32_t blend2(uint32_t r, uint32_t s, uint32_t m0, uint32_t m1) {
  const uint32_t p0 = (m0 * lo16(r) + (64u - m0) * lo16(s) + 32u) >> 6;
  const uint32_t p1 = (m1 * hi16(r) + (64u - m1) * hi16(s) + 32u) >> 6;
  return p0 | (p1 << 16);
}
// the blend weights of the candidate: the mask bytes, or 64 - them
__device__ __forceinline__ uint32_t fold_mask(uint32_t m, int invert) {
  return invert ? 0x40404040u - m : m;  // (every byte <= 64: no borrow)
}
// osdf of 2 pixels: sum of ROUND_POWER_OF_TWO(|wsrc - pre * mask|, 12)
__device__ __forceinline__ uint32_t obmc2(uint32_t r, int w0, int w1, int m0, int m1) {
  return ((uint32_t)(abs(w0 - __mul24((int)lo16(r), m0)) + 2048) >> 12) +
         ((uint32_t)(abs(w1 - __mul24((int)hi16(r), m1)) + 2048) >> 12);
}
// ROUND_POWER_OF_TWO_SIGNED(wsrc - pre * mask, 12) into (sum, sse)
__device__ __forceinline__ void obmc_acc(int pre, int w, int m, int& sum, uint32_t& sse) {
  const int v = w - __mul24(pre, m);
  const int rnd = (abs(v) + 2048) >> 12, d = v < 0 ? -rnd : rnd;
  sum += d;
  sse += (uint32_t)(d * d);
}
// LDS slice of one wave, in dwords: second_pred (N / 2); with a mask the
// folded weights after it (N / 4); OBMC wsrc and mask (N each)
template <int W, int H, int FORM>
struct Slice {
  static constexpr int N = W * H;
  static constexpr bool kOn = N <= 512 && FORM != kPlain;
  static constexpr int SIZE = !kOn ? 1 : FORM == kAvg ? N / 2 : FORM == kMask ? 3 * N / 4 : 2 * N;
};

template <int W, int H, int FORM>
struct HbdCompSearch {
  using G = Geo<2 * W, H, false>;  // in bytes: DW = W / 2 dwords per row
  using SL = Slice<W, H, FORM>;
  static constexpr int DW = G::DW, RPL = G::RPL, N = W * H;
  static constexpr bool kCache = N <= 512;  // source in VGPRs, invariants in LDS
  static_assert(kCache == (RPL * DW <= 32) || H < 8, "the cached source fits 32 dwords a lane");
  static_assert(kCache || DW % 8 == 0, "uncached rows are whole 32-byte chunks");
  static constexpr bool kSrc = kCache && FORM != kObmc;
  uint32_t s[kSrc ? RPL : 1][kSrc ? DW : 1];
  int l, sh;
  lds_u32 lds;
  Inv iv;

  __device__ __forceinline__ void load(const Ctx& c, int lane, int shift, const Inv& inv,
                                       lds_u32 slice) {
    l = lane & 7;
    sh = shift;
    lds = slice;
    iv = inv;
    if constexpr (kSrc) {
#pragma unroll
      for (int k = 0; k < RPL; ++k) {
        const int row = l + 8 * k;
        if (row < H) load_row<DW>(c.src + (int64_t)row * c.ss, s[k]);
      }
    }
    if constexpr (SL::kOn) {
      // the whole wave stages the invariants, one dword (2 pixels) per lane
      for (int i = lane; i < N / 2; i += 64) {
        if constexpr (FORM == kObmc) {
          uint32_t w2[2], m2[2];
          load_row<2>(iv.wsrc + 8 * i, w2);
          load_row<2>(iv.omask + 8 * i, m2);
          lds[2 * i] = w2[0];
          lds[2 * i + 1] = w2[1];
          lds[N + 2 * i] = m2[0];
          lds[N + 2 * i + 1] = m2[1];
        } else {
          uint32_t t[1];
          load_row<1>(iv.second + 4 * i, t);
          lds[i] = t[0];
        }
      }
      if constexpr (FORM == kMask) {
        // the weights, one dword (4 pixels) per lane
        for (int i = lane; i < N / 4; i += 64) {
          const int y = i / (W / 4), x = i - y * (W / 4);
          uint32_t m[1];
          load_row<1>(iv.mask + (int64_t)y * iv.ms + 4 * x, m);
          lds[N / 2 + i] = fold_mask(m[0], iv.invert);
        }
      }
      wave_sync();
    }
  }

  // the combined SAD of dword wi (= row * DW + i) against candidate dword r,
  // invariants from LDS
  __device__ __forceinline__ uint32_t word_lds(uint32_t sw, uint32_t r, int wi, uint32_t acc) const {
    if constexpr (FORM == kPlain) {
      return sad2(sw, r, acc);
    } else if constexpr (FORM == kAvg) {
      return sad2(sw, avg2(r, lds[wi]), acc);
    } else if constexpr (FORM == kMask) {
      const uint32_t m = lds[N / 2 + (wi >> 1)] >> (16 * (wi & 1));  // (DW is even)
      return sad2(sw, blend2(r, lds[wi], m & 0xFFu, (m >> 8) & 0xFFu), acc);
    } else {
      return acc + obmc2(r, (int)lds[2 * wi], (int)lds[2 * wi + 1], (int)lds[N + 2 * wi],
                         (int)lds[N + 2 * wi + 1]);
    }
  }

  // comp_avg_pred / comp_mask_pred of 4 pixels (dwords r[0], r[1]) at unit u
  // (4 pixels) of row y, invariants from global memory
  __device__ __forceinline__ void pred_mem4(const uint32_t (&r)[2], int y, int u,
                                            uint32_t (&p)[2]) const {
    if constexpr (FORM == kAvg || FORM == kMask) {
      uint32_t t[2];
      load_row<2>(iv.second + 2 * (y * W + 4 * u), t);
      if constexpr (FORM == kAvg) {
        p[0] = avg2(r[0], t[0]);
        p[1] = avg2(r[1], t[1]);
      } else {
        uint32_t m[1];
        load_row<1>(iv.mask + (int64_t)y * iv.ms + 4 * u, m);
        const uint32_t f = fold_mask(m[0], iv.invert);
        p[0] = blend2(r[0], t[0], f & 0xFFu, (f >> 8) & 0xFFu);
        p[1] = blend2(r[1], t[1], (f >> 16) & 0xFFu, f >> 24);
      }
    } else {
      p[0] = r[0];
      p[1] = r[1];
    }
  }
  // the combined SAD of the 4 pixels at unit u of row y, everything but the
  // candidate from global memory
  __device__ __forceinline__ uint32_t unit_mem(const Ctx& c, const uint32_t (&r)[2], int y, int u,
                                               uint32_t acc) const {
    if constexpr (FORM == kObmc) {
      uint32_t w4[4], m4[4];
      load_row<4>(iv.wsrc + 4 * (y * W + 4 * u), w4);
      load_row<4>(iv.omask + 4 * (y * W + 4 * u), m4);
      return acc + obmc2(r[0], (int)w4[0], (int)w4[1], (int)m4[0], (int)m4[1]) +
             obmc2(r[1], (int)w4[2], (int)w4[3], (int)m4[2], (int)m4[3]);
    } else {
      uint32_t sw[2], p[2];
      load_row<2>(c.src + (int64_t)y * c.ss + 8 * u, sw);
      pred_mem4(r, y, u, p);
      return sad2(sw[1], p[1], sad2(sw[0], p[0], acc));
    }
  }

  // the _bitsN SAD of the candidate at mv (r, cc): the group's 8 lanes reduce
  // the block's combined SAD, then the depth's shift; a group whose candidate
  // is not valid reads the block at (sr, sc) instead
  __device__ __forceinline__ uint32_t group_sad(const Ctx& c, int r, int cc, bool valid, int sr,
                                                int sc) const {
    r = valid ? r : sr;
    cc = valid ? cc : sc;
    const uint8_t* base = c.ref + ((int64_t)r * c.rs + 2 * cc);
    uint32_t acc = 0;
    if constexpr (kCache) {
      // every candidate row in flight first, then row by row (the compiler
      // barrier keeps the invariants' LDS reads of one row from being
      // hoisted above the previous row, as in mcomp_comp.hip)
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
          for (int i = 0; i < DW; ++i)
            acc = word_lds(kSrc ? s[kSrc ? k : 0][kSrc ? i : 0] : 0u, rw[k][i], row * DW + i, acc);
        }
      }
    } else {
      constexpr int CH = kChunk<DW>;
      acc = chunk_rows<DW, RPL, 1>(base, c.rs, l,
                                   [&](const uint32_t (&rw)[CH], int y, int x, uint32_t a) {
#pragma unroll
                                     for (int i = 0; i < CH; i += 2) {
                                       const uint32_t r2[2] = {rw[i], rw[i + 1]};
                                       a = unit_mem(c, r2, y, (x + i) >> 1, a);
                                     }
                                     return a;
                                   });
    }
    return group_sum8(acc) >> sh;
  }

  // get_mvpred_compound_var_cost / get_obmc_mvpred_var at (row, col): the
  // whole wave walks the block one 4-pixel unit per lane, everything from
  // global memory (once per run).  A lane sees at most 256 pixels: its sse
  // stays below 2^32 (256 * 4095^2)
  __device__ int var_cost_at(const Ctx& c, int lane, int row, int col) const {
    constexpr int UW = W / 4;
    int sum = 0;
    uint32_t sse = 0;
    const uint8_t* rb = c.ref + ((int64_t)row * c.rs + 2 * col);
    for (int i = lane; i < H * UW; i += 64) {
      const int y = i / UW, u = i - y * UW;
      uint32_t b[2];
      load_row<2>(rb + (int64_t)y * c.rs + 8 * u, b);
      if constexpr (FORM == kObmc) {
        uint32_t w4[4], m4[4];
        load_row<4>(iv.wsrc + 16 * i, w4);
        load_row<4>(iv.omask + 16 * i, m4);
        obmc_acc((int)lo16(b[0]), (int)w4[0], (int)m4[0], sum, sse);
        obmc_acc((int)hi16(b[0]), (int)w4[1], (int)m4[1], sum, sse);
        obmc_acc((int)lo16(b[1]), (int)w4[2], (int)m4[2], sum, sse);
        obmc_acc((int)hi16(b[1]), (int)w4[3], (int)m4[3], sum, sse);
      } else {
        uint32_t a[2], p[2];
        load_row<2>(c.src + (int64_t)y * c.ss + 8 * u, a);
        pred_mem4(b, y, u, p);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // (svaf / msvf take the prediction first: its sum's sign matters
          // to the 10 / 12-bit rounding)
          const int d0 = (int)lo16(p[j]) - (int)lo16(a[j]);
          const int d1 = (int)hi16(p[j]) - (int)hi16(a[j]);
          sum += d0 + d1;
          sse += (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1);
        }
      }
    }
    const int ts = (int)groups_sum(group_sum8((uint32_t)sum));  // |.| <= 2^14 * 4095
    const uint64_t tq = groups_sum64(sse);
    return (int)hbd_var_tail(ts, tq, sh, W * H) + mv_cost(c, row, col);
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

struct KArgs {
  const uint8_t* src;
  const uint8_t* ref;
  const CompJob* jobs;
  const uint8_t* second;
  const uint8_t* mask;
  const uint8_t* wsrc;
  const uint8_t* omask;
  LavishCompSearchResult* out;
  int ss, rs, njobs, sh, what, method, step_param, mask_stride;  // ss / rs: byte strides
};

template <int W, int H, int FORM>
__global__ __launch_bounds__(64 * kDkWaves) void hbd_csearch_kernel(KArgs a, LavishMvCostParams cost) {
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = wg * kDkWaves + wave;
  if (j >= a.njobs) return;
  using SL = Slice<W, H, FORM>;
  __shared__ __attribute__((aligned(16))) uint32_t slice_s[kDkWaves * SL::SIZE];
  const lds_u32 slice = (lds_u32)(slice_s + wave * SL::SIZE);
  CompJob jb = a.jobs[j];
  jb.base.src_off *= 2;  // elements -> bytes
  jb.base.ref_off *= 2;
  // (an OBMC job has no source: its Ctx source is the reference, never read)
  const Ctx c = job_ctx(FORM == kObmc ? a.ref : a.src, a.ss, a.ref, a.rs, jb.base, cost);
  Inv iv;
  iv.second = a.second + 2 * jb.second_off;
  iv.mask = a.mask + jb.mask_off;
  iv.ms = a.mask_stride;
  iv.invert = jb.invert_mask;
  iv.wsrc = a.wsrc + 4 * jb.second_off;
  iv.omask = a.omask + 4 * jb.mask_off;
  HbdCompSearch<W, H, FORM> S;
  S.load(c, lane, a.sh, iv, slice);

  // clamp_fullmv; every run starts here, its cost is read once
  const int srow = min(max((int)jb.base.start_row, c.row_min), c.row_max);
  const int scol = min(max((int)jb.base.start_col, c.col_min), c.col_max);
  const uint32_t c0 = rdlane(S.group_sad(c, srow, scol, true, srow, scol), 0) +
                      mvsad_cost(c, srow, scol);
  int br = srow, bc = scol, steps = 0, sme;
  int sec_r = kInvalidMv, sec_c = kInvalidMv;
  if (a.what == kRefine8) {
    sme = (int)refine<true>(S, c, lane, srow, scol, c0, br, bc, steps);
    sec_r = br;
    sec_c = bc;
  } else if (a.what == kObmcFast) {
    refine<false>(S, c, lane, srow, scol, c0, br, bc, steps);
    sme = S.var_cost_at(c, lane, br, bc);
  } else {
    // full_pixel_diamond / obmc_full_pixel_diamond
    constexpr bool OB = FORM == kObmc;
    int n, num00 = 0;
    diamond_walk<true, OB>(S, c, lane, a.method, srow, scol, c0, a.step_param, br, bc, n, steps,
                           &sec_r, &sec_c);
    sme = S.var_cost_at(c, lane, br, bc);
    const int further = method_steps(a.method) - 1 - a.step_param;
    while (n < further) {
      ++n;
      if (OB && num00) {
        --num00;
        continue;
      }
      int tr, tc;
      diamond_walk<true, OB>(S, c, lane, a.method, srow, scol, c0, a.step_param + n, tr, tc,
                             num00, steps, &sec_r, &sec_c);
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
    a.out[j] = r;
  }
}

template <int W, int H, int FORM>
void launch_comp(const KArgs& a, const LavishMvCostParams& cost, hipStream_t s) {
  const int nwg = xcd_grid((a.njobs + kDkWaves - 1) / kDkWaves);
  hipLaunchKernelGGL((hbd_csearch_kernel<W, H, FORM>), dim3(nwg), dim3(64 * kDkWaves), 0, s, a, cost);
}

bool size_ok(int w, int h) {
#define LAVISH_HC_SIZE(W, H) \
  if (w == W && h == H) return true;
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_HC_SIZE)
#undef LAVISH_HC_SIZE
  return false;
}

// the checks the step-taking entry points share; with the pointer, depth and
// size checks everything is refused before any device work
int comp_args_ok(int method, int step_param, const LavishMvCostParams* cost) {
  if (!diamond_method(method)) return -4;
  if (step_param < 0 || step_param >= method_steps(method)) return -1;
  if (!mv_cost_ok(cost)) return -2;
  return 0;
}

int comp_batch(int w, int h, int form, const KArgs& a, const LavishMvCostParams& cost,
               hipStream_t s) {
#define LAVISH_HC_CASE(W, H)                                          \
  if (w == W && h == H) {                                             \
    if (form == kObmc) launch_comp<W, H, kObmc>(a, cost, s);          \
    else if (form == kMask) launch_comp<W, H, kMask>(a, cost, s);     \
    else if (form == kAvg) launch_comp<W, H, kAvg>(a, cost, s);       \
    else launch_comp<W, H, kPlain>(a, cost, s);                       \
    LAVISH_CHECK(hipGetLastError());                                  \
    return 0;                                                         \
  }
  LAVISH_ENCODER_BLOCK_SIZES(LAVISH_HC_CASE)
#undef LAVISH_HC_CASE
  return -3;
}

KArgs comp_kargs(const uint16_t* src, int ss, const uint16_t* ref, int rs, int bit_depth,
                 const LavishCompSearchJob* jobs, int njobs, int what, int method, int step_param,
                 const uint16_t* second, const uint8_t* mask, int mask_stride,
                 const int32_t* wsrc, const int32_t* omask, LavishCompSearchResult* out) {
  KArgs a = {};
  a.src = (const uint8_t*)src;
  a.ref = (const uint8_t*)ref;
  a.jobs = (const CompJob*)jobs;
  a.second = (const uint8_t*)second;
  a.mask = mask;
  a.wsrc = (const uint8_t*)wsrc;
  a.omask = (const uint8_t*)omask;
  a.out = out;
  a.ss = 2 * ss;
  a.rs = 2 * rs;
  a.njobs = njobs;
  a.sh = bit_depth - 8;
  a.what = what;
  a.method = method;
  a.step_param = step_param;
  a.mask_stride = mask_stride;
  return a;
}

}  // namespace
}  // namespace lavish

using namespace lavish;

extern "C" int lavish_highbd_comp_full_pixel_search_batch(
    const uint16_t* src, int src_stride, const uint16_t* ref, int ref_stride, int w, int h,
    int bit_depth, const LavishCompSearchJob* jobs, int njobs, int search_method, int step_param,
    const LavishMvCostParams* cost, const uint16_t* second_pred, const uint8_t* mask,
    int mask_stride, LavishCompSearchResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = comp_args_ok(search_method, step_param, cost)) return rc;
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      second_pred == nullptr || (mask != nullptr && mask_stride < w) || !bd_ok(bit_depth, 1))
    return -7;
  if (!size_ok(w, h)) return -3;
  const KArgs a = comp_kargs(src, src_stride, ref, ref_stride, bit_depth, jobs, njobs, kFullpel,
                             search_method, step_param, second_pred, mask, mask_stride, nullptr,
                             nullptr, out);
  return comp_batch(w, h, mask ? kMask : kAvg, a, *cost, (hipStream_t)stream);
}

extern "C" int lavish_highbd_refining_search_8p_batch(
    const uint16_t* src, int src_stride, const uint16_t* ref, int ref_stride, int w, int h,
    int bit_depth, const LavishCompSearchJob* jobs, int njobs, const LavishMvCostParams* cost,
    const uint16_t* second_pred, const uint8_t* mask, int mask_stride,
    LavishCompSearchResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (!mv_cost_ok(cost)) return -2;
  // (a mask without second_pred has nothing to blend with)
  if (src == nullptr || ref == nullptr || jobs == nullptr || out == nullptr ||
      (mask != nullptr && (second_pred == nullptr || mask_stride < w)) || !bd_ok(bit_depth, 1))
    return -7;
  if (!size_ok(w, h)) return -3;
  const KArgs a = comp_kargs(src, src_stride, ref, ref_stride, bit_depth, jobs, njobs, kRefine8,
                             kDiamond, 0, second_pred, mask, mask_stride, nullptr, nullptr, out);
  return comp_batch(w, h, mask ? kMask : second_pred ? kAvg : kPlain, a, *cost,
                    (hipStream_t)stream);
}

extern "C" int lavish_highbd_obmc_full_pixel_search_batch(
    const uint16_t* ref, int ref_stride, int w, int h, int bit_depth,
    const LavishCompSearchJob* jobs, int njobs, int search_method, int step_param,
    const LavishMvCostParams* cost, int fast_obmc_search, const int32_t* wsrc,
    const int32_t* obmc_mask, LavishCompSearchResult* out, void* stream) {
  if (njobs <= 0) return 0;
  if (const int rc = comp_args_ok(search_method, step_param, cost)) return rc;
  if (ref == nullptr || jobs == nullptr || out == nullptr || wsrc == nullptr ||
      obmc_mask == nullptr || !bd_ok(bit_depth, 1))
    return -7;
  if (!size_ok(w, h)) return -3;
  const KArgs a = comp_kargs(nullptr, ref_stride, ref, ref_stride, bit_depth, jobs, njobs,
                             fast_obmc_search ? kObmcFast : kFullpel, search_method, step_param,
                             nullptr, nullptr, 0, wsrc, obmc_mask, out);
  return comp_batch(w, h, kObmc, a, *cost, (hipStream_t)stream);
}
