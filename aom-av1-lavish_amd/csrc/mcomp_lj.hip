// mcomp_lj.hip -- the lane-job family of the full-pixel search (C3): DIAMOND
// (full_pixel_diamond / diamond_search_sad, av1/encoder/mcomp.c:1318-1526,
// with the quality recheck :1840-1867) over 16x16 blocks and tiled
// references with eight jobs per wave, its capped and queue-fed launches, the
// 64-VGPR lean variant that runs beside C2 (diamond_lj_lean_kernel and its
// redo launch), the fused C2 + C3 launch (lavish_txq_frame_search; the only
// unit that includes txq_dev.h) and the tiled reference copy
// (lavish_ref_tiles_build).
#include <atomic>

#include "mcomp_dev.h"
#include "txq_dev.h"

namespace lavish {
namespace {

// DIAMOND, 16x16 blocks, tiled references: eight jobs per wave.
//
// The one-job-per-wave kernel spends ~70 VALU + ~60 SALU instructions per
// 8-site step on one job: its time goes to instruction issue and to the
// per-step dependency chain, not to memory (halving its address-path work
// with the tiled layout changed nothing, profiles/r03_*).  Here lane
// (j = lane >> 3, l = lane & 7) works for job j of eight: a step evaluates
// the job's 8 sites one after the other, lane l reading row 2l (downsampled
// SAD; rows l and l + 8 otherwise) of each candidate from the tiled copy, so
// one load instruction covers one site of all eight jobs (8 x 256 contiguous
// bytes) and one step's bookkeeping serves eight jobs.  Each job carries its
// own walk in the lanes of its group (row, col, radius, search index, num00
// state): jobs at different radii / searches step together, branch-free.
// full_pixel_diamond's var costs do not steer the search sequence (n and
// num00 come from the walks alone), so each search's result is recorded and
// the var costs are evaluated once the job's walks are done, in the
// reference's order with its strict "sme < bestsme".  Then the cost list,
// the downsampled-SAD quality check (mcomp.c:1840-1867) and, for the jobs it
// fails, a second pass with full-row SADs.  Bit-exact with diamond_kernel.
constexpr int kLjJobs = 8;  // jobs per wave
constexpr int kMvDecHalf = 2047;          // MV_MAX / 8: full-pel reach of the cost tables
constexpr int kMvDecN = 2 * kMvDecHalf + 1;

__device__ __forceinline__ uint32_t group_min8(uint32_t v) {  // min over the 8-lane group
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));
  return v;
}

// source rows of lane l: sk = row 2l (downsampled SAD), fr[k] = row l + 8k
struct LjSrc {
  uint32_t sk[4], fr[2][4];
};

// group SAD of the job's candidate at (r, cc) (in range), from the tiles
template <bool SKIP>
__device__ __forceinline__ uint32_t lj_sad(const Ctx& c, const LjSrc& s, int l, int r, int cc) {
  const int x = c.ox + cc;
  uint32_t acc = 0;
  if constexpr (SKIP) {
    uint32_t t[4];
    load_row<4>(c.tiles + tile_off(c, c.oy + r + 2 * l, x), t);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = sad4(s.sk[i], t[i], acc);
  } else {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      uint32_t t[4];
      load_row<4>(c.tiles + tile_off(c, c.oy + r + l + 8 * k, x), t);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = sad4(s.fr[k][i], t[i], acc);
    }
  }
  acc = group_sum8(acc);
  return SKIP ? 2 * acc : acc;
}

// aom_variance16x16 + mv_err_cost at (r, cc), the linear reference; lane l
// takes rows l and l + 8
__device__ __forceinline__ int lj_var(const Ctx& c, const LjSrc& s, int l, int r, int cc) {
  int sum = 0;
  uint32_t sse = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    uint32_t t[4];
    load_row<4>(c.ref + (int64_t)(r + l + 8 * k) * c.rs + cc, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) var_acc(s.fr[k][i], t[i], sum, sse);
  }
  const uint32_t ts = group_sum8((uint32_t)sum), tq = group_sum8(sse);
  const uint32_t var = tq - (uint32_t)(((int64_t)(int)ts * (int)ts) / 256);
  return (int)var + mv_cost(c, r, cc);
}

// N candidates' group SADs with every load in flight before the first SAD:
// (r[i], cc[i]) in range where v[i]; an invalid candidate's rows are read at
// an offset past the tiled buffer's end, which the buffer descriptor's range
// check drops (no memory request, the value 0; its SAD is masked by the
// caller).  Loads through a branch per candidate were serialised by the
// compiler, one memory round trip per candidate (profiles/r04_c3_isa_*).
template <bool SKIP, int N>
__device__ __forceinline__ void lj_sads(const Ctx& c, const LjSrc& s, int l,
                                        __amdgpu_buffer_rsrc_t trs, int oob, const int (&r)[N],
                                        const int (&cc)[N], const bool (&v)[N],
                                        uint32_t (&out)[N]) {
  constexpr int RW = SKIP ? 1 : 2;  // rows per lane
  u32x4 t[N][RW];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      const int y = c.oy + r[i] + (SKIP ? 2 * l : l + 8 * k);
      t[i][k] = __builtin_amdgcn_raw_buffer_load_b128(
          trs, v[i] ? (int)tile_off(c, y, c.ox + cc[i]) : oob, 0, 0);
    }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      const uint32_t* q = SKIP ? s.sk : s.fr[k];
      acc = sad4(q[0], t[i][k].x, acc);
      acc = sad4(q[1], t[i][k].y, acc);
      acc = sad4(q[2], t[i][k].z, acc);
      acc = sad4(q[3], t[i][k].w, acc);
    }
    acc = group_sum8(acc);
    out[i] = SKIP ? 2 * acc : acc;
  }
}

// The 8 candidates' group SADs of a diamond step, lane l of each 8-lane
// group keeping the one of site l: a reduce-scatter over the group instead
// of 8 full group sums and a select.  Stage 1 pairs lane l with its mirror
// 7 - l (row_half_mirror): the lane keeps the half of the sites it will end
// with (0-3 below lane 4, 4-7 above), adds its partner's partial sums of
// that half and hands over the other; stages 2 and 3 do the same with lane
// l ^ 2 and l ^ 1 (quad_perm), so lane l ends with site 4 b2 + 2 b1 + b0 =
// l summed over all 8 lanes: 21 DPP adds / selects per step instead of 24
// DPP adds + 8 selects.  The same sums as group_sum8 (integer adds).
__device__ __forceinline__ uint32_t scatter_sum8(const uint32_t (&p)[8], int l) {
  const bool hi = l & 4, m1 = l & 2, m0 = l & 1;
  uint32_t q[4], r[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t send = hi ? p[k] : p[k + 4];
    const uint32_t keep = hi ? p[k + 4] : p[k];
    q[k] = keep + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send, 0x141, 0xF, 0xF, false);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t send = m1 ? q[k] : q[k + 2];
    const uint32_t keep = m1 ? q[k + 2] : q[k];
    r[k] = keep + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send, 0x4E, 0xF, 0xF, false);
  }
  const uint32_t send = m0 ? r[0] : r[1];
  const uint32_t keep = m0 ? r[1] : r[0];
  return keep + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send, 0xB1, 0xF, 0xF, false);
}

// the 8-site step (downsampled rows) at offsets into the tiled copy computed
// by the caller, lane l reading row 2l of each candidate: lane l gets site
// l's group SAD
__device__ __forceinline__ uint32_t lj_step_sad(const LjSrc& s, __amdgpu_buffer_rsrc_t trs,
                                                int oob, const uint32_t (&off)[8],
                                                const bool (&v)[8], int l) {
  u32x4 t[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    t[i] = __builtin_amdgcn_raw_buffer_load_b128(trs, v[i] ? (int)off[i] : oob, 0, 0);
  uint32_t p[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t acc = sad4(s.sk[0], t[i].x, 0);
    acc = sad4(s.sk[1], t[i].y, acc);
    acc = sad4(s.sk[2], t[i].z, acc);
    p[i] = sad4(s.sk[3], t[i].w, acc);
  }
  return 2 * scatter_sum8(p, l);
}

// mvsad_err_cost's table reads for the entropy cost through the decimated
// copy of the caller's row / column tables (dec[0..4094] = mvcost0[8 k],
// dec[4095..] = mvcost1[8 k], k = -2047 .. 2047, built per call by
// mvcost_dec_kernel): a full-pel search only ever indexes multiples of 8,
// so the copy is contiguous in what a step reads (a job's 8 sites differ by
// +-rad full pels) and the site costs of a step share cache lines.
__device__ __forceinline__ MvRate mvsad_rate_dec(const Ctx& c, const int32_t* dec, int row,
                                                 int col) {
  if (dec == nullptr) return mvsad_rate(c, row, col);
  const int kr = row - c.full_ref_row, kc = col - c.full_ref_col;
  const int joint = (kc != 0) | ((kr != 0) << 1);  // av1_get_mv_joint
  typedef const __attribute__((address_space(1))) int32_t* gi32;
  return MvRate{((gi32)c.mvjcost)[joint], ((gi32)dec)[kr + kMvDecHalf],
                ((gi32)dec)[kc + kMvDecHalf + kMvDecN]};
}

// one pass of full_pixel_diamond (+ its cost list) for the wave's jobs whose
// `run` is set; accumulates steps / searches, leaves the pass's best mv, var
// cost and cost list
template <bool SKIP>
__device__ void lj_pass(const Ctx& c, const LjSrc& s, int l, __amdgpu_buffer_rsrc_t trs, int oob,
                        const int32_t* dec, bool run, int step_param, bool want_cl,
                        uint32_t* res, int& steps,
                        int& searches, int& br, int& bc, int& sme, int (&cl)[5]) {
  // (br / bc carry the start mv on entry; diamond_search_sad clamps it)
  const int srow = min(max(br, c.row_min), c.row_max);
  const int scol = min(max(bc, c.col_min), c.col_max);
  const int sdr = site_dr(l), sdc = site_dc(l);
  // the start: its SAD once per pass (every run restarts there)
  uint32_t c0;
  {
    const int r1[1] = {srow}, c1[1] = {scol};
    const bool v1[1] = {true};
    uint32_t o1[1];
    lj_sads<SKIP, 1>(c, s, l, trs, oob, r1, c1, v1, o1);
    c0 = o1[0] + mvsad_finish(c, mvsad_rate_dec(c, dec, srow, scol), srow, scol);
  }
  const int further = kMaxSteps - 1 - step_param;
  bool active = run;
  bool first = true;
  int n = 0, row = srow, col = scol, stp = kMaxSteps - step_param - 1, center = 0, nres = 0;
  bool offc = false;
  uint32_t best = c0;
  while (__builtin_amdgcn_ballot_w64(active) != 0) {
    const int rad = 1 << stp;
    // lane l: site l's cost (its loads in flight with the SAD loads below)
    const int rl = row + sdr * rad, cl_ = col + sdc * rad;
    const bool vl = cl_ >= c.col_min && cl_ <= c.col_max && rl >= c.row_min && rl <= c.row_max;
    // loads only for in-range sites of jobs still walking: out-of-range
    // sites (most of the large radii) and finished jobs issue no memory
    // requests (the range-checked offset); a job's 8 lanes share both
    // conditions, so each group's DPP sum stays whole
    MvRate mr = {0, 0, 0};
    if (vl && active) mr = mvsad_rate_dec(c, dec, rl, cl_);
    uint32_t mine = 0;
    // the 8 sites: all loads issued, then the SADs (SKIP: 8 x 1 row per
    // lane; full rows: two halves of 4 sites x 2 rows)
    constexpr int NS = SKIP ? 8 : 4;
    if constexpr (SKIP) {
      // the sites' tile offsets and range checks from per-step parts: the
      // walk's position is in range, so a site is valid iff its row and
      // column moves stay inside; with an even radius the site rows keep
      // the field of row y and move its row half linearly (rad / 2 strip
      // rows), so an offset is one add of a row part (3 per step) and a
      // column part (3 per step) instead of a tile_off per site
      const bool up = row - rad >= c.row_min, dn = row + rad <= c.row_max;
      const bool lf = col - rad >= c.col_min, rt = col + rad <= c.col_max;
      const int y0 = c.oy + row + 2 * l, x0 = c.ox + col;
      uint32_t off[8];
      bool vv[8];
      if (stp > 0) {
        const int yb = (y0 & 1) * c.fsz + ((y0 >> 1) << 5), d16 = rad << 4;
        const int f32 = c.fh << 5;
        auto xo = [&](int x) { return __mul24(x >> 4, f32) + (x & 15); };
        const int xm = xo(x0 - rad), xc = xo(x0), xp = xo(x0 + rad);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int dr = site_dr(t), dc = site_dc(t);
          off[t] = (uint32_t)((dr < 0 ? yb - d16 : dr > 0 ? yb + d16 : yb) +
                              (dc < 0 ? xm : dc > 0 ? xp : xc));
        }
      } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) off[t] = tile_off(c, y0 + site_dr(t), x0 + site_dc(t));
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int dr = site_dr(t), dc = site_dc(t);
        vv[t] = active && (dr < 0 ? up : dr > 0 ? dn : true) && (dc < 0 ? lf : dc > 0 ? rt : true);
      }
      if (active) mine = lj_step_sad(s, trs, oob, off, vv, l);
    } else
    if (active)  // finished jobs' lanes off for the whole step (one branch; measured neutral, r04_v6)
#pragma unroll
    for (int h = 0; h < 8 / NS; ++h) {
      int rr[NS], cc[NS];
      bool vv[NS];
      uint32_t sd[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int t = h * NS + i;
        rr[i] = row + site_dr(t) * rad;
        cc[i] = col + site_dc(t) * rad;
        vv[i] = active && cc[i] >= c.col_min && cc[i] <= c.col_max && rr[i] >= c.row_min &&
                rr[i] <= c.row_max;
      }
      lj_sads<SKIP, NS>(c, s, l, trs, oob, rr, cc, vv, sd);
#pragma unroll
      for (int i = 0; i < NS; ++i) mine = l == h * NS + i ? sd[i] : mine;
    }
    const uint32_t key =
        (((mine + mvsad_finish(c, mr, rl, cl_)) << 3) | (uint32_t)l) | (vl ? 0u : ~0u);
    const uint32_t kmin = group_min8(key);
    if (active) {
      ++steps;
      if (kmin < (best << 3)) {
        best = kmin >> 3;
        const int i = (int)(kmin & 7);
        row += site_dr(i) * rad;
        col += site_dc(i) * rad;
        offc = true;
      }
      if (!offc) ++center;
      if (--stp < 0) {  // this diamond_search_sad run is over
        if (l == 0) res[nres] = ((uint32_t)(uint16_t)row << 16) | (uint16_t)col;
        ++nres;
        ++searches;
        if (first) n = center;       // the first run's num00
        else if (center) n += center;
        first = false;
        if (n < further) {           // the next run, one step shorter
          ++n;
          row = srow;
          col = scol;
          best = c0;
          stp = kMaxSteps - (step_param + n) - 1;
          center = 0;
          offc = false;
        } else {
          active = false;
          stp = 0;  // a finished job keeps stepping in place at radius 1 (masked)
        }
      }
    }
  }
  wave_sync();
  if (!run) return;
  // var costs of the runs' results in order, strict "<" (full_pixel_diamond)
  for (int i = 0; i < nres; ++i) {
    const uint32_t p = res[i];
    const int r = (int16_t)(p >> 16), cc = (int16_t)(p & 0xFFFF);
    const int v = lj_var(c, s, l, r, cc);
    if (i == 0 || v < sme) {
      sme = v;
      br = r;
      bc = cc;
    }
  }
  if (want_cl) {  // calc_int_sad_list around (br, bc): centre, left, bottom, right, top
    int rr[5], cc[5];
    bool vv[5];
    uint32_t sd[5];
    MvRate m[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      rr[t] = br + (t == 2 ? 1 : t == 4 ? -1 : 0);
      cc[t] = bc + (t == 1 ? -1 : t == 3 ? 1 : 0);
      vv[t] = t == 0 ||
              (cc[t] >= c.col_min && cc[t] <= c.col_max && rr[t] >= c.row_min && rr[t] <= c.row_max);
      m[t] = mvsad_rate_dec(c, dec, vv[t] ? rr[t] : br, vv[t] ? cc[t] : bc);  // (in-range indices)
    }
    lj_sads<SKIP, 5>(c, s, l, trs, oob, rr, cc, vv, sd);
#pragma unroll
    for (int t = 0; t < 5; ++t)
      cl[t] = vv[t] ? (int)(sd[t] + mvsad_finish(c, m[t], rr[t], cc[t])) : INT_MAX;
  }
}

template <bool LIST = false>
__device__ __forceinline__ void lj_jobs(
    const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs,
    const LavishRefTiles& tiles, const Job* __restrict__ jobs, int njobs, int step_param,
    const LavishMvCostParams& cost, const int32_t* dec, int skip,
    LavishDiamondResult* __restrict__ out, int32_t* __restrict__ cost_lists, int j0,
    uint32_t* res, const int* __restrict__ list = nullptr, int nlist = 0);

// one group of WPG x 8 jobs: virtual workgroup vwg of nvwg (a multiple of 8)
template <int WPG>
__device__ __forceinline__ void lj_group(
    const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs,
    const LavishRefTiles& tiles, const Job* __restrict__ jobs, int njobs, int step_param,
    const LavishMvCostParams& cost, const int32_t* dec, int skip,
    LavishDiamondResult* __restrict__ out, int32_t* __restrict__ cost_lists, int vwg, int nvwg) {
  __shared__ uint32_t res_s[WPG][kLjJobs][kMaxSteps];  // (LDS-addressed, not through a pointer)
  const int wg = xcd_remap(vwg, nvwg);
  const int lane = threadIdx.x & 63;
  const int wave = WPG == 1 ? 0 : threadIdx.x >> 6;
  const int j0 = (wg * WPG + wave) * kLjJobs;
  if (j0 >= njobs) return;
  lj_jobs(src, ss, ref, rs, tiles, jobs, njobs, step_param, cost, dec, skip, out, cost_lists, j0,
          res_s[wave][lane >> 3]);
}

// the eight jobs j0 .. j0 + 7 of one wave (res: this lane group's LDS slot
// for the runs' results); LIST: the jobs list[j0 .. j0 + 7] of a list of
// nlist job indices (the lean search's redo list)
template <bool LIST>
__device__ __forceinline__ void lj_jobs(
    const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs,
    const LavishRefTiles& tiles, const Job* __restrict__ jobs, int njobs, int step_param,
    const LavishMvCostParams& cost, const int32_t* dec, int skip,
    LavishDiamondResult* __restrict__ out, int32_t* __restrict__ cost_lists, int j0,
    uint32_t* res, const int* __restrict__ list, int nlist) {
  const int lane = threadIdx.x & 63;
  const int jg = lane >> 3, l = lane & 7;
  const int cnt = LIST ? nlist : njobs;
  const int jj = min(j0 + jg, cnt - 1);  // a surplus group repeats the last job, never stores
  const int j = LIST ? list[jj] : jj;
  const bool mine_job = j0 + jg < cnt;
  const Job jb = jobs[j];
  Ctx c;
  c.src = src + jb.src_off;
  c.ref = ref + jb.ref_off;
  c.ss = ss;
  c.rs = rs;
  c.col_min = jb.col_min;
  c.col_max = jb.col_max;
  c.row_min = jb.row_min;
  c.row_max = jb.row_max;
  c.ref_mv_row = jb.ref_mv_row;
  c.ref_mv_col = jb.ref_mv_col;
  c.full_ref_row = rawpel(jb.ref_mv_row);
  c.full_ref_col = rawpel(jb.ref_mv_col);
  c.cost_type = cost.mv_cost_type;
  c.sad_lambda = sad_lambda(cost.mv_cost_type);
  c.sse_lambda = sse_lambda(cost.mv_cost_type);
  c.sad_per_bit = cost.sad_per_bit;
  c.error_per_bit = cost.error_per_bit;
  const bool ent = cost.mv_cost_type == 0;
  c.mvjcost = ent ? cost.mvjcost : kZeroRate;
  c.mvcost0 = ent ? cost.mvcost[0] : kZeroRate;
  c.mvcost1 = ent ? cost.mvcost[1] : kZeroRate;
  c.tiles = tiles.data;
  c.fh = tiles.field_rows;
  c.fsz = (int)tiles.field_bytes;
  c.oy = (int)(jb.ref_off / rs);
  c.ox = (int)(jb.ref_off - (int64_t)c.oy * rs);
  // the tiled copy through a range-checked buffer descriptor (uniform:
  // kernel arguments only); `oob` = an offset past its end
  const int oob = (int)(2 * tiles.field_bytes);
  const __amdgpu_buffer_rsrc_t trs =
      __builtin_amdgcn_make_buffer_rsrc((void*)tiles.data, 0, oob, 0x00020000);
  LjSrc s;
  load_row<4>(c.src + (int64_t)(2 * l) * ss, s.sk);
  load_row<4>(c.src + (int64_t)l * ss, s.fr[0]);
  load_row<4>(c.src + (int64_t)(l + 8) * ss, s.fr[1]);
  const bool want_cl = cost_lists != nullptr;
  int cl[5] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  int steps = 0, searches = 0, sme = 0;
  int br = jb.start_row, bc = jb.start_col;
  bool full = true;
  if (skip) {
    lj_pass<true>(c, s, l, trs, oob, dec, true, step_param, want_cl, res, steps, searches, br, bc,
                  sme, cl);
    // quality check of the row-skipping search (mcomp.c:1840-1867): sad and
    // sad_skip at the result, rows l and l + 8 of lane l (same parity as l)
    uint32_t all = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      uint32_t t[4];
      load_row<4>(c.ref + (int64_t)(br + l + 8 * k) * rs + bc, t);
#pragma unroll
      for (int i = 0; i < 4; ++i) all = sad4(s.fr[k][i], t[i], all);
    }
    const int sad = (int)group_sum8(all);
    const int ssad = (int)(2 * group_sum8((l & 1) ? 0u : all));
    full = sad > 16 && abs(ssad - sad) * 10 >= max(sad, 1) * 9;
    if (full) {
      br = jb.start_row;
      bc = jb.start_col;
    }
  }
  if (__builtin_amdgcn_ballot_w64(full) != 0)
    lj_pass<false>(c, s, l, trs, oob, dec, full, step_param, want_cl, res, steps, searches, br, bc,
                   sme, cl);
  if (!mine_job) return;
  if (l == 0) {
    LavishDiamondResult r;
    r.best_row = (int16_t)br;
    r.best_col = (int16_t)bc;
    r.bestsme = sme;
    r.steps = steps;
    r.searches = searches;
    out[j] = r;
  }
  if (want_cl && l < 5) {
    const int v = l == 0 ? cl[0] : l == 1 ? cl[1] : l == 2 ? cl[2] : l == 3 ? cl[3] : cl[4];
    cost_lists[5 * (int64_t)j + l] = v;
  }
}

// nvwg virtual workgroups over gridDim.x (<= nvwg, both multiples of 8, so a
// virtual workgroup runs on the XCD of its first): with a smaller grid the
// search holds fewer CU slots while a concurrent leg runs beside it
// WPG waves per workgroup.  1 would let the dispatcher refill a SIMD slot as
// soon as one wave's eight jobs are done; measured, four-wave workgroups are
// faster (0.294 vs 0.303 ms, profiles/r04_v5_c3_wpg_ab.txt): the four waves
// of a workgroup are consecutive job groups on one CU, sharing its L1
#ifndef LAVISH_LJ_WAVES
#define LAVISH_LJ_WAVES 4  // minimum waves per SIMD requested (VGPR budget 512 / this)
#endif
template <int WPG>
__global__ __launch_bounds__(64 * WPG, LAVISH_LJ_WAVES) void diamond_lj_kernel(
    const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs,
    LavishRefTiles tiles, const Job* __restrict__ jobs, int njobs, int step_param,
    LavishMvCostParams cost, const int32_t* dec, int skip, LavishDiamondResult* __restrict__ out,
    int32_t* __restrict__ cost_lists, int nvwg) {
  for (int v = blockIdx.x; v < nvwg; v += gridDim.x)
    lj_group<WPG>(src, ss, ref, rs, tiles, jobs, njobs, step_param, cost, dec, skip, out,
                  cost_lists, v, nvwg);
}

// The capped grid with work pulled from queues: beside C2 the search runs in
// `cap` workgroups (lavish_set_search_workgroup_cap) that each process many
// 8-job wave units.  Dealt statically (grid-stride over virtual workgroups),
// ceil(groups / cap) rounds set the leg's length while most workgroups sit
// idle in the last round (1760 groups over 512 workgroups: 223 do 4, 289 do
// 3) and every wave of a workgroup waits for its slowest unit.  Here every
// wave pulls its next unit from a queue with one returning atomic: the
// units of XCD label x = blockIdx % 8 (blocks b and b + 8 share an XCD, so
// neighbouring blocks' reference tiles stay in one L2, as with the static
// mapping) are the contiguous range [units x / 8, units (x + 1) / 8); a
// label's workgroups drain it together.  queue: 8 counters 16 ints apart,
// zero at launch (mvcost_dec_kernel or lj_queue_zero clears them on the
// same stream).  The order of the units changes no result.
constexpr int kLjQueueStride = 16;  // ints between two labels' counters (64 B)

template <int WPG>
__global__ __launch_bounds__(64 * WPG, LAVISH_LJ_WAVES) void diamond_lj_dyn_kernel(
    const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs,
    LavishRefTiles tiles, const Job* __restrict__ jobs, int njobs, int step_param,
    LavishMvCostParams cost, const int32_t* dec, int skip, LavishDiamondResult* __restrict__ out,
    int32_t* __restrict__ cost_lists, int* __restrict__ queue) {
  __shared__ uint32_t res_s[WPG][kLjJobs][kMaxSteps];
  const int units = (njobs + kLjJobs - 1) / kLjJobs;
  const int x = blockIdx.x & 7;
  const int u0 = units * x / 8, u1 = units * (x + 1) / 8;
  const int lane = threadIdx.x & 63;
  const int wave = WPG == 1 ? 0 : threadIdx.x >> 6;
  uint32_t* res = res_s[wave][lane >> 3];
  int* q = queue + x * kLjQueueStride;
  for (;;) {
    int t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = __builtin_amdgcn_readfirstlane(t);
    if (u0 + t >= u1) break;  // every wave of the label ends here once the range is drained
    lj_jobs(src, ss, ref, rs, tiles, jobs, njobs, step_param, cost, dec, skip, out, cost_lists,
            (u0 + t) * kLjJobs, res);
  }
}

// the queue block: the 8 labels' counters, then the lean search's redo
// counter; the redo list (job indices) follows the block
constexpr int kLjQueueInts = 9 * kLjQueueStride;

__global__ void lj_queue_zero(int* __restrict__ queue) {
  if (threadIdx.x < kLjQueueInts) queue[threadIdx.x] = 0;
}

// ---------------------------------------------------------------------------
// The lean variant of the queue-fed search: the same walk in at most 64 VGPRs
// and under 3 KB of LDS per workgroup, so a search wave finds a slot on a
// SIMD whose four transform (C2) workgroups hold 448 of its 512 VGPRs.
//  - Only the row-skipping pass and its quality check run here.  A job that
//    fails the check is appended to a redo list (a device counter + job
//    indices behind the queue's counters) and diamond_lj_redo_kernel, the
//    next launch on the stream, reruns it from its start with the full body
//    (lj_jobs<true>, skip = 1): the accumulated steps / searches, the record
//    and the cost list are diamond_lj_dyn_kernel's.
//  - Per-job constants (the mv window, the reference mv, the block's origin
//    in the tiled copy, the clamped start and its cost, the source offset)
//    sit in a 10-word LDS record per lane group, written once per unit and
//    read where used; launch-uniform values stay scalar.
//  - Only source row 2l (sk) is live during the walk; rows l and l + 8 are
//    reloaded for the variance costs and the quality check.
//  - A step's 8 candidate loads go in two halves of 4; every offset is a row
//    part + a column part (tile_off splits that way at any radius).
//  - The variance costs of a job's runs are evaluated kVarBatch at a time,
//    their loads in flight together, as byte dot products.
// The compiler's register count after each of these: DESIGN.md section 4.
constexpr int kLjRecWords = 10;
constexpr int kVarBatch = 2;  // results' variance costs in flight together
enum {
  kRecRows = 0,   // row_min | row_max << 16
  kRecCols = 1,   // col_min | col_max << 16
  kRecFref = 2,   // full_ref_row | full_ref_col << 16
  kRecRefMv = 3,  // ref_mv_row | ref_mv_col << 16
  kRecOy = 4,
  kRecOx = 5,
  kRecStart = 6,  // the clamped start: row | col << 16
  kRecC0 = 7,     // its cost
  kRecSrc = 8     // src_off (2 words)
};
__device__ __forceinline__ int lo16(uint32_t v) { return (int)(int16_t)(v & 0xFFFF); }
__device__ __forceinline__ int hi16(uint32_t v) { return (int)v >> 16; }
__device__ __forceinline__ uint32_t pack16(int lo, int hi) {
  return ((uint32_t)hi << 16) | (uint32_t)(uint16_t)lo;
}
__device__ __forceinline__ int64_t rec_i64(lds_u32 rec, int at) {
  return (int64_t)(((uint64_t)rec[at + 1] << 32) | rec[at]);
}

// mvsad_rate_dec's loads at unsigned indices (in range by the same contract):
// a scalar table base + a 32-bit lane offset, no 64-bit lane address; no
// decimated tables (dec null: not the entropy cost) = no loads, the rates
// are not used
__device__ __forceinline__ MvRate lean_rate(const int32_t* mvjcost, const int32_t* dec, int kr,
                                            int kc) {
  const uint32_t joint = (uint32_t)((kc != 0) | ((kr != 0) << 1));  // av1_get_mv_joint
  typedef const __attribute__((address_space(1))) int32_t* gi32;
  return MvRate{((gi32)mvjcost)[joint], ((gi32)dec)[(uint32_t)(kr + kMvDecHalf)],
                ((gi32)dec)[(uint32_t)(kc + kMvDecHalf + kMvDecN)]};
}
// a lane value the compiler may not carry across this point: what depends on
// it is computed where it is used (carried, the per-lane row offsets, site
// moves and lane masks hold registers for the whole kernel)
__device__ __forceinline__ int lane_fresh(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// u: the launch-uniform fields of Ctx (the per-job fields are filled from the
// record where a helper needs them)
__device__ __forceinline__ void lj_lean_jobs(
    const Ctx& u, const uint8_t* __restrict__ src, const uint8_t* __restrict__ ref,
    __amdgpu_buffer_rsrc_t trs, int oob, const Job* __restrict__ jobs, int njobs, int step_param,
    const int32_t* dec, LavishDiamondResult* __restrict__ out, int32_t* __restrict__ cost_lists,
    int j0, lds_u32 res_s, lds_u32 rec_s, int* __restrict__ redo) {
  // this lane group's slot for the runs' results and its record
  const int tid = lane_fresh((int)threadIdx.x);
  const lds_u32 res = res_s + (tid >> 3) * kMaxSteps, rec = rec_s + (tid >> 3) * kLjRecWords;
  const int jg = (tid & 63) >> 3;
  int l = tid & 7;
  const int j = min(j0 + jg, njobs - 1);  // a surplus group repeats the last job, never stores
  uint32_t sk[4];
  {
    const Job jb = jobs[j];
    const int oy = (int)(jb.ref_off / u.rs), ox = (int)(jb.ref_off - (int64_t)oy * u.rs);
    const int srow = min(max((int)jb.start_row, (int)jb.row_min), (int)jb.row_max);
    const int scol = min(max((int)jb.start_col, (int)jb.col_min), (int)jb.col_max);
    Ctx c = u;
    c.full_ref_row = rawpel(jb.ref_mv_row);
    c.full_ref_col = rawpel(jb.ref_mv_col);
    c.oy = oy;
    c.ox = ox;
    load_row<4>(src + jb.src_off + (int64_t)(2 * l) * u.ss, sk);
    // the start: its SAD once per job (every run restarts there)
    MvRate m0 = {0, 0, 0};
    if (dec != nullptr)
      m0 = lean_rate(u.mvjcost, dec, srow - c.full_ref_row, scol - c.full_ref_col);
    const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(
        trs, (int)tile_off(c, oy + srow + 2 * l, ox + scol), 0, 0);
    uint32_t acc = sad4(sk[0], t.x, 0);
    acc = sad4(sk[1], t.y, acc);
    acc = sad4(sk[2], t.z, acc);
    acc = sad4(sk[3], t.w, acc);
    const uint32_t c0 = 2 * group_sum8(acc) + mvsad_finish(c, m0, srow, scol);
    if (l == 0) {
      rec[kRecRows] = pack16(jb.row_min, jb.row_max);
      rec[kRecCols] = pack16(jb.col_min, jb.col_max);
      rec[kRecFref] = pack16(c.full_ref_row, c.full_ref_col);
      rec[kRecRefMv] = pack16(jb.ref_mv_row, jb.ref_mv_col);
      rec[kRecOy] = (uint32_t)oy;
      rec[kRecOx] = (uint32_t)ox;
      rec[kRecStart] = pack16(srow, scol);
      rec[kRecC0] = c0;
      rec[kRecSrc] = (uint32_t)jb.src_off;
      rec[kRecSrc + 1] = (uint32_t)((uint64_t)jb.src_off >> 32);
    }
  }
  wave_sync();
  const int further = kMaxSteps - 1 - step_param;
  bool active = true, first = true, offc = false;
  int n = 0, stp = kMaxSteps - step_param - 1, center = 0, nres = 0, steps = 0;
  int row = lo16(rec[kRecStart]), col = hi16(rec[kRecStart]);
  uint32_t best = rec[kRecC0];
  while (__builtin_amdgcn_ballot_w64(active) != 0) {
    // (the record's reads stay inside the loop: hoisted, they are the
    // per-job registers again)
    asm volatile("" ::: "memory");
    const int rad = 1 << stp;
    const uint32_t wr = rec[kRecRows], wc = rec[kRecCols], wf = rec[kRecFref];
    const int row_min = lo16(wr), row_max = hi16(wr), col_min = lo16(wc), col_max = hi16(wc);
    Ctx c = u;
    c.full_ref_row = lo16(wf);
    c.full_ref_col = hi16(wf);
    // lane l: site l's cost (its loads in flight with the SAD loads below)
    const int rl = row + site_dr(l) * rad, cl_ = col + site_dc(l) * rad;
    const bool vl = cl_ >= col_min && cl_ <= col_max && rl >= row_min && rl <= row_max;
    MvRate mr = {0, 0, 0};
    if (dec != nullptr && vl && active)
      mr = lean_rate(u.mvjcost, dec, rl - c.full_ref_row, cl_ - c.full_ref_col);
    uint32_t mine = 0;
    if (active) {
      // the walk's position is in range, so a site is valid iff its row and
      // column moves stay inside; an out-of-range site reads the
      // range-checked offset (no memory request)
      const bool up = row - rad >= row_min, dn = row + rad <= row_max;
      const bool lf = col - rad >= col_min, rt = col + rad <= col_max;
      const int y0 = (int)rec[kRecOy] + row + 2 * l, x0 = (int)rec[kRecOx] + col;
      // tile_off(y, x) = a row part + a column part
      auto yo = [&](int y) { return (y & 1) * u.fsz + ((y >> 1) << 5); };
      const int f32 = u.fh << 5;
      auto xo = [&](int x) { return __mul24(x >> 4, f32) + (x & 15); };
      const int ym = yo(y0 - rad), yc = yo(y0), yp = yo(y0 + rad);
      const int xm = xo(x0 - rad), xc = xo(x0), xp = xo(x0 + rad);
      uint32_t p[8];
      // two halves of 4 sites: a half's loads all issued, then its SADs
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        u32x4 t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int dr = site_dr(4 * h + i), dc = site_dc(4 * h + i);
          const bool v = (dr < 0 ? up : dr > 0 ? dn : true) && (dc < 0 ? lf : dc > 0 ? rt : true);
          const int off = (dr < 0 ? ym : dr > 0 ? yp : yc) + (dc < 0 ? xm : dc > 0 ? xp : xc);
          t[i] = __builtin_amdgcn_raw_buffer_load_b128(trs, v ? off : oob, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t acc = sad4(sk[0], t[i].x, 0);
          acc = sad4(sk[1], t[i].y, acc);
          acc = sad4(sk[2], t[i].z, acc);
          p[4 * h + i] = sad4(sk[3], t[i].w, acc);
        }
      }
      mine = 2 * scatter_sum8(p, l);
    }
    const uint32_t key =
        (((mine + mvsad_finish(c, mr, rl, cl_)) << 3) | (uint32_t)l) | (vl ? 0u : ~0u);
    const uint32_t kmin = group_min8(key);
    if (active) {
      ++steps;
      if (kmin < (best << 3)) {
        best = kmin >> 3;
        const int i = (int)(kmin & 7);
        row += site_dr(i) * rad;
        col += site_dc(i) * rad;
        offc = true;
      }
      if (!offc) ++center;
      if (--stp < 0) {  // this diamond_search_sad run is over
        if (l == 0) res[nres] = pack16(col, row);
        ++nres;
        if (first) n = center;  // the first run's num00
        else if (center) n += center;
        first = false;
        if (n < further) {  // the next run, one step shorter
          ++n;
          const uint32_t st = rec[kRecStart];
          row = lo16(st);
          col = hi16(st);
          best = rec[kRecC0];
          stp = kMaxSteps - (step_param + n) - 1;
          center = 0;
          offc = false;
        } else {
          active = false;
          stp = 0;  // a finished job keeps stepping in place at radius 1 (masked)
        }
      }
    }
  }
  wave_sync();
  // var costs of the runs' results in order, strict "<" (full_pixel_diamond),
  // kVarBatch results' rows and mv rates in flight at a time; lane l takes
  // rows l and l + 8.  The linear reference at 32-bit offsets from its
  // (scalar) base: the tiled copy spans the same buffer in under 2^31 bytes
  l = lane_fresh(l);
  const bool mine_job = j0 + jg < njobs;
  const uint8_t* sp = src + rec_i64(rec, kRecSrc);
  uint32_t fr[2][4];
  load_row<4>(sp + (int64_t)l * u.ss, fr[0]);
  load_row<4>(sp + (int64_t)(l + 8) * u.ss, fr[1]);
  const uint32_t lin0 = (uint32_t)(((int)rec[kRecOy] + l) * u.rs + (int)rec[kRecOx]);
  int sme = 0, br = 0, bc = 0;
  {
    // sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum a b, in byte dot products
    // (exact: each sum < 2^22); the source's parts once per job
    uint32_t saa = 0, sa = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        saa = __builtin_amdgcn_udot4(fr[h][i], fr[h][i], saa, false);
        sa = sad4(fr[h][i], 0, sa);
      }
    const bool ent = u.cost_type == 0;
    const int ref_mv_row = lo16(rec[kRecRefMv]), ref_mv_col = hi16(rec[kRecRefMv]);
    typedef const __attribute__((address_space(1))) int32_t* gi32;
    for (int i0 = 0; __builtin_amdgcn_ballot_w64(i0 < nres) != 0; i0 += kVarBatch) {
      uint32_t t[kVarBatch][2][4];
      MvRate m[kVarBatch];
#pragma unroll
      for (int k = 0; k < kVarBatch; ++k) {
        const uint32_t q = res[min(i0 + k, nres - 1)];  // (a surplus slot repeats the last)
        const int r = hi16(q), cc = lo16(q);
        // mv_rate's loads, branch-free as mvsad_rate's (index 0 of kZeroRate
        // for the other cost types)
        const int dr = r * 8 - ref_mv_row, dc = cc * 8 - ref_mv_col;
        const int joint = ent ? ((dc != 0) | ((dr != 0) << 1)) : 0;
        m[k] = MvRate{((gi32)u.mvjcost)[joint], ((gi32)u.mvcost0)[ent ? dr : 0],
                      ((gi32)u.mvcost1)[ent ? dc : 0]};
#pragma unroll
        for (int h = 0; h < 2; ++h)
          load_row<4>(ref + (uint32_t)(lin0 + (uint32_t)((r + 8 * h) * u.rs + cc)), t[k][h]);
      }
#pragma unroll
      for (int k = 0; k < kVarBatch; ++k) {
        const uint32_t q = res[min(i0 + k, nres - 1)];
        const int r = hi16(q), cc = lo16(q);
        uint32_t sbb = saa, sab = 0, sb = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sbb = __builtin_amdgcn_udot4(t[k][h][i], t[k][h][i], sbb, false);
            sab = __builtin_amdgcn_udot4(fr[h][i], t[k][h][i], sab, false);
            sb = sad4(t[k][h][i], 0, sb);
          }
        const uint32_t ts = group_sum8(sa - sb), tq = group_sum8(sbb - 2 * sab);
        const uint32_t var = tq - (uint32_t)(((int64_t)(int)ts * (int)ts) / 256);
        // mv_err_cost (mv_cost of mcomp_dev.h)
        const int dr = r * 8 - ref_mv_row, dc = cc * 8 - ref_mv_col;
        const int mvc =
            ent ? (int)(((int64_t)(m[k].j + m[k].r + m[k].c) * u.error_per_bit + 8192) >> 14)
                : (u.sse_lambda * (abs(dr) + abs(dc))) >> 3;
        const int v = (int)var + mvc;
        if (i0 + k < nres && (i0 + k == 0 || v < sme)) {
          sme = v;
          br = r;
          bc = cc;
        }
      }
    }
  }
  // quality check of the row-skipping search (mcomp.c:1840-1867): sad and
  // sad_skip at the result, rows l and l + 8 of lane l (same parity as l)
  bool full;
  {
    uint32_t all = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      uint32_t t[4];
      load_row<4>(ref + (uint32_t)(lin0 + (uint32_t)((br + 8 * k) * u.rs + bc)), t);
#pragma unroll
      for (int i = 0; i < 4; ++i) all = sad4(fr[k][i], t[i], all);
    }
    const int sad = (int)group_sum8(all);
    const int ssad = (int)(2 * group_sum8((l & 1) ? 0u : all));
    full = sad > 16 && abs(ssad - sad) * 10 >= max(sad, 1) * 9;
  }
  if (!mine_job) return;
  if (full) {  // the full-row rerun is diamond_lj_redo_kernel's
    if (l == 0)
      redo[kLjQueueStride + __hip_atomic_fetch_add(redo, 1, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT)] = j;
    return;
  }
  if (l == 0) {
    LavishDiamondResult r;
    r.best_row = (int16_t)br;
    r.best_col = (int16_t)bc;
    r.bestsme = sme;
    r.steps = steps;
    r.searches = nres;
    out[j] = r;
  }
  if (cost_lists != nullptr) {  // calc_int_sad_list around (br, bc): centre, left, bottom, right, top
    asm volatile("" ::: "memory");  // (the record read here, not carried through the var costs)
    const uint32_t wr = rec[kRecRows], wc = rec[kRecCols], wf = rec[kRecFref];
    const int row_min = lo16(wr), row_max = hi16(wr), col_min = lo16(wc), col_max = hi16(wc);
    Ctx c = u;
    c.full_ref_row = lo16(wf);
    c.full_ref_col = hi16(wf);
    c.oy = (int)rec[kRecOy];
    c.ox = (int)rec[kRecOx];
    l = lane_fresh(l);
    LjSrc s;
    load_row<4>(sp + (int64_t)(2 * l) * u.ss, s.sk);
    int rr[5], cc[5];
    bool vv[5];
    uint32_t sd[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      rr[t] = br + (t == 2 ? 1 : t == 4 ? -1 : 0);
      cc[t] = bc + (t == 1 ? -1 : t == 3 ? 1 : 0);
      vv[t] = t == 0 || (cc[t] >= col_min && cc[t] <= col_max && rr[t] >= row_min && rr[t] <= row_max);
    }
    // lane l: point l's mv cost (lanes 5-7 repeat point 4 and store nothing)
    const int tl = min(l, 4);
    const int rl = br + (tl == 2 ? 1 : tl == 4 ? -1 : 0), cl_ = bc + (tl == 1 ? -1 : tl == 3 ? 1 : 0);
    const bool vl =
        tl == 0 || (cl_ >= col_min && cl_ <= col_max && rl >= row_min && rl <= row_max);
    MvRate m = {0, 0, 0};
    if (dec != nullptr)  // (in-range indices)
      m = lean_rate(u.mvjcost, dec, (vl ? rl : br) - c.full_ref_row,
                    (vl ? cl_ : bc) - c.full_ref_col);
    lj_sads<true, 5>(c, s, l, trs, oob, rr, cc, vv, sd);
    uint32_t sdl = sd[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) sdl = tl == t ? sd[t] : sdl;
    const int mine = vl ? (int)(sdl + mvsad_finish(c, m, rl, cl_)) : INT_MAX;
    if (l < 5) cost_lists[5 * (int64_t)j + l] = mine;
  }
}

#ifndef LAVISH_LJ_LEAN_WAVES
#define LAVISH_LJ_LEAN_WAVES 8  // 512 / 8 = 64 VGPRs: the room beside four transform workgroups
#endif
template <int WPG>
__global__ __launch_bounds__(64 * WPG, LAVISH_LJ_LEAN_WAVES) void diamond_lj_lean_kernel(
    const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs,
    LavishRefTiles tiles, const Job* __restrict__ jobs, int njobs, int step_param,
    LavishMvCostParams cost, const int32_t* dec, LavishDiamondResult* __restrict__ out,
    int32_t* __restrict__ cost_lists, int* __restrict__ queue) {
  __shared__ uint32_t res_s[WPG][kLjJobs][kMaxSteps];
  __shared__ uint32_t rec_s[WPG][kLjJobs][kLjRecWords];
  const int units = (njobs + kLjJobs - 1) / kLjJobs;
  const int x = blockIdx.x & 7;
  const int u0 = units * x / 8, u1 = units * (x + 1) / 8;
  const int lane = threadIdx.x & 63;
  Ctx u{};
  u.ss = ss;
  u.rs = rs;
  u.cost_type = cost.mv_cost_type;
  u.sad_lambda = sad_lambda(cost.mv_cost_type);
  u.sse_lambda = sse_lambda(cost.mv_cost_type);
  u.sad_per_bit = cost.sad_per_bit;
  u.error_per_bit = cost.error_per_bit;
  const bool ent = cost.mv_cost_type == 0;
  u.mvjcost = ent ? cost.mvjcost : kZeroRate;
  u.mvcost0 = ent ? cost.mvcost[0] : kZeroRate;
  u.mvcost1 = ent ? cost.mvcost[1] : kZeroRate;
  u.tiles = tiles.data;
  u.fh = tiles.field_rows;
  u.fsz = (int)tiles.field_bytes;
  const int oob = (int)(2 * tiles.field_bytes);
  const __amdgpu_buffer_rsrc_t trs =
      __builtin_amdgcn_make_buffer_rsrc((void*)tiles.data, 0, oob, 0x00020000);
  int* q = queue + x * kLjQueueStride;
  for (;;) {
    int t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = __builtin_amdgcn_readfirstlane(t);
    if (u0 + t >= u1) break;  // every wave of the label ends here once the range is drained
    lj_lean_jobs(u, src, ref, trs, oob, jobs, njobs, step_param, dec, out, cost_lists,
                 (u0 + t) * kLjJobs, (lds_u32)&res_s[0][0][0], (lds_u32)&rec_s[0][0][0],
                 queue + 8 * kLjQueueStride);
    wave_sync();  // the next unit's record after this unit's last read
  }
}

// the lean search's redo list, walked by a fixed grid with the full body
// (both passes); an empty list ends the kernel at once
template <int WPG>
__global__ __launch_bounds__(64 * WPG, LAVISH_LJ_WAVES) void diamond_lj_redo_kernel(
    const uint8_t* __restrict__ src, int ss, const uint8_t* __restrict__ ref, int rs,
    LavishRefTiles tiles, const Job* __restrict__ jobs, int njobs, int step_param,
    LavishMvCostParams cost, const int32_t* dec, LavishDiamondResult* __restrict__ out,
    int32_t* __restrict__ cost_lists, const int* __restrict__ redo) {
  __shared__ uint32_t res_s[WPG][kLjJobs][kMaxSteps];
  const int n = min(redo[0], njobs);
  if (n <= 0) return;
  const int units = (n + kLjJobs - 1) / kLjJobs;
  const int lane = threadIdx.x & 63;
  const int wave = WPG == 1 ? 0 : threadIdx.x >> 6;
  for (int v = blockIdx.x * WPG + wave; v < units; v += gridDim.x * WPG)
    lj_jobs<true>(src, ss, ref, rs, tiles, jobs, njobs, step_param, cost, dec, 1, out, cost_lists,
                  v * kLjJobs, res_s[wave][lane >> 3], redo + kLjQueueStride, n);
}

// ---------------------------------------------------------------------------
// C2 + C3 in one launch (lavish_txq_frame_search): the <= 16-point class of
// lavish_txq_frame (txq_multi_body<0>) and the 16x16 DIAMOND search's job
// groups (lj_group) in one grid.  The dispatch order -- units of 8
// consecutive workgroups, so a unit keeps the XCD congruence both mappings
// rely on -- places a search unit every `every` units from the start and the
// transform workgroups around them: the long-lived search waves (a dependent
// chain of L2 round trips per job) take a bounded share of the CU slots while
// the transform's write stream keeps the rest, instead of two streams'
// workgroups racing for the slots.  VGPRs: the larger of the two bodies
// (both 115), LDS: the class's 37 KB + the search's result slots.
struct LjLaunch {
  const uint8_t* src;
  int ss;
  const uint8_t* ref;
  int rs;
  LavishRefTiles tiles;
  const Job* jobs;
  int njobs, step_param;
  LavishMvCostParams cost;
  const int32_t* dec;
  int skip;
  LavishDiamondResult* out;
  int32_t* cost_lists;
  int nvwg;   // the search's virtual workgroups (a multiple of 8)
  int units;  // nvwg / 8
  int every;  // a search unit every `every` units of the dispatch order
};

__global__ __launch_bounds__(256, 4) void txq_search_kernel(TxqDispatch d, TxqArgs a0, TxqArgs a1,
                                                            TxqArgs a2, TxqArgs a3, TxqArgs a4,
                                                            TxqArgs a5, TxqArgs a6, TxqArgs a7,
                                                            TxqArgs a8, LjLaunch c) {
  __shared__ __attribute__((aligned(16))) char lds[class_lds(0)];
  const int u = blockIdx.x >> 3, x = blockIdx.x & 7;
  const int k = u / c.every;
  if (u - k * c.every == 0 && k < c.units) {
    lj_group<4>(c.src, c.ss, c.ref, c.rs, c.tiles, c.jobs, c.njobs, c.step_param, c.cost, c.dec,
                c.skip, c.out, c.cost_lists, k * 8 + x, c.nvwg);
    return;
  }
  const int before = min((u + c.every - 1) / c.every, c.units);  // search units in 0 .. u - 1
  txq_multi_body<0>(d, a0, a1, a2, a3, a4, a5, a6, a7, a8, (u - before) * 8 + x, lds);
}

// the decimated entropy cost tables of mvsad_rate_dec
// (+ the search queue's counters zeroed, when given)
__global__ __launch_bounds__(256) void mvcost_dec_kernel(const int32_t* __restrict__ mvcost0,
                                                         const int32_t* __restrict__ mvcost1,
                                                         int32_t* __restrict__ dec,
                                                         int* __restrict__ queue) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (queue != nullptr && i < kLjQueueInts) queue[i] = 0;
  if (i >= 2 * kMvDecN) return;
  const int k = (i % kMvDecN) - kMvDecHalf;
  dec[i] = (i < kMvDecN ? mvcost0 : mvcost1)[8 * k];
}

thread_local StreamScratch t_mvdec;

// at most this many workgroups for the 16x16 DIAMOND search (rounded to 8;
// 0: one per 32 jobs): lavish_set_search_workgroup_cap
static std::atomic<int> g_lj_cap{0};
static int lj_grid_cap() { return g_lj_cap.load(std::memory_order_relaxed); }
// a capped grid: 1 = units pulled from queues (default), 0 = the static
// grid-stride (lavish_set_search_schedule, A/B)
static std::atomic<int> g_lj_queue{1};
// 0 = auto: the lean kernel for a capped, queue-fed search with the
// downsampled SAD; 1 = always diamond_lj_kernel / diamond_lj_dyn_kernel;
// 2 = lean whenever the downsampled SAD is on (lavish_set_search_variant)
static std::atomic<int> g_lj_variant{0};
constexpr int kLjRedoGrid = 128;  // workgroups of the lean search's follow-up launch

// LavishRefTiles copy through LDS, both sides coalesced: a workgroup takes
// field f, strips [k0, k0 + 8) and field rows [fy0, fy0 + 32): it reads the
// 32 source rows' 144-byte segments (the 8 strips + the 16 bytes the last
// strip row overlaps into) as 16-byte chunks, then writes the 8 strips' 1 KB
// runs (32 field rows x 32 bytes each).  Bytes past the row end or past the
// last row are zero.
constexpr int kTilesK = 8, kTilesF = 32, kTilesC = kTilesK + 1;  // chunks per row segment
__global__ __launch_bounds__(256) void ref_tiles_kernel(const uint8_t* __restrict__ ref,
                                                        int stride, int rows, int nstrips,
                                                        int fh, uint8_t* __restrict__ out,
                                                        int ktiles, int ftiles) {
  __shared__ u32x4 seg[kTilesF][kTilesC];
  const int t = threadIdx.x;
  int b = blockIdx.x;
  const int kt = b % ktiles;
  b /= ktiles;
  const int ft = b % ftiles;
  const int f = b / ftiles;
  const int k0 = kt * kTilesK, fy0 = ft * kTilesF;
  for (int idx = t; idx < kTilesF * kTilesC; idx += 256) {
    const int i = idx / kTilesC, m = idx - i * kTilesC;
    const int y = 2 * (fy0 + i) + f, x = 16 * (k0 + m);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (y < rows && x < stride) {
      const uint8_t* p = ref + (int64_t)y * stride + x;
      if (x + 16 <= stride) {
        const u32x4u w = *(const __attribute__((address_space(1))) u32x4u*)p;
        v = u32x4{w.x, w.y, w.z, w.w};
      } else {
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < 16 && x + j < stride; ++j) q[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
        v = u32x4{q[0], q[1], q[2], q[3]};
      }
    }
    seg[i][m] = v;
  }
  __syncthreads();
  for (int q = t; q < kTilesK * kTilesF * 2; q += 256) {
    const int kk = q >> 6, i = (q >> 1) & (kTilesF - 1), h = q & 1;
    const int k = k0 + kk, fy = fy0 + i;
    if (k < nstrips && fy < fh)
      *(u32x4*)(out + ((((int64_t)f * nstrips + k) * fh + fy) << 5) + 16 * h) = seg[i][kk + h];
  }
}

}  // namespace

void launch_lj(const uint8_t* src, int ss, const uint8_t* ref, int rs, const LavishRefTiles& t,
               const LavishDiamondJob* jobs, int njobs, int step_param,
               const LavishMvCostParams& cost, int skip, LavishDiamondResult* out,
               int32_t* cost_lists, hipStream_t s) {
  const int waves = (njobs + kLjJobs - 1) / kLjJobs;
  constexpr int wpg = 4;
  const int nwg = xcd_grid((waves + wpg - 1) / wpg);
  const int cap = lj_grid_cap();
  const int grid = cap > 0 && cap < nwg ? cap : nwg;
  // a capped grid pulls its units from the queues (diamond_lj_dyn_kernel)
  const int variant = g_lj_variant.load(std::memory_order_relaxed);
  const bool queued = grid < nwg && g_lj_queue.load(std::memory_order_relaxed);
  // the lean kernel is queue-fed at any grid (capless: the queues cover all units)
  const bool lean = skip != 0 && (variant == 2 || (variant == 0 && queued));
  const bool dyn = queued || lean;
  constexpr size_t kDecBytes = 2 * kMvDecN * sizeof(int32_t);
  // the queue block, then the lean search's redo list (a job index per job)
  const size_t qbytes = dyn ? (kLjQueueInts + (lean ? (size_t)njobs : 0)) * sizeof(int) : 0;
  int32_t* dec = nullptr;
  int* queue = nullptr;
  char* scr = nullptr;
  if (cost.mv_cost_type == 0 || dyn) {
    scr = (char*)t_mvdec.acquire(kDecBytes + qbytes, s);
    if (dyn) queue = (int*)(scr + kDecBytes);
  }
  if (cost.mv_cost_type == 0) {
    dec = (int32_t*)scr;
    hipLaunchKernelGGL(mvcost_dec_kernel, dim3((2 * kMvDecN + 255) / 256), dim3(256), 0,
                       s, cost.mvcost[0], cost.mvcost[1], dec, queue);
  } else if (dyn) {
    hipLaunchKernelGGL(lj_queue_zero, dim3(1), dim3(kLjQueueInts), 0, s, queue);
  }
  if (lean) {
    hipLaunchKernelGGL(diamond_lj_lean_kernel<wpg>, dim3(grid), dim3(64 * wpg), 0, s, src, ss,
                       ref, rs, t, (const Job*)jobs, njobs, step_param, cost,
                       (const int32_t*)dec, out, cost_lists, queue);
    hipLaunchKernelGGL(diamond_lj_redo_kernel<wpg>, dim3(min(kLjRedoGrid, grid)), dim3(64 * wpg),
                       0, s, src, ss, ref, rs, t, (const Job*)jobs, njobs, step_param, cost,
                       (const int32_t*)dec, out, cost_lists,
                       (const int*)(queue + 8 * kLjQueueStride));
  } else if (dyn)
    hipLaunchKernelGGL(diamond_lj_dyn_kernel<wpg>, dim3(grid), dim3(64 * wpg), 0, s, src,
                       ss, ref, rs, t, (const Job*)jobs, njobs, step_param, cost,
                       (const int32_t*)dec, skip, out, cost_lists, queue);
  else
    hipLaunchKernelGGL(diamond_lj_kernel<wpg>, dim3(grid), dim3(64 * wpg), 0, s, src, ss,
                       ref, rs, t, (const Job*)jobs, njobs, step_param, cost,
                       (const int32_t*)dec, skip, out, cost_lists, nwg);
  if (scr) t_mvdec.release(s);
}

}  // namespace lavish

using namespace lavish;

extern "C" int lavish_set_search_schedule(int queued) {
  if (queued != 0 && queued != 1) return -1;
  lavish::g_lj_queue.store(queued, std::memory_order_relaxed);
  return 0;
}

extern "C" int lavish_set_search_variant(int variant) {
  if (variant < 0 || variant > 2) return -1;
  lavish::g_lj_variant.store(variant, std::memory_order_relaxed);
  return 0;
}

extern "C" int lavish_set_search_workgroup_cap(int workgroups) {
  if (workgroups < 0) return -1;
  lavish::g_lj_cap.store(xcd_grid(workgroups), std::memory_order_relaxed);
  return 0;
}

static int64_t tiles_nstrips(int stride) { return (stride + 15) / 16; }

extern "C" int64_t lavish_ref_tiles_bytes(int stride, int rows) {
  if (stride <= 0 || rows <= 0) return -1;
  return 2 * tiles_nstrips(stride) * ((rows + 1) / 2) * 32;
}

extern "C" int lavish_ref_tiles_build(const uint8_t* ref, int stride, int rows, uint8_t* data,
                                      LavishRefTiles* tiles, void* stream) {
  const int64_t bytes = lavish_ref_tiles_bytes(stride, rows);
  if (ref == nullptr || data == nullptr || tiles == nullptr || bytes <= 0) return -1;
  if (bytes >= ((int64_t)1 << 31)) return -1;  // 32-bit offsets in the search kernels
  const int nstrips = (int)tiles_nstrips(stride), fh = (rows + 1) / 2;
  tiles->data = data;
  tiles->field_bytes = (int64_t)nstrips * fh * 32;
  tiles->field_rows = fh;
  tiles->stride = stride;
  const int ktiles = (nstrips + kTilesK - 1) / kTilesK, ftiles = (fh + kTilesF - 1) / kTilesF;
  hipLaunchKernelGGL(ref_tiles_kernel, dim3((unsigned)(2 * ktiles * ftiles)), dim3(256), 0,
                     (hipStream_t)stream, ref, stride, rows, nstrips, fh, data, ktiles, ftiles);
  LAVISH_CHECK(hipGetLastError());
  return 0;
}

extern "C" int lavish_txq_frame_search(
    const int16_t* residual, int stride, int width, int height, uint32_t size_mask,
    const uint32_t* type_masks, int bit_depth, int quant_kind, const LavishQuantParams* qp,
    int32_t* const* qcoeff, int32_t* const* dqcoeff, uint16_t* const* eob, const uint8_t* src,
    int src_stride, const uint8_t* ref, int ref_stride, const LavishRefTiles* tiles,
    const LavishDiamondJob* jobs, int njobs, int step_param, const LavishMvCostParams* cost,
    int use_downsampled_sad, LavishDiamondResult* out, int32_t* cost_lists, int every,
    void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (every < 1) return -6;
  if (tiles == nullptr || tiles->data == nullptr || tiles->stride != ref_stride) return -5;
  if (step_param < 0 || step_param >= kMaxSteps) return -1;
  if (!mv_cost_ok(cost)) return -2;
  // C2: every requested size outside the <= 16-point class as lavish_txq_frame
  // runs it (the 64-point sizes, then the 32-point class's launch)
  uint32_t cls0 = 0;
  for (int t = 0; t < 19; ++t)
    if (((size_mask >> t) & 1) && tx_w(t) <= 32 && tx_h(t) <= 32 && !txq_class(t)) cls0 |= 1u << t;
  int rc = 0;
  if (size_mask & ~cls0) {
    rc = txq_frame(residual, stride, width, height, size_mask & ~cls0, type_masks, bit_depth,
                   quant_kind, qp, qcoeff, dqcoeff, eob, s);
    if (rc) return rc;
  }
  TxqMulti m;
  int g = 0;
  rc = txq_frame_plan(residual, stride, width, height, cls0, type_masks, bit_depth, quant_kind, qp,
                      qcoeff, dqcoeff, eob, 0, m, g);
  if (rc) return rc;
  LjLaunch c{};
  c.src = src;
  c.ss = src_stride;
  c.ref = ref;
  c.rs = ref_stride;
  c.tiles = *tiles;
  c.jobs = (const Job*)jobs;
  c.njobs = njobs > 0 ? njobs : 0;
  c.step_param = step_param;
  c.cost = *cost;
  c.skip = use_downsampled_sad;
  c.out = out;
  c.cost_lists = cost_lists;
  const int waves = (c.njobs + kLjJobs - 1) / kLjJobs;
  c.nvwg = xcd_grid((waves + 3) / 4);
  c.units = c.nvwg / 8;
  if (c.units > 0 && cost->mv_cost_type == 0) {
    c.dec = (const int32_t*)t_mvdec.acquire(2 * kMvDecN * sizeof(int32_t), s);
    hipLaunchKernelGGL(mvcost_dec_kernel, dim3((2 * kMvDecN + 255) / 256), dim3(256), 0, s,
                       cost->mvcost[0], cost->mvcost[1], (int32_t*)c.dec, (int*)nullptr);
  }
  // the search units must all lie inside the grid: units * every may not
  // pass the grid's units (clamp the spacing)
  const int u2 = g / 8, ut = u2 + c.units;
  c.every = c.units > 1 ? min(every, max(1, (ut - 1) / (c.units - 1))) : every;
  if (ut > 0)
    hipLaunchKernelGGL(txq_search_kernel, dim3(ut * 8), dim3(256), 0, s, m.d, m.a[0], m.a[1],
                       m.a[2], m.a[3], m.a[4], m.a[5], m.a[6], m.a[7], m.a[8], c);
  LAVISH_CHECK(hipGetLastError());
  if (c.dec) t_mvdec.release(s);
  return 0;
}
