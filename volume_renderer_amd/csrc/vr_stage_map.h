// vr_stage_map.h -- the lane map of the staging copy (vr_stage.h stage_box): which floats of a box a
// lane moves in which pass, with V = 1, 2 or 4 consecutive floats of a row per lane.  Plain C++:
// also compiled on the host (tests/test_stage_map_host.py simulates the 64 lanes with these very
// functions).
//
// A row of ex floats is cut into gx = ceil(ex / V) groups of V floats; lane -> (row slot, group), so a
// pass moves per = 64 / gx whole rows and the box takes ceil(rows / per) passes (rows = ey * ez).
// The last group of a row starts at x = ex - V, not at V * (gx - 1): when ex is no multiple of V it
// overlaps its neighbour (two lanes move the same floats to the same slot words) and no lane touches
// anything beyond its own row.  Needs V <= ex <= 64.
//
// Quotients by the wave-uniform gx, per and ey are udiv_small's (vr_udiv.h).  Its bounds hold: gx and
// per are at most 64; the dividends are the lane (< 64), its row slot (<= lane) and the row count
// rounded up to a pass (< rows + 64, which the caller keeps below UDIV_MAX_N).  ey may exceed 64 (a
// narrow box): a row slot below 64 then has the quotient 0 by 64 as well.
#pragma once
#include <stdint.h>

#include "vr_udiv.h"

#ifndef VR_UDIV_MAGIC
// 1 (round 15): the quotients as udiv_small, the magics from a table (on the device in constant memory,
// one scalar load each); 0 (A/B, tests): the compiler's u32 division sequences
#define VR_UDIV_MAGIC 1
#endif

namespace vr {

// n / d (n % d from the quotient q), m = udiv_magic(d)
VR_UDIV_HD inline uint32_t stage_div(uint32_t n, uint32_t d, uint32_t m) {
#if VR_UDIV_MAGIC
  (void)d;
  return udiv_small(n, m);
#else
  (void)m;
  return n / d;
#endif
}
VR_UDIV_HD inline uint32_t stage_rem(uint32_t n, uint32_t q, uint32_t d) {
#if VR_UDIV_MAGIC
  return urem_small(n, q, d);
#else
  (void)q;
  return n % d;
#endif
}

// Floats per lane for a row of ex floats: the widest of 4, 2, 1 that is at most vmax and at most ex.
VR_UDIV_HD inline int stage_width(uint32_t ex, int vmax) {
  return (vmax >= 4 && ex >= 4u) ? 4 : ((vmax >= 2 && ex >= 2u) ? 2 : 1);
}

// The wave-uniform part of the map.
struct StageMap {
  uint32_t gx;      // groups per row
  uint32_t per;     // rows per pass
  uint32_t x_last;  // first float of a row's last group
  uint32_t ey;
  uint32_t m_gx, m_per, m_ey;  // udiv_magic of gx, per and min(ey, 64)
  uint32_t wq, wr;             // per = wq * ey + wr: the planes and rows a pass advances
};
template <int V>
VR_UDIV_HD inline StageMap stage_map(uint32_t ex, uint32_t ey, const UdivTab &tab) {
  StageMap M;
  M.gx = (ex + (uint32_t)(V - 1)) / (uint32_t)V;
  M.m_gx = tab.e[M.gx].m;
  M.m_per = tab.e[M.gx].mper;
  M.per = stage_div(64u, M.gx, M.m_gx);
  M.x_last = ex - (uint32_t)V;
  M.ey = ey;
  M.m_ey = tab.e[ey < 64u ? ey : 64u].m;
  M.wq = M.per < ey ? 0u : stage_div(M.per, ey, M.m_ey);  // (per <= 64: ey <= 64 where it is divided)
  M.wr = M.per - M.wq * ey;
  return M;
}

// Passes of the whole box.
VR_UDIV_HD inline uint32_t stage_passes(const StageMap &M, uint32_t rows) {
  return stage_div(rows + M.per - 1u, M.per, M.m_per);
}

// A lane's part: the x of its group, the (y, z) of its first row, and the number of passes in which
// it has a row (0 for the lanes beyond per * gx).
struct StageLane {
  uint32_t x, y, z, n;
};
template <int V>
VR_UDIV_HD inline StageLane stage_lane(const StageMap &M, uint32_t lane, uint32_t rows) {
  const uint32_t rr = stage_div(lane, M.gx, M.m_gx);  // row slot
  const uint32_t xg = stage_rem(lane, rr, M.gx);
  StageLane s;
  if (V == 1) {
    s.x = xg;
  } else {
    const uint32_t x = xg * (uint32_t)V;
    s.x = x < M.x_last ? x : M.x_last;
  }
  s.n = rr < M.per ? stage_div(rows - rr + M.per - 1u, M.per, M.m_per) : 0u;
  s.z = stage_div(rr, M.ey, M.m_ey);
  s.y = stage_rem(rr, s.z, M.ey);
  return s;
}

// From one pass to the next a lane's row moves on by `per` rows: wq whole planes and wr rows
// (StageMap), so y + wr crosses at most one more plane.  g: the lane's offset in the source (in `unit`s
// of an element: 4 for bytes; OffT wide), l: its slot word.  g_row / l_row: the advance of per rows with
// its wq plane steps; g_wrap / l_wrap: what one more plane step adds (the plane pitch less ey row
// pitches: 0 for a dense pitch).
template <class OffT>
struct StageStep {
  OffT g_row, g_wrap;
  int32_t l_row, l_wrap;
};
template <class OffT>
VR_UDIV_HD inline StageStep<OffT> stage_step(const StageMap &M, OffT px, OffT pxy, OffT unit, int32_t lpx, int32_t lpxy) {
  StageStep<OffT> S;
  S.g_wrap = (pxy - (OffT)M.ey * px) * unit;
  S.g_row = (OffT)M.per * px * unit + (OffT)M.wq * S.g_wrap;
  S.l_wrap = lpxy - (int32_t)M.ey * lpx;
  S.l_row = (int32_t)M.per * lpx + (int32_t)M.wq * S.l_wrap;
  return S;
}
template <class OffT>
VR_UDIV_HD inline void stage_next(const StageMap &M, const StageStep<OffT> &S, OffT &g, int32_t &l, uint32_t &y) {
  g += S.g_row;
  l += S.l_row;
  y += M.wr;
  // (at most once.  Written as a loop: as an `if` the device compiler selects instead of branching, and
  // the scalar registers of the march's lit sample loop move -- four s_mov_b64 more per iteration)
  while (y >= M.ey) {
    y -= M.ey;
    g += S.g_wrap;
    l += S.l_wrap;
  }
}

}  // namespace vr
