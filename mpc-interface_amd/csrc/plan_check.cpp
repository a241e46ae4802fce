// plan_check.cpp -- the checker of plan tables: what mpcasm_plan_create and every table-taking entry of capi.hip
// run before anything else reads a plan.  Host only: no HIP header, builds with a plain C++17 compiler (the
// sanitizer sweep of tools/plan_check_sweep.cpp links this file alone).  One function per family of
// plan_tables.h, all on the same small context; every sum or product of table words is formed in int64_t, so
// that no bound can wrap.
#include "plan_check.h"

#include <string.h>

#include <algorithm>
#include <vector>

namespace mpcasm {
namespace {

// section [off, off + len) must lie inside [lo, n)
bool in_range(int64_t off, int64_t len, int64_t n, int64_t lo) {
  return off >= lo && len >= 0 && off + len <= n;
}

// the tables under check: itab (n words), dtab (nd doubles)
struct Tables {
  const int32_t* it;
  const double* dt;
  int64_t n, nd;
  int64_t h(int word) const { return it[word]; }                 // a header word, widened
  const int32_t* at(int word) const { return it + it[word]; }    // the section a header word points to
  bool sec(int word, int64_t len) const { return in_range(it[word], len, n, H_WORDS); }   // ... inside itab
  bool dsec(int word, int64_t len) const { return in_range(it[word], len, nd, 0); }       // ... inside dtab
};

// the signed low 24 bits of a column-table word (elements per base row)
int64_t low24(int32_t w) {
  const int64_t v = w & 0xFFFFFF;
  return v >= 0x800000 ? v - 0x1000000 : v;
}

// the per-column table of the diagonal gterms (H_OFF_RS_DPAR, H_DOFF_RS_DCOEF; read when no column has more than
// RS_DIAG_MAX): aligned sections, every slot a parameter or the free one
bool diag_table_ok(const Tables& t) {
  const int64_t no = t.h(H_NO), nparams = t.h(H_NPARAMS);
  if (!t.sec(H_OFF_RS_DPAR, no * 2 * RS_DIAG_MAX) || t.h(H_OFF_RS_DPAR) % 4 ||
      !t.dsec(H_DOFF_RS_DCOEF, no * RS_DIAG_MAX) || t.h(H_DOFF_RS_DCOEF) % 2)
    return false;
  const int32_t* dp = t.at(H_OFF_RS_DPAR);
  for (int64_t i = 0; i < no * 2 * RS_DIAG_MAX; ++i)
    if (dp[i] < 0 || dp[i] > nparams) return false;
  return true;
}

// a row record of G: its number of axes, the extreme's slot, every axis' arrow and centre a parameter or the
// free slot
bool row_record_slots_ok(const int32_t* x, int64_t nparams) {
  if (x[RR_NAXES] < 0 || x[RR_NAXES] > RS_AXMAX || x[RR_EXTREME] < 0 || x[RR_EXTREME] >= nparams) return false;
  for (int a = 0; a < RS_AXMAX; ++a)
    if (x[RR_ARROW + a] < 0 || x[RR_ARROW + a] > nparams || x[RR_CENTER + a] < 0 || x[RR_CENTER + a] > nparams)
      return false;
  return true;
}

// ---- header and section ranges ----------------------------------------------------------------------------
int check_header(const int32_t* it, size_t n_itab, size_t n_dtab) {
  if (n_itab < (size_t)H_WORDS) return MPCASM_ERR_PLAN;
  if (it[H_MAGIC] != PLAN_MAGIC || it[H_VERSION] != PLAN_VERSION) return MPCASM_ERR_PLAN;
  if ((size_t)it[H_NITAB] != n_itab || (size_t)it[H_NDTAB] != n_dtab) return MPCASM_ERR_PLAN;
  if (it[H_NG] < 0 || it[H_NO] < 0 || it[H_NC] < 0 || it[H_NPARAMS] < 0) return MPCASM_ERR_PLAN;
  if (it[H_NSRC] < 0 || it[H_NSRC] > MAX_SOURCES) return MPCASM_ERR_LIMIT;
  if (it[H_LDV] < (int64_t)it[H_NO] + 1 || (it[H_LDV] & 1)) return MPCASM_ERR_PLAN;
  return MPCASM_OK;
}

bool check_sections(const Tables& t) {
  const int64_t W = t.h(H_NG) + t.h(H_NO);
  bool ok = true;
  ok = ok && t.sec(H_OFF_SEG, t.h(H_NSEG) * SEG_WORDS);
  ok = ok && t.sec(H_OFF_COLSEG, t.h(H_NBASE) * W);
  ok = ok && t.sec(H_OFF_ROWPTR, t.h(H_RTOT) + 1);
  ok = ok && t.sec(H_OFF_ENTBASE, t.h(H_NENT));
  ok = ok && t.sec(H_OFF_ENTK, t.h(H_NENT));
  ok = ok && t.sec(H_OFF_GTERM, t.h(H_NGTERM) * GT_WORDS);
  ok = ok && t.sec(H_OFF_LIMIT, t.h(H_NLIMIT) * LM_WORDS);
  ok = ok && t.sec(H_OFF_LAX, t.h(H_NLAX) * LX_WORDS);
  ok = ok && t.sec(H_OFF_ROWLIMIT, t.h(H_NC));
  ok = ok && t.sec(H_OFF_PM_ROWPTR, t.h(H_PMROWS) + 1);
  ok = ok && t.sec(H_OFF_PM_ENTBASE, t.h(H_PM_NENT));
  ok = ok && t.sec(H_OFF_PM_ENTK, t.h(H_PM_NENT));
  ok = ok && t.dsec(H_DOFF_ENTCOEF, t.h(H_NENT));
  ok = ok && t.dsec(H_DOFF_PM_ENTCOEF, t.h(H_PM_NENT));
  ok = ok && t.dsec(H_DOFF_DIAGCOEF, t.h(H_NDIAGCOEF));
  if (t.h(H_FUSED_OK) != 0 && t.h(H_FUSED_OK) != 1) return false;
  if (t.h(H_FUSED_OK)) {
    ok = ok && t.h(H_ARENA_TOTAL) >= 1 && t.h(H_NFD) >= 0 && t.h(H_NOPS) >= 0 && t.h(H_NCOEF) >= 0;
    ok = ok && t.sec(H_OFF_ARENA, t.h(H_NSRC) * 2);
    ok = ok && t.sec(H_OFF_FD_IDX, t.h(H_NFD));
    ok = ok && t.sec(H_OFF_FD_PTR, t.h(H_NFD) + 1);
    ok = ok && t.sec(H_OFF_OP, t.h(H_NOPS) * 2);
    ok = ok && t.dsec(H_DOFF_COEFPOOL, t.h(H_NCOEF));
  }
  return ok;
}

// ---- fused program ----------------------------------------------------------------------------------------
bool check_fused(const Tables& t) {
  if (!t.h(H_FUSED_OK)) return true;
  const int64_t nsrc = t.h(H_NSRC), total = t.h(H_ARENA_TOTAL), nfd = t.h(H_NFD), nops = t.h(H_NOPS);
  const int32_t* ar = t.at(H_OFF_ARENA);
  for (int64_t s = 0; s < nsrc; ++s)
    if (ar[2 * s] < 1 || ar[2 * s + 1] < 0 || (int64_t)ar[2 * s] + ar[2 * s + 1] > total) return false;
  const int64_t vsize = t.h(H_RTOT) * t.h(H_LDV);
  const int32_t* fi = t.at(H_OFF_FD_IDX);
  const int32_t* fp = t.at(H_OFF_FD_PTR);
  if (fp[0] != 0 || fp[nfd] != nops) return false;
  for (int64_t i = 0; i < nfd; ++i)
    if (fi[i] < 0 || fi[i] >= vsize || fp[i + 1] < fp[i]) return false;
  const uint32_t* op = reinterpret_cast<const uint32_t*>(t.at(H_OFF_OP));
  for (int64_t o = 0; o < nops; ++o) {
    if (op[2 * o] >= (uint32_t)total) return false;
    if ((op[2 * o + 1] >> 16) > (uint32_t)t.h(H_NG) || (op[2 * o + 1] & 0xFFFFu) >= (uint32_t)t.h(H_NCOEF))
      return false;
  }
  return true;
}

// ---- the element program of the preview matrices ----------------------------------------------------------
bool check_preview_program(const Tables& t) {
  if (t.h(H_PM_NFD) < 0) return false;
  if (t.h(H_PM_NFD) == 0) return true;
  const int64_t nfd = t.h(H_PM_NFD), nops = t.h(H_PM_NOPS), npool = t.h(H_PM_NPOOL), nsrc = t.h(H_NSRC);
  const int64_t elems = t.h(H_PMROWS) * (t.h(H_NG) + t.h(H_NO));
  if (nops < nfd || npool < 1 || elems < nfd || !t.sec(H_OFF_PM_MAP, elems) || !t.sec(H_OFF_PM_FDPTR, nfd + 1) ||
      !t.sec(H_OFF_PM_OP, nops * 2) || t.h(H_OFF_PM_OP) % 2 || !t.dsec(H_DOFF_PM_POOL, npool) ||
      !t.sec(H_OFF_ARENA, nsrc * 2) || nsrc > 254)
    return false;
  const int32_t* mp = t.at(H_OFF_PM_MAP);
  for (int64_t e = 0; e < elems; ++e)
    if (mp[e] < -1 || mp[e] >= nfd) return false;
  const int32_t* fp = t.at(H_OFF_PM_FDPTR);
  if (fp[0] != 0 || fp[nfd] != nops) return false;
  for (int64_t i = 0; i < nfd; ++i)
    if (fp[i + 1] < fp[i]) return false;
  const uint32_t* op = reinterpret_cast<const uint32_t*>(t.at(H_OFF_PM_OP));
  const int32_t* ar = t.at(H_OFF_ARENA);
  for (int64_t o = 0; o < nops; ++o) {
    const uint32_t sid = op[2 * o + 1] & 255u, cid = op[2 * o + 1] >> 8;
    if (cid >= (uint64_t)npool) return false;
    if (sid == 255u) {
      if (op[2 * o] != 0) return false;
    } else if (sid >= (uint32_t)nsrc || ar[2 * sid + 1] < 0 || op[2 * o] >= (uint32_t)ar[2 * sid + 1]) {
      return false;
    }
  }
  return true;
}

// ---- resident program (the persistent kernel's tables) ----------------------------------------------------
// the workspace's geometry (plan_tables.h H_RS_COMPACT), read once the header part has been checked
struct Workspace {
  int64_t ldv, vd, row0, rows, size;
};
Workspace resident_workspace(const Tables& t) {
  Workspace w;
  w.ldv = t.h(H_RS_LDV);
  w.vd = t.h(H_RS_VD);
  w.row0 = t.h(H_RS_VROW0);
  w.rows = w.row0 + t.h(H_RTOT);
  w.size = w.rows * w.ldv;
  return w;
}

// sizes, section ranges, the constants, the workspace's geometry
bool check_resident_header(const Tables& t) {
  const int64_t ng = t.h(H_NG), no = t.h(H_NO), nc = t.h(H_NC), nparams = t.h(H_NPARAMS);
  const int64_t jc = t.h(H_RS_JC), slots = jc * RS_NT;
  const int64_t img = t.h(H_RS_IMG), unit = t.h(H_RS_UNIT), nchunk = t.h(H_RS_NCHUNK);
  if (jc < 1 || jc > RS_JC_MAX || t.h(H_RS_NTRIP) < 0 || t.h(H_RS_NSPLIT) < 0) return false;
  const int64_t dma = t.h(H_RS_IMG_DMA), nlti = t.h(H_RS_NLTI), nab = t.h(H_RS_AB);
  if ((unit != 4 && unit != 16) || dma < 128 || dma % 128 || img < dma || (img & 1) || img > 65535 ||
      nchunk * 64 * unit != dma * 8 || nparams > 65535 || nlti < 0 || nlti > RS_LTI_MAX || nab < 0 || nab % 32 ||
      nab > 4096 || (nlti == 0) != (nab == 0))
    return false;
  bool r = true;
  r = r && t.sec(H_OFF_RS_SRC, slots);
  r = r && t.sec(H_OFF_RS_GIDX, slots);
  r = r && t.sec(H_OFF_RS_DST, slots);
  r = r && t.dsec(H_DOFF_RS_COEF, slots);
  // (two spare records behind the table: the kernel reads that far ahead)
  r = r && t.sec(H_OFF_RS_TRIP, (t.h(H_RS_NTRIP) + 2) * RS_TRIP_WORDS);
  r = r && t.sec(H_OFF_RS_WTRIP, RS_WAVES * 2);
  r = r && t.sec(H_OFF_RS_SPLIT, t.h(H_RS_NSPLIT));
  r = r && t.h(H_RS_NZBLK) >= 0 && t.sec(H_OFF_RS_ZBLK, t.h(H_RS_NZBLK));
  r = r && (t.h(H_OFF_RS_TRIP) % 8 == 0);
  r = r && t.sec(H_OFF_RS_RR, nc * RS_RR_WORDS) && t.h(H_OFF_RS_RR) % 4 == 0;
  r = r && t.sec(H_OFF_RS_INMETA, nchunk * 64 * 2) && t.h(H_OFF_RS_INMETA) % 2 == 0;
  r = r && t.dsec(H_DOFF_RS_CONST, 4) && t.h(H_DOFF_RS_CONST) % 2 == 0;
  r = r && in_range(t.h(H_RS_IMG_GIVEN), ng + 1, dma, 0);
  r = r && in_range(t.h(H_RS_IMG_PARAMS), nparams + 1, dma, 0);
  r = r && t.sec(H_OFF_RS_LTI, nlti * RS_LTI_WORDS);
  r = r && t.sec(H_OFF_RS_ABMETA, nab * 4) && t.h(H_OFF_RS_ABMETA) % 2 == 0;
  if (!r) return false;
  const double* c = t.dt + t.h(H_DOFF_RS_CONST);
  if (c[0] != 1.0 || c[1] != 1.0 || c[2] != 0.0 || c[3] != 0.0) return false;
  // the workspace's geometry: dense = the fused kernel's, or compact
  const Workspace w = resident_workspace(t);
  if (t.h(H_RS_COMPACT) == 0) return w.ldv == t.h(H_LDV) && w.vd == no && w.row0 == 0;
  return t.h(H_RS_COMPACT) == 1 && w.ldv >= 6 && w.ldv % 4 == 2 && w.vd == w.ldv - 2 && w.vd <= no + 3 &&
         w.row0 >= 0 && w.row0 % 4 == 0 && w.row0 <= 1024 && t.h(H_RR_PACKED) && t.h(H_CSC_PNNZ) == 0 &&
         t.h(H_CSC_GNNZ) == 0 && t.sec(H_OFF_RS_RRWIN, nc);
}

// the compose program (four tables and their packed copy), the split elements, the zero blocks of P
bool check_resident_compose(const Tables& t) {
  const int64_t slots = t.h(H_RS_JC) * RS_NT, img = t.h(H_RS_IMG), vsize = resident_workspace(t).size;
  const int32_t* ts = t.at(H_OFF_RS_SRC);
  const int32_t* tg = t.at(H_OFF_RS_GIDX);
  const int32_t* td = t.at(H_OFF_RS_DST);
  for (int64_t i = 0; i < slots; ++i)
    if (ts[i] < 0 || ts[i] >= img || tg[i] < 0 || tg[i] >= img || td[i] < -1 ||
        (td[i] >= 0 && (td[i] & ~RS_DST_ACC) >= vsize))
      return false;
  {  // the packed copy of the program says what the four tables say
    if (!t.sec(H_OFF_RS_PROG, slots * 4) || t.h(H_OFF_RS_PROG) % 4) return false;
    const int32_t* pr = t.at(H_OFF_RS_PROG);
    const double* tc = t.dt + t.h(H_DOFF_RS_COEF);
    for (int64_t i = 0; i < slots; ++i)
      if ((uint32_t)pr[4 * i] != ((uint32_t)ts[i] | ((uint32_t)tg[i] << 16)) || pr[4 * i + 1] != td[i] ||
          memcmp(pr + 4 * i + 2, &tc[i], sizeof(double)) != 0)
        return false;
  }
  const int32_t* sp = t.at(H_OFF_RS_SPLIT);
  for (int64_t i = 0; i < t.h(H_RS_NSPLIT); ++i)
    if (sp[i] < 0 || sp[i] >= vsize) return false;
  const int64_t nb = (t.h(H_NO) + 3) / 4;  // 4-column blocks of the unknowns
  if (nb > RS_BLOCKS_MAX) return false;
  const int32_t* zb = t.at(H_OFF_RS_ZBLK);
  for (int64_t i = 0; i < t.h(H_RS_NZBLK); ++i)
    if (zb[i] < 0 || (zb[i] >> 8) >= nb || (zb[i] & 255) >= nb) return false;
  return true;
}

// the trip records: what every one of them reads stays inside the workspace and the parameters
bool check_resident_trips(const Tables& t) {
  const int64_t no = t.h(H_NO), nparams = t.h(H_NPARAMS), ntrip = t.h(H_RS_NTRIP), rtot = t.h(H_RTOT);
  const int64_t nb = (no + 3) / 4;
  const Workspace w = resident_workspace(t);
  const int32_t* tr = t.at(H_OFF_RS_TRIP);
  for (int i = 0; i < 2 * RS_TRIP_WORDS; ++i)
    if (tr[ntrip * RS_TRIP_WORDS + i] != 0) return false;
  const int64_t row_bytes = w.ldv * 8;
  if (t.h(H_LDV) < no + 2) return false;  // columns: unknowns, d, ones
  for (int64_t i = 0; i < ntrip; ++i) {
    const int32_t* x = tr + i * RS_TRIP_WORDS;
    const int word = x[RT_WORD], rows = word & 31;
    const int live = (word >> RT_LIVE) & 15, qmask = (word >> RT_QMASK) & 15;
    const bool is_short = (word >> RT_SHORT) & 1;
    if (word < 0 || (word >> 19) != 0 || (rows != 0 && rows != 4 && rows != 16) || (qmask & ~live) || live == 0 ||
        (is_short != (rows == 4)) || (rows == 0 && ((word >> RT_TERM_END) & 1)) || x[RT_W] < 0 || x[RT_W] % 8 ||
        x[RT_W] / 8 >= nparams || x[RT_AIM] < 0 || x[RT_AIM] % 8 || x[RT_AIM] / 8 >= nparams)
      return false;
    for (int g = 0; g < 4; ++g)  // (all four groups load, live or not)
      if (((x[RT_BI] >> (8 * g)) & 255) >= nb || ((x[RT_BJ] >> (8 * g)) & 255) >= nb) return false;
    // offsets: whole rows on group boundaries (the d offset: column RS_VD of its row); a trip
    // reads `rows` rows from each
    if (t.h(H_RS_COMPACT) == 0) {
      const int64_t offs[3] = {x[RT_A], x[RT_B], (int64_t)x[RT_D] - (rows > 0 ? no * 8 : 0)};
      for (int k = 0; k < 3; ++k)
        if (offs[k] < 0 || offs[k] % (4 * row_bytes) || offs[k] / row_bytes + rows > rtot) return false;
    } else if (rows > 0) {
      // compact: the offsets carry the window's first column; what every group really reads -- 32
      // bytes at its block in each of the rows -- stays inside the workspace
      const int64_t d = (int64_t)x[RT_D] - w.vd * 8;
      if (d < 0 || d % (4 * row_bytes) || d / row_bytes + rows > w.rows) return false;
      for (int g = 0; g < 4; ++g) {
        const int64_t a = (int64_t)x[RT_A] + 32 * ((x[RT_BI] >> (8 * g)) & 255);
        const int64_t b = (int64_t)x[RT_B] + 32 * ((x[RT_BJ] >> (8 * g)) & 255);
        if (a < 0 || a % 32 || a + (rows - 1) * row_bytes + 32 > w.size * 8) return false;
        if (!((qmask >> g) & 1) && (b < 0 || b % 32 || b + (rows - 1) * row_bytes + 32 > w.size * 8)) return false;
      }
    }
  }
  // every wavefront's trips: consecutive, whole packs (first ... last)
  const int32_t* wt = t.at(H_OFF_RS_WTRIP);
  int64_t next = 0;
  for (int wv = 0; wv < RS_WAVES; ++wv) {
    if (wt[2 * wv] != next || wt[2 * wv + 1] < 0) return false;
    const int64_t first = next;
    next += wt[2 * wv + 1];
    if (next > ntrip) return false;
    const int32_t* open = nullptr;
    for (int64_t i = first; i < next; ++i) {
      const int32_t* x = tr + i * RS_TRIP_WORDS;
      const int word = x[RT_WORD];
      if ((word >> RT_FIRST) & 1) {
        if (open != nullptr) return false;
        open = x;
      }
      if (open == nullptr || open[RT_BI] != x[RT_BI] || open[RT_BJ] != x[RT_BJ] ||
          (((open[RT_WORD] ^ word) >> RT_LIVE) & 0xFF) != 0)  // live groups, groups of q
        return false;
      if ((word >> RT_LAST) & 1) open = nullptr;
    }
    if (open != nullptr) return false;
  }
  return next == ntrip;
}

// the row records of G, their packed words and (compact) their windows
bool check_resident_rows(const Tables& t) {
  const int64_t no = t.h(H_NO), nc = t.h(H_NC), nparams = t.h(H_NPARAMS);
  const Workspace w = resident_workspace(t);
  const int32_t* rrw = t.at(H_OFF_RS_RR);
  for (int64_t R = 0; R < nc; ++R) {
    const int32_t* x = rrw + R * RS_RR_WORDS;
    if (!row_record_slots_ok(x, nparams)) return false;
    for (int a = 0; a < RS_AXMAX; ++a)
      if (x[RR_VOFF + a] < 0 || x[RR_VOFF + a] % w.ldv != 0 || x[RR_VOFF + a] / w.ldv >= std::max<int64_t>(w.rows, 1))
        return false;
    // the packed words the 16-byte-piece path of G reads instead of the fields above
    if (t.h(H_RR_PACKED) &&
        (x[RR_NAXES] > 2 || x[RR_VOFF] > 65535 || x[RR_VOFF + 1] > 65535 || x[RR_ARROW] > 65535 ||
         x[RR_ARROW + 1] > 65535 ||
         (uint32_t)x[RR_PACKED] != ((uint32_t)x[RR_VOFF] | ((uint32_t)x[RR_VOFF + 1] << 16)) ||
         (uint32_t)x[RR_PACKED + 1] != ((uint32_t)x[RR_ARROW] | ((uint32_t)x[RR_ARROW + 1] << 16))))
      return false;
  }
  if (t.h(H_RR_PACKED) != 0 && (t.h(H_RR_PACKED) != 1 || (no & 1) || nc < 1)) return false;
  if (t.h(H_RS_COMPACT)) {  // a window lies inside its row: first + count column pairs <= RS_VD / 2
    const int32_t* win = t.at(H_OFF_RS_RRWIN);
    for (int64_t R = 0; R < nc; ++R)
      for (int a = 0; a < 2; ++a) {
        const uint32_t v = ((uint32_t)win[R] >> (16 * a)) & 0xFFFF;
        if (2 * (int64_t)(v >> 8) > w.vd) return false;
      }
  }
  return true;
}

// the per-column tables of the diagonal gterms and the piece descriptors of G
bool check_resident_descriptors(const Tables& t) {
  const int64_t no = t.h(H_NO), nc = t.h(H_NC), nparams = t.h(H_NPARAMS), ngd = t.h(H_RS_NGDESC);
  const int32_t* rrw = t.at(H_OFF_RS_RR);
  if (!diag_table_ok(t)) return false;
  if (ngd == 0) return t.h(H_RS_NGFIX) == 0;
  const int64_t pieces = nc * (no / 2);
  if (t.h(H_RS_GSINGLE) < 0 || (t.h(H_RS_GSINGLE) >> (RS_GDESC_PIECES * (RS_GDESC_THREADS / 64))) != 0) return false;
  if (!t.h(H_RR_PACKED) || ngd != (int64_t)RS_GDESC_PIECES * RS_GDESC_THREADS || pieces > ngd ||
      !t.sec(H_OFF_RS_GDESC, ngd * 2) || t.h(H_OFF_RS_GDESC) % 2)
    return false;
  const int32_t* gd = t.at(H_OFF_RS_GDESC);
  for (int64_t e = 0; e < ngd; ++e) {  // the same numbers as the row record of the piece
    const int64_t R = e < pieces ? e / (no / 2) : 0, cp = e < pieces ? e % (no / 2) : 0;
    const int32_t* x = rrw + R * RS_RR_WORDS;
    uint32_t v0 = (uint32_t)x[RR_VOFF] + 2 * (uint32_t)cp, v1 = (uint32_t)x[RR_VOFF + 1] + 2 * (uint32_t)cp;
    uint32_t a0 = (uint32_t)x[RR_ARROW], a1 = (uint32_t)x[RR_ARROW + 1];
    if (t.h(H_RS_COMPACT)) {  // ... the piece inside the axis' window, or row 0 and the zero arrow
      const uint32_t win = (uint32_t)t.at(H_OFF_RS_RRWIN)[R];
      const uint32_t d0 = (uint32_t)cp - (win & 255), d1 = (uint32_t)cp - ((win >> 16) & 255);
      const bool in0 = d0 < ((win >> 8) & 255), in1 = d1 < (win >> 24);
      v0 = in0 ? (uint32_t)x[RR_VOFF] + 2 * d0 : 0;
      a0 = in0 ? a0 : (uint32_t)nparams;
      v1 = in1 ? (uint32_t)x[RR_VOFF + 1] + 2 * d1 : (x[RR_NAXES] >= 2 ? 0 : (uint32_t)x[RR_VOFF + 1]);
      a1 = in1 || x[RR_NAXES] < 2 ? a1 : (uint32_t)nparams;
    }
    const bool as_is = (uint32_t)gd[2 * e] == (v0 | (v1 << 16)) && (uint32_t)gd[2 * e + 1] == (a0 | (a1 << 16));
    const bool swapped = (uint32_t)gd[2 * e] == (v1 | (v0 << 16)) && (uint32_t)gd[2 * e + 1] == (a1 | (a0 << 16));
    if (!as_is && !swapped) return false;
  }
  // per thread, the second axis of at most one of its pieces: the same numbers as the
  // second half of that piece's descriptor
  const int64_t nfix = t.h(H_RS_NGFIX);
  if (nfix < 0 || nfix > RS_GDESC_THREADS) return false;
  if (nfix == 0) return true;
  if (!t.sec(H_OFF_RS_GFIX, RS_GDESC_THREADS * 2) || t.h(H_OFF_RS_GFIX) % 2) return false;
  const int32_t* gf = t.at(H_OFF_RS_GFIX);
  int64_t seen = 0;
  for (int64_t th = 0; th < RS_GDESC_THREADS; ++th) {
    const uint32_t v = (uint32_t)gf[2 * th], u = v >> 16, arrow = (uint32_t)gf[2 * th + 1];
    if (u == (uint32_t)RS_GFIX_NONE) {
      if ((v & 0xFFFF) != 0 || arrow != (uint32_t)nparams) return false;
      continue;
    }
    const int64_t e = th + (int64_t)u * RS_GDESC_THREADS;
    if (u >= (uint32_t)RS_GDESC_PIECES || e >= pieces || (v & 0xFFFF) != ((uint32_t)gd[2 * e] >> 16) ||
        arrow != ((uint32_t)gd[2 * e + 1] >> 16))
      return false;
    ++seen;
  }
  return seen == nfix;
}

// the CSC hand-off tables
bool check_resident_csc(const Tables& t) {
  if (t.h(H_CSC_PNNZ) == 0 && t.h(H_CSC_GNNZ) == 0) return true;
  const int64_t no = t.h(H_NO), nc = t.h(H_NC);
  const int64_t pn = t.h(H_CSC_PNNZ), gn = t.h(H_CSC_GNNZ), ldp = no + (no & 1);
  if (gn * nc > (1ll << 27)) return false;  // (far beyond what fits on chip)
  if (pn < 0 || gn < 0 || pn > no * no || gn > nc * no || (t.h(H_CSC_GSINGLE) & ~1) || !t.sec(H_OFF_CSC_P, pn) ||
      !t.sec(H_OFF_CSC_G, gn * 2) || t.h(H_OFF_CSC_G) % 2)
    return false;
  const int32_t* cp = t.at(H_OFF_CSC_P);
  for (int64_t k = 0; k < pn; ++k)
    if (cp[k] < 0 || cp[k] / ldp >= no || cp[k] % ldp >= no) return false;
  // an entry of G: the numbers of some row's record, its axes in either order, one column
  const int32_t* cg = t.at(H_OFF_CSC_G);
  const int32_t* rrw = t.at(H_OFF_RS_RR);
  for (int64_t k = 0; k < gn; ++k) {
    const uint32_t w0 = (uint32_t)cg[2 * k], w1 = (uint32_t)cg[2 * k + 1];
    bool found = false;
    for (int64_t R = 0; R < nc && !found; ++R) {
      const int32_t* x = rrw + R * RS_RR_WORDS;
      if (x[RR_NAXES] > 2) return false;
      for (int sw = 0; sw < 2 && !found; ++sw) {
        const uint32_t v0 = (uint32_t)x[RR_VOFF + sw], v1 = (uint32_t)x[RR_VOFF + 1 - sw];
        const uint32_t a0 = (uint32_t)x[RR_ARROW + sw], a1 = (uint32_t)x[RR_ARROW + 1 - sw];
        if (w1 != (a0 | (a1 << 16))) continue;
        const uint32_t c = (w0 & 0xFFFF) - v0;
        found = (w0 & 0xFFFF) >= v0 && c < (uint32_t)no && (w0 >> 16) == v1 + c && v1 + c < 65536;
      }
    }
    if (!found) return false;
  }
  return true;
}

// generated groups (loaded A, B and the tables), the input loads, the diagonal gterms on one column
bool check_resident_inputs(const Tables& t) {
  const int64_t ng = t.h(H_NG), no = t.h(H_NO), nparams = t.h(H_NPARAMS), nsrc = t.h(H_NSRC);
  const int64_t img = t.h(H_RS_IMG), dma = t.h(H_RS_IMG_DMA), nab = t.h(H_RS_AB);
  for (int64_t g = 0; g < t.h(H_RS_NLTI); ++g) {
    const int32_t* x = t.at(H_OFF_RS_LTI) + g * RS_LTI_WORDS;
    const int64_t gn = x[LT_N], gm = x[LT_M], gN = x[LT_HORIZON];
    if (gn < 1 || gm < 1 || gN < 1 || gn > 64 || gm > 64 || gN > 4096) return false;
    int stages = 0;
    while ((1ll << stages) < gN) ++stages;
    if (!in_range(x[LT_A], gn * gn, nab, 0) || !in_range(x[LT_B], gn * gm, nab, 0) ||
        !in_range(x[LT_TA], gN * gn * gn, img, dma) || !in_range(x[LT_TB], gN * gn * gm, img, dma) ||
        !in_range(x[LT_TP], (stages + 1) * gn * gn, img, dma))
      return false;
  }
  // every input load stays inside its stream: sources, given, params, the constants
  auto loads_ok = [&](const int32_t* im, int64_t lanes, int64_t bytes) {
    for (int64_t i = 0; i < lanes; ++i) {
      const int64_t st = im[2 * i], off = im[2 * i + 1];
      if (st < 0 || st > nsrc + 2 || off < 0 || off % bytes) return false;
      const int64_t lim = st < nsrc ? t.at(H_OFF_ARENA)[2 * st + 1] : st == nsrc ? ng : st == nsrc + 1 ? nparams : 4;
      if (off + bytes > lim * 8) return false;
    }
    return true;
  };
  if (!loads_ok(t.at(H_OFF_RS_INMETA), t.h(H_RS_NCHUNK) * 64, t.h(H_RS_UNIT)) ||
      !loads_ok(t.at(H_OFF_RS_ABMETA), nab * 2, 4))
    return false;
  for (int64_t c = 0; c < no; ++c) {  // diagonal gterms on one column: RS_DIAG_MAX slots
    int on = 0;
    for (int64_t g = 0; g < t.h(H_NGTERM); ++g) {
      const int32_t* r = t.at(H_OFF_GTERM) + g * GT_WORDS;
      const int64_t c0 = r[GT_AOFF], nr = r[GT_NROWS];
      if ((r[GT_FLAGS] & GT_FLAG_DIAG) && c >= c0 && c < c0 + nr) ++on;
    }
    if (on > RS_DIAG_MAX) return false;
  }
  return true;
}

bool check_resident(const Tables& t) {
  if (t.h(H_RS_OK) != 0 && t.h(H_RS_OK) != 1) return false;
  if (!t.h(H_RS_OK)) return true;
  return t.h(H_FUSED_OK) && check_resident_header(t) && check_resident_compose(t) && check_resident_trips(t) &&
         check_resident_rows(t) && check_resident_descriptors(t) && check_resident_csc(t) &&
         check_resident_inputs(t);
}

// ---- column tables (H_T_CI_OK): every stream and offset a kernel of tiled.hip or preview.hip derives from them
// stays inside its table -------------------------------------------------------------------------------------
bool check_column_tables(const Tables& t) {
  const int32_t* it = t.it;
  const int64_t ng = t.h(H_NG), no = t.h(H_NO), nbase = t.h(H_NBASE), nsrc = t.h(H_NSRC);
  const int64_t nop = t.h(H_T_NOP), ndelta = t.h(H_T_NDELTA), ddelta = t.h(H_T_DOFF_DELTA);
  if (nop < no || nop < T_BLOCK || nop % T_BLOCK || ndelta < 2 || !t.dsec(H_T_DOFF_DELTA, ndelta) ||
      t.dt[ddelta] != 0.0 || !t.sec(H_OFF_T_CIG, nbase * ng * 2) || !t.sec(H_OFF_T_CIO, nbase * nop * 2) ||
      t.h(H_OFF_T_CIO) % 4 || !t.sec(H_OFF_ARENA, nsrc * 2) || !t.sec(H_OFF_ENTBASE, t.h(H_NENT)) ||
      !t.sec(H_OFF_ENTK, t.h(H_NENT)) || !t.sec(H_OFF_PM_ENTBASE, t.h(H_PM_NENT)) ||
      !t.sec(H_OFF_PM_ENTK, t.h(H_PM_NENT)))
    return false;
  // generated groups: their sources are tables in the scratch
  const int64_t nlti = t.h(H_T_NLTI), twork = t.h(H_T_WORK), rtot = t.h(H_RTOT);
  if (nlti < 0 || nlti > RS_LTI_MAX || twork < rtot || !t.sec(H_OFF_T_LTI, nlti * T_LTI_WORDS)) return false;
  std::vector<int64_t> size(T_SID_CONST + 1, 0);
  for (int64_t sx = 0; sx < nsrc; ++sx) size[sx] = t.at(H_OFF_ARENA)[2 * sx + 1];
  size[T_SID_CONST] = t.nd;
  for (int64_t g = 0; g < nlti; ++g) {
    const int32_t* x = t.at(H_OFF_T_LTI) + g * T_LTI_WORDS;
    const int64_t gn = x[TL_N], gm = x[TL_M], gN = x[TL_HORIZON];
    if (gn < 1 || gm < 1 || gN < 1 || gn > 64 || gm > 64 || gN > 4096 ||
        !in_range(t.h(H_OFF_T_LTI_IDS) + x[TL_IDS], gm + 1, t.n, H_WORDS) || x[TL_IDS] < 0 ||
        !in_range(x[TL_TA], gN * gn * gn, twork, rtot) || !in_range(x[TL_TB], gn * gm * 2 * gN, twork, rtot))
      return false;
    const int32_t* ids = it + t.h(H_OFF_T_LTI_IDS) + x[TL_IDS];
    for (int64_t j = 0; j <= gm; ++j) {
      if (ids[j] < 0 || ids[j] >= nsrc) return false;
      size[ids[j]] = j < gm ? gn * gm * 2 * gN : gN * gn * gn;
    }
  }
  // rows of every base variable some program reads
  std::vector<int64_t> kmax(std::max<int64_t>(nbase, 1), 0);
  auto scan = [&](int off_word_b, int off_word_k, int64_t cnt) {
    for (int64_t e = 0; e < cnt; ++e) {
      const int64_t b = t.at(off_word_b)[e], k = t.at(off_word_k)[e];
      if (b < 0 || b >= nbase || k < 0) return false;
      kmax[b] = std::max(kmax[b], k);
    }
    return true;
  };
  if (!scan(H_OFF_ENTBASE, H_OFF_ENTK, t.h(H_NENT)) || !scan(H_OFF_PM_ENTBASE, H_OFF_PM_ENTK, t.h(H_PM_NENT)))
    return false;
  {  // first rows of the base variables: ascending, every row some program reads lies inside
    if (!t.sec(H_OFF_T_BROW0, nbase + 1)) return false;
    const int32_t* r0 = t.at(H_OFF_T_BROW0);
    if (r0[0] != 0) return false;
    for (int64_t b = 0; b < nbase; ++b)
      if (r0[b + 1] < r0[b] || (r0[b + 1] > r0[b] ? kmax[b] >= (int64_t)r0[b + 1] - r0[b] : kmax[b] != 0)) return false;
  }
  {  // the covered columns of every base variable: ascending ranges of one list, inside [0, ng + no)
    if (!t.sec(H_OFF_T_BCOLPTR, nbase + 1)) return false;
    const int32_t* cp = t.at(H_OFF_T_BCOLPTR);
    if (cp[0] != 0 || cp[nbase] < 0 || !t.sec(H_OFF_T_BCOLS, cp[nbase])) return false;
    const int32_t* cl = t.at(H_OFF_T_BCOLS);
    for (int64_t b = 0; b < nbase; ++b) {
      if (cp[b + 1] < cp[b] || cp[b + 1] > cp[nbase]) return false;
      for (int64_t i = cp[b]; i < cp[b + 1]; ++i)
        if (cl[i] < 0 || cl[i] >= ng + no || (i > cp[b] && cl[i] <= cl[i - 1])) return false;
    }
  }
  auto stream_ok = [&](int64_t sid) { return sid == T_SID_CONST || sid < nsrc; };
  auto inside = [&](int64_t sid, int64_t off) {  // an element offset inside its stream (the constants: the deltas)
    const int64_t lo = sid == T_SID_CONST ? ddelta : 0;
    const int64_t hi = sid == T_SID_CONST ? ddelta + ndelta : size[sid];
    return off >= lo && off < hi;
  };
  auto table_ok = [&](const int32_t* ci, int64_t cols) {
    for (int64_t b = 0; b < nbase; ++b)
      for (int64_t c = 0; c < cols; ++c) {
        const int64_t off = (uint32_t)ci[(b * cols + c) * 2];
        const int32_t meta = ci[(b * cols + c) * 2 + 1];
        const int64_t sid = (uint32_t)meta >> 24;
        if (!stream_ok(sid) || !inside(sid, off) || !inside(sid, off + kmax[b] * low24(meta))) return false;
      }
    return true;
  };
  if (!table_ok(t.at(H_OFF_T_CIG), ng) || !table_ok(t.at(H_OFF_T_CIO), nop)) return false;
  if (t.h(H_T_NP1) < 0) return t.h(H_T_NP1) == -1;
  // f2's unrolled tables: every entry inside its stream, every index inside its array
  const int64_t np1 = t.h(H_T_NP1), nbrow = t.at(H_OFF_T_BROW0)[nbase], pment = t.h(H_PM_NENT);
  if (!t.sec(H_OFF_T_P1PTR, nbrow + 1) || !t.sec(H_OFF_T_P1ENT, np1 * 2) || t.h(H_OFF_T_P1ENT) % 2 ||
      !t.sec(H_OFF_T_P2Y, pment))
    return false;
  const int32_t* pp = t.at(H_OFF_T_P1PTR);
  if (pp[0] != 0 || pp[nbrow] != np1) return false;
  for (int64_t r = 0; r < nbrow; ++r)
    if (pp[r + 1] < pp[r]) return false;
  const int32_t* pe = t.at(H_OFF_T_P1ENT);
  for (int64_t e = 0; e < np1; ++e) {
    const int64_t off = (uint32_t)pe[2 * e], sid = (uint32_t)pe[2 * e + 1] >> 24, c = pe[2 * e + 1] & 0xFFFFFF;
    if (!stream_ok(sid) || c >= ng + no || !inside(sid, off)) return false;
  }
  const int32_t* py = t.at(H_OFF_T_P2Y);
  for (int64_t e = 0; e < pment; ++e)
    if (py[e] < 0 || py[e] >= nbrow) return false;
  return true;
}

// ---- tiled program (H_T_OK): sections and stages.  g_written: the rows of G that ride on a stage -----------
bool check_tiled_stages(const Tables& t, std::vector<char>* g_written) {
  const int64_t no = t.h(H_NO), nc = t.h(H_NC), nbase = t.h(H_NBASE), nparams = t.h(H_NPARAMS);
  const int64_t nstage = t.h(H_T_NSTAGE), rtot = t.h(H_RTOT), nent = t.h(H_NENT), ngrest = t.h(H_T_NGREST);
  if (no < T_BLOCK || nstage < 0 || !t.sec(H_OFF_T_STAGE, nstage * T_STAGE_WORDS) || t.h(H_OFF_T_STAGE) % 4 ||
      !t.sec(H_OFF_T_GROW, nc * RS_AXMAX) || !t.sec(H_OFF_RS_RR, nc * RS_RR_WORDS) || !t.sec(H_OFF_ROWPTR, rtot + 1))
    return false;
  if (!diag_table_ok(t)) return false;
  if (!t.sec(H_OFF_T_SROW, nstage * 2 * 16) || !t.dsec(H_T_DOFF_SCOEF, nstage * 2 * 16) ||
      !t.sec(H_OFF_T_PIG, nstage * 16 * T_PIG_MAX * 2) || t.h(H_OFF_T_PIG) % 4 || ngrest < 0 || ngrest > nc ||
      !t.sec(H_OFF_T_GREST, ngrest))
    return false;
  const int32_t* rowptr = t.at(H_OFF_ROWPTR);
  const int32_t* entbase = t.at(H_OFF_ENTBASE);
  const int32_t* entk = t.at(H_OFF_ENTK);
  const int32_t* srow = t.at(H_OFF_T_SROW);
  const int32_t* pig = t.at(H_OFF_T_PIG);
  const int32_t* grow = t.at(H_OFF_T_GROW);
  const int32_t* rrw = t.at(H_OFF_RS_RR);
  int last_cls = 0;
  for (int64_t sx = 0; sx < nstage; ++sx) {
    const int32_t* x = t.at(H_OFF_T_STAGE) + sx * T_STAGE_WORDS;
    const int64_t arow = x[TS_AROW], brow = x[TS_BROW], drow = x[TS_DROW];
    const int rows = x[TS_INFO] & 255, fl = (x[TS_INFO] >> 8) & 255, cls = x[TS_INFO] >> 16;
    // sorted by class; class 0 exactly for the stages without a Hessian part
    if (x[TS_INFO] < 0 || cls < last_cls || cls > 4 || (cls > 0) != ((fl & TS_FLAG_P) != 0)) return false;
    last_cls = cls;
    // the class covers the masks: in every 64-column quarter only tiles 0 .. cls - 1
    if (fl & TS_FLAG_P)
      for (int side = 0; side < 2; ++side) {
        uint64_t m = ((uint64_t)(uint32_t)x[side ? TS_MASKB_HI : TS_MASKA_HI] << 32) |
                     (uint32_t)x[side ? TS_MASKB_LO : TS_MASKA_LO];
        if ((m >> 63) && cls < 4) return false;  // (folded tiles: anything)
        for (; m; m >>= 4)
          if ((m & 15u) >> cls) return false;
      }
    for (int side = 0; side < 2; ++side) {  // base rows of simple stages: the rows' own entries
      if (!(fl & (side ? TS_FLAG_SIMPLE_B : TS_FLAG_SIMPLE_A))) continue;
      const int64_t row0 = side ? brow : arow;
      if (row0 < 0 || row0 + rows > rtot) return false;
      for (int i = 0; i < 16; ++i) {
        const int k = srow[(sx * 2 + side) * 16 + i];
        if (i < rows ? (rowptr[row0 + i] < 0 || rowptr[row0 + i] >= nent || k != entk[rowptr[row0 + i]]) : k != 0)
          return false;
      }
    }
    for (int i = 0; i < 16; ++i)  // riding rows of G: one axis, this very workspace row, once
      for (int p = 0; p < T_PIG_MAX; ++p) {
        const int64_t R = pig[((sx * 16 + i) * T_PIG_MAX + p) * 2], slot = pig[((sx * 16 + i) * T_PIG_MAX + p) * 2 + 1];
        if (R == -1) continue;
        if (R < 0 || R >= nc || i >= rows || !(fl & TS_FLAG_G) || (*g_written)[R] ||
            rrw[R * RS_RR_WORDS + RR_NAXES] != 1 || grow[R * RS_AXMAX] != arow + i ||
            slot != rrw[R * RS_RR_WORDS + RR_ARROW])
          return false;
        (*g_written)[R] = 1;
      }
    if (rows < 1 || rows > 16 || (fl & ~127) || arow < 0 || arow + rows > rtot || brow < 0 || brow + rows > rtot ||
        drow < 0 || drow + rows > rtot || x[TS_WPARAM] < 0 || x[TS_WPARAM] >= nparams || x[TS_AIMPARAM] < 0 ||
        x[TS_AIMPARAM] >= nparams || ((fl & TS_FLAG_SAME) != 0) != (arow == brow))
      return false;
    // a stage flagged simple: one entry per row, all of the stated base
    for (int side = 0; side < 2; ++side) {
      if (!(fl & (side ? TS_FLAG_SIMPLE_B : TS_FLAG_SIMPLE_A))) continue;
      const int64_t row0 = side ? brow : arow;
      const int64_t base = side ? (int64_t)((uint32_t)x[TS_BASE] >> 16) : (x[TS_BASE] & 0xFFFF);
      if (base >= nbase) return false;
      for (int64_t r = row0; r < row0 + rows; ++r)
        if ((int64_t)rowptr[r + 1] - rowptr[r] != 1 || rowptr[r] < 0 || rowptr[r] >= nent ||
            entbase[rowptr[r]] != base)
          return false;
    }
  }
  return true;
}

// ---- Toeplitz form: all stages or none; one generated group; every stage's rows are consecutive rows of one
// of its states with one coefficient, and -- what lets the kernel keep ONE set of per-lane column offsets -- a
// column's table offset less the state's own part is the same for every state, inside the group's TB table
// together with the window -------------------------------------------------------------------------------
bool check_toeplitz(const Tables& t) {
  const int64_t nstage = t.h(H_T_NSTAGE), nbase = t.h(H_NBASE), nop = t.h(H_T_NOP);
  if (t.h(H_T_TOEPLITZ) & ~1) return false;
  if (!t.h(H_T_TOEPLITZ)) return true;
  int64_t ntoep = 0;
  for (int64_t sx = 0; sx < nstage; ++sx)
    ntoep += ((t.at(H_OFF_T_STAGE) + sx * T_STAGE_WORDS)[TS_INFO] >> 8) & TS_FLAG_TOEPLITZ ? 1 : 0;
  if (ntoep != nstage || nstage == 0 || t.h(H_T_NLTI) != 1) return false;
  const int32_t* g = t.at(H_OFF_T_LTI);
  const int64_t gn = g[TL_N], gm = g[TL_M], gN = g[TL_HORIZON], tbn = gn * gm * 2 * gN;
  const int32_t* ids = t.it + t.h(H_OFF_T_LTI_IDS) + g[TL_IDS];
  const double* sc = t.dt + t.h(H_T_DOFF_SCOEF);
  const int32_t* srow = t.at(H_OFF_T_SROW);
  const int32_t* cio = t.at(H_OFF_T_CIO);
  const int32_t* x0 = t.at(H_OFF_T_STAGE);
  const int64_t base0 = x0[TS_BASE] & 0xFFFF, sb0 = x0[TS_SBOFFA];
  // (a stage's window of TK rows may start up to TK - 1 rows before the horizon's end: what it reads behind the
  // last row of the table are the zeros the kernel itself keeps there, toeplitz_zero_pad of them -- held to 16,
  // a stage that starts at row 32 of a horizon of 33 or 34 was refused as malformed)
  if (base0 >= nbase) return false;
  auto is_u = [&](int64_t sid) {
    for (int64_t j = 0; j < gm; ++j)
      if (ids[j] == sid) return true;
    return false;
  };
  for (int64_t sx = 0; sx < nstage; ++sx) {
    const int32_t* x = t.at(H_OFF_T_STAGE) + sx * T_STAGE_WORDS;
    const int rows = x[TS_INFO] & 255, fl = (x[TS_INFO] >> 8) & 255;
    for (int side = 0; side < ((fl & TS_FLAG_P) ? 2 : 1); ++side) {
      if (!(fl & (side ? TS_FLAG_SIMPLE_B : TS_FLAG_SIMPLE_A))) return false;
      const int64_t base = side ? (int64_t)((uint32_t)x[TS_BASE] >> 16) : (x[TS_BASE] & 0xFFFF);
      const int64_t sb = x[side ? TS_SBOFFB : TS_SBOFFA], U = x[side ? TS_UB : TS_UA];
      const int32_t* ks = srow + (sx * 2 + side) * 16;
      if (base >= nbase || sb < 0 || sb % (gm * 2 * gN) || sb / (gm * 2 * gN) >= gn || U != sb + ks[0]) return false;
      for (int i = 0; i < rows; ++i)
        if (ks[i] != (int64_t)ks[0] + i || sc[(sx * 2 + side) * 16 + i] != sc[(sx * 2 + side) * 16]) return false;
      for (int64_t c = 0; c < nop; ++c) {
        const int32_t* e = cio + (base * nop + c) * 2;
        const int32_t* e0 = cio + (base0 * nop + c) * 2;
        const int64_t sid = (uint32_t)e[1] >> 24, sid0 = (uint32_t)e0[1] >> 24;
        const bool valid = sid != T_SID_CONST;
        if (valid != (sid0 != T_SID_CONST)) return false;
        if (!valid) continue;
        const int64_t part = (int64_t)(uint32_t)e[0] - sb;
        if (!is_u(sid) || low24(e[1]) != 1 || part != (int64_t)(uint32_t)e0[0] - sb0 || part + U < 0 ||
            part + U + 15 + 3 >= tbn + toeplitz_zero_pad((int)gN))
          return false;
      }
    }
  }
  return true;
}

// ---- scan form (toeplitz_scan_kernel): only beside the Toeplitz form; every index the kernel forms from these
// tables stays inside TB, d, the parameters and the results ------------------------------------------------
bool check_scan(const Tables& t) {
  const int64_t no = t.h(H_NO), nc = t.h(H_NC), nparams = t.h(H_NPARAMS), rtot = t.h(H_RTOT);
  const int64_t K = t.h(H_T_SCAN), nblk = t.h(H_T_SCAN_NBLK), nrest = t.h(H_T_SCAN_NGREST);
  if (K < 0 || K > T_SCAN_KMAX || (K > 0 && !t.h(H_T_TOEPLITZ))) return false;
  if (K == 0) return t.h(H_T_SCAN_FUSED) == 0;
  const int32_t* g = t.at(H_OFF_T_LTI);
  const int64_t gn = g[TL_N], gm = g[TL_M], gN = g[TL_HORIZON], per_state = gm * gN;
  if (gN < 1 || gN > T_SCAN_NMAX || nblk < 1 || nblk > T_SCAN_BLKMAX || nrest < 0 || nrest > nc ||
      !t.sec(H_OFF_T_SCAN_BLK, nblk * 2) || !t.sec(H_OFF_T_SCAN_GT, K * T_SCAN_GT_WORDS) ||
      !t.sec(H_OFF_T_SCAN_GROW, nc * 2) || t.h(H_OFF_T_SCAN_GROW) % 2 || !t.sec(H_OFF_T_SCAN_GREST, nrest) ||
      !t.sec(H_OFF_T_SCAN_COLBLK, no) || !t.dsec(H_T_DOFF_SCAN_GC, K) || !t.dsec(H_T_DOFF_SCAN_GCOEF, nc))
    return false;
  const int32_t* blk = t.at(H_OFF_T_SCAN_BLK);
  const int32_t* colblk = t.at(H_OFF_T_SCAN_COLBLK);
  int64_t covered = 0;
  for (int64_t b = 0; b < nblk; ++b) {
    const int64_t c0 = blk[2 * b], pbase = blk[2 * b + 1];
    if (c0 < 0 || c0 + gN > no || pbase < 0 || pbase % gN || pbase / gN >= gm) return false;
    for (int64_t l = 0; l < gN; ++l)
      if (colblk[c0 + l] != b) return false;  // (hence disjoint)
    covered += gN;
  }
  int64_t other = 0;
  for (int64_t c = 0; c < no; ++c) {
    if (colblk[c] < -1 || colblk[c] >= nblk) return false;
    other += colblk[c] < 0;
  }
  if (other != t.h(H_T_SCAN_NOTHER) || covered + other != no) return false;
  const int32_t* gt = t.at(H_OFF_T_SCAN_GT);
  for (int64_t k = 0; k < K; ++k) {
    const int32_t* x = gt + k * T_SCAN_GT_WORDS;
    if (x[SG_SBOFF] < 0 || x[SG_SBOFF] % per_state || x[SG_SBOFF] / per_state >= gn || x[SG_WPARAM] < 0 ||
        x[SG_WPARAM] >= nparams || x[SG_AIMPARAM] < 0 || x[SG_AIMPARAM] >= nparams || x[SG_DROW] < 0 ||
        x[SG_DROW] + gN > rtot)
      return false;
  }
  const int32_t* sg = t.at(H_OFF_T_SCAN_GROW);
  const int32_t* rest = t.at(H_OFF_T_SCAN_GREST);
  const int32_t* rrw = t.at(H_OFF_RS_RR);
  int64_t r = 0;
  for (int64_t R = 0; R < nc; ++R) {
    const int64_t u = sg[2 * R], slot = sg[2 * R + 1];
    if (u == -1) {
      if (slot != -1 || r >= nrest || rest[r] != R) return false;
      ++r;
      continue;
    }
    if (u < 0 || u / per_state >= gn || u % per_state >= gN || slot < 0 || slot >= nparams ||
        rrw[R * RS_RR_WORDS + RR_NAXES] != 1 || rrw[R * RS_RR_WORDS + RR_ARROW] != slot)
      return false;
  }
  if (r != nrest) return false;
  // fused set-up: `given` is the initial state, the K terms' rows tile the workspace (the kernel writes
  // d[first row + k] for every term and reads nothing else), no row of G through the column tables,
  // every input an unknown
  if (t.h(H_T_SCAN_FUSED) == 0) return true;
  if (t.h(H_T_SCAN_FUSED) != 1 || t.h(H_NG) != gn || nrest != 0 || rtot != K * gN || nblk != gm) return false;
  std::vector<char> seen((size_t)K, 0);
  for (int64_t k = 0; k < K; ++k) {
    const int64_t dr = gt[k * T_SCAN_GT_WORDS + SG_DROW];
    if (dr % gN || seen[(size_t)(dr / gN)]) return false;
    seen[(size_t)(dr / gN)] = 1;
  }
  return true;
}

// every row of G is written exactly once -- riding on a stage or listed in the rest -- and its record names
// workspace rows and parameters that exist
bool check_tiled_rows(const Tables& t, std::vector<char>* g_written) {
  const int64_t nc = t.h(H_NC), nparams = t.h(H_NPARAMS), rtot = t.h(H_RTOT);
  const int32_t* grest = t.at(H_OFF_T_GREST);
  for (int64_t i = 0; i < t.h(H_T_NGREST); ++i) {
    if (grest[i] < 0 || grest[i] >= nc || (*g_written)[grest[i]]) return false;
    (*g_written)[grest[i]] = 1;
  }
  for (int64_t R = 0; R < nc; ++R)
    if (!(*g_written)[R]) return false;
  const int32_t* grow = t.at(H_OFF_T_GROW);
  for (int64_t R = 0; R < nc; ++R) {
    const int32_t* x = t.at(H_OFF_RS_RR) + R * RS_RR_WORDS;
    if (!row_record_slots_ok(x, nparams)) return false;
    for (int a = 0; a < RS_AXMAX; ++a) {
      const int64_t row = grow[R * RS_AXMAX + a];
      if (a < x[RR_NAXES] ? (row < 0 || row >= rtot) : row != -1) return false;
      if (a < x[RR_NAXES] && (x[RR_ARROW + a] >= nparams || x[RR_CENTER + a] >= nparams)) return false;
    }
  }
  return true;
}

// the column tables (H_T_CI_OK) and the tiled program (H_T_OK)
bool check_tiled(const Tables& t) {
  if ((t.h(H_T_CI_OK) & ~1) || (t.h(H_T_OK) & ~1)) return false;
  if (!t.h(H_T_CI_OK)) return !t.h(H_T_OK);
  if (!check_column_tables(t)) return false;
  if (!t.h(H_T_OK)) return true;
  std::vector<char> g_written(std::max<int64_t>(t.h(H_NC), 1), 0);
  return check_tiled_stages(t, &g_written) && check_toeplitz(t) && check_scan(t) && check_tiled_rows(t, &g_written);
}

// ---- the sweep kernel's tables (H_SW_OK): every column, parameter slot, step and combination it reads ------
// the per-step lists say what the records say: every cost row and every line once, at its step
bool check_sweep_steps(const Tables& t) {
  const int64_t N = t.h(H_SW_HORIZON), nc = t.h(H_NC), nterm = t.h(H_SW_NTERM), nlim = t.h(H_SW_NLIM);
  const int64_t ncent = t.h(H_SW_NCENT), ngent = t.h(H_SW_NGENT);
  constexpr int64_t LIMW = SW_LIM_WORDS + SW_AXMAX * SW_LAX_WORDS;
  if (ncent < 0 || ngent != nc || !t.sec(H_OFF_SW_CPTR, N + 1) || !t.sec(H_OFF_SW_CENT, ncent) ||
      !t.sec(H_OFF_SW_GPTR, N + 1) || !t.sec(H_OFF_SW_GENT, ngent * 2))
    return false;
  const int32_t* cptr = t.at(H_OFF_SW_CPTR);
  const int32_t* cent = t.at(H_OFF_SW_CENT);
  const int32_t* gptr = t.at(H_OFF_SW_GPTR);
  const int32_t* gent = t.at(H_OFF_SW_GENT);
  if (cptr[0] != 0 || cptr[N] != ncent || gptr[0] != 0 || gptr[N] != ngent) return false;
  std::vector<int64_t> rows(std::max<int64_t>(nterm, 1), 0);
  std::vector<char> line(std::max<int64_t>(nc, 1), 0);
  for (int64_t l = 0; l < N; ++l) {
    if (cptr[l + 1] < cptr[l] || cptr[l + 1] > ncent || gptr[l + 1] < gptr[l] || gptr[l + 1] > ngent) return false;
    for (int64_t e = cptr[l]; e < cptr[l + 1]; ++e) {
      const int64_t ti = cent[e];
      if (ti < 0 || ti >= nterm) return false;
      const int32_t* x = t.at(H_OFF_SW_TERM) + ti * SW_TERM_WORDS;
      const int64_t ks = x[ST_KSTEP], dk = l - x[ST_K0];
      ++rows[ti];
      if (ks == 0 ? dk != 0 : (dk % ks != 0 || dk / ks < 0 || dk / ks >= x[ST_COUNT])) return false;
    }
    for (int64_t e = gptr[l]; e < gptr[l + 1]; ++e) {
      const int64_t li = gent[2 * e], i = gent[2 * e + 1];
      if (li < 0 || li >= nlim) return false;
      const int32_t* x = t.at(H_OFF_SW_LIM) + li * LIMW;
      if (i < 0 || i >= x[SL_COUNT] || x[SW_LIM_WORDS + SX_K0] + i * x[SW_LIM_WORDS + SX_KSTEP] != l ||
          line[x[SL_OUT0] + i])
        return false;
      line[x[SL_OUT0] + i] = 1;
    }
  }
  for (int64_t k = 0; k < nterm; ++k)
    if (rows[k] != (t.at(H_OFF_SW_TERM) + k * SW_TERM_WORDS)[ST_COUNT]) return false;
  return true;
}

bool check_sweep(const Tables& t) {
  if (t.h(H_SW_OK) & ~1) return false;
  if (!t.h(H_SW_OK)) return true;
  const int64_t sn = t.h(H_SW_N), sm = t.h(H_SW_M), N = t.h(H_SW_HORIZON), naxes = t.h(H_SW_NAXES);
  const int64_t ng = t.h(H_NG), no = t.h(H_NO), nc = t.h(H_NC), nparams = t.h(H_NPARAMS), nsrc = t.h(H_NSRC);
  const int64_t nterm = t.h(H_SW_NTERM), nlim = t.h(H_SW_NLIM), ncv = t.h(H_SW_NCVEC);
  constexpr int64_t LIMW = SW_LIM_WORDS + SW_AXMAX * SW_LAX_WORDS;
  if (sn < 1 || sn > SW_NMAX || sm < 1 || sm > SW_MMAX || N < 1 || N > 32767 || naxes < 1 || naxes > SW_AXMAX ||
      t.h(H_SW_SRC_A) < 0 || t.h(H_SW_SRC_A) >= nsrc || t.h(H_SW_SRC_B) < 0 || t.h(H_SW_SRC_B) >= nsrc ||
      t.h(H_SW_SRC_A) == t.h(H_SW_SRC_B) || nterm < 0 || nlim < 0 || ncv < 0 ||
      !t.sec(H_OFF_SW_AXIS, naxes * SW_AXIS_WORDS) || !t.sec(H_OFF_SW_TERM, nterm * SW_TERM_WORDS) ||
      !t.sec(H_OFF_SW_LIM, nlim * LIMW) || !t.sec(H_OFF_SW_COL, no) || !t.dsec(H_SW_DOFF_CVEC, ncv * SW_NMAX) ||
      !diag_table_ok(t))
    return false;
  const int32_t* ax = t.at(H_OFF_SW_AXIS);
  const int32_t* col = t.at(H_OFF_SW_COL);
  std::vector<char> seen(std::max<int64_t>(no, 1), 0);
  for (int64_t a = 0; a < naxes; ++a) {
    if (ax[a * SW_AXIS_WORDS] < 0 || ax[a * SW_AXIS_WORDS] + sn > ng) return false;
    for (int64_t j = 0; j < sm; ++j) {
      const int64_t c0 = ax[a * SW_AXIS_WORDS + 1 + j];
      if (c0 < 0 || c0 + N > no) return false;
      for (int64_t l = 0; l < N; ++l) {
        if (seen[c0 + l] || col[c0 + l] != (int32_t)(a | (j << 8) | (l << 16))) return false;
        seen[c0 + l] = 1;
      }
    }
  }
  for (int64_t c = 0; c < no; ++c)
    if (!seen[c]) return false;  // every unknown is an input of the system
  auto steps_ok = [&](int64_t k0, int64_t ks, int64_t cnt) {
    return cnt >= 1 && k0 >= 0 && k0 < N && k0 + (cnt - 1) * ks >= 0 && k0 + (cnt - 1) * ks < N;
  };
  auto slot_ok = [&](int64_t slot, int64_t step, int64_t cnt) {
    return slot >= 0 && step >= 0 && slot + (cnt - 1) * step < nparams;
  };
  auto cvec_ok = [&](int64_t cv) { return cv >= 0 && cv % SW_NMAX == 0 && cv / SW_NMAX < ncv; };
  const int32_t* tr = t.at(H_OFF_SW_TERM);
  for (int64_t k = 0; k < nterm; ++k, tr += SW_TERM_WORDS)
    if (tr[ST_AXIS] < 0 || tr[ST_AXIS] >= naxes || !steps_ok(tr[ST_K0], tr[ST_KSTEP], tr[ST_COUNT]) ||
        tr[ST_KSTEP] < 0 ||  // (the kernel walks a term's steps downwards from its last)
        tr[ST_WPARAM] < 0 || tr[ST_WPARAM] >= nparams || tr[ST_AIMPARAM] < 0 || tr[ST_AIMPARAM] >= nparams ||
        !cvec_ok(tr[ST_CVEC]))
      return false;
  std::vector<char> line(std::max<int64_t>(nc, 1), 0);
  const int32_t* lm = t.at(H_OFF_SW_LIM);
  for (int64_t k = 0; k < nlim; ++k, lm += LIMW) {
    const int64_t out0 = lm[SL_OUT0], cnt = lm[SL_COUNT], nax = lm[SL_NAXES];
    if (out0 < 0 || cnt < 1 || out0 + cnt > nc || nax < 1 || nax > SW_AXMAX ||
        !slot_ok(lm[SL_EXTREME], lm[SL_EXTREME_STEP], cnt))
      return false;
    for (int64_t i = 0; i < cnt; ++i) {
      if (line[out0 + i]) return false;
      line[out0 + i] = 1;
    }
    const int32_t* x0 = lm + SW_LIM_WORDS;
    for (int64_t a = 0; a < nax; ++a) {
      const int32_t* x = x0 + a * SW_LAX_WORDS;
      if (x[SX_AXIS] < 0 || x[SX_AXIS] >= naxes || !steps_ok(x[SX_K0], x[SX_KSTEP], cnt) ||
          x[SX_K0] != x0[SX_K0] || x[SX_KSTEP] != x0[SX_KSTEP] ||  // (a line's axes: one step)
          !cvec_ok(x[SX_CVEC]) || !slot_ok(x[SX_ARROW], x[SX_ARROW_STEP], cnt) ||
          !slot_ok(x[SX_CENTER], x[SX_CENTER_STEP], cnt))
        return false;
    }
  }
  for (int64_t R = 0; R < nc; ++R)
    if (!line[R]) return false;  // every line of G, h is written
  return check_sweep_steps(t);
}

// ---- content checks: every index a kernel dereferences stays inside its table -----------------------------
bool check_segments_and_rows(const Tables& t) {
  const int64_t W = t.h(H_NG) + t.h(H_NO), nsrc = t.h(H_NSRC), nseg = t.h(H_NSEG), nbase = t.h(H_NBASE);
  const int32_t* seg = t.at(H_OFF_SEG);
  for (int64_t s = 0; s < nseg; ++s) {
    const int32_t* r = seg + s * SEG_WORDS;
    const int64_t dst0 = r[SEG_DST0], len = r[SEG_LEN];
    if (r[SEG_KIND] != SEG_KIND_GATHER && r[SEG_KIND] != SEG_KIND_IDENTITY) return false;
    if (r[SEG_KIND] == SEG_KIND_GATHER && (r[SEG_SRC] < 0 || r[SEG_SRC] >= nsrc)) return false;
    if (dst0 < 0 || len < 0 || dst0 + len > W) return false;
  }
  const int32_t* colseg = t.at(H_OFF_COLSEG);
  for (int64_t i = 0; i < nbase * W; ++i)
    if (colseg[i] < -1 || colseg[i] >= nseg) return false;
  auto check_csr = [&](int ptr_word, int64_t rows, int base_word, int64_t nent) {
    const int32_t* rp = t.at(ptr_word);
    if (rp[0] != 0 || rp[rows] != nent) return false;
    for (int64_t r = 0; r < rows; ++r)
      if (rp[r + 1] < rp[r]) return false;
    const int32_t* eb = t.at(base_word);
    for (int64_t e = 0; e < nent; ++e)
      if (eb[e] < 0 || eb[e] >= nbase) return false;
    return true;
  };
  return check_csr(H_OFF_ROWPTR, t.h(H_RTOT), H_OFF_ENTBASE, t.h(H_NENT)) &&
         check_csr(H_OFF_PM_ROWPTR, t.h(H_PMROWS), H_OFF_PM_ENTBASE, t.h(H_PM_NENT));
}

bool check_gterms(const Tables& t) {
  const int64_t no = t.h(H_NO), nparams = t.h(H_NPARAMS), rtot = t.h(H_RTOT);
  const int32_t* gt = t.at(H_OFF_GTERM);
  for (int64_t g = 0; g < t.h(H_NGTERM); ++g) {
    const int32_t* r = gt + g * GT_WORDS;
    const int64_t nr = r[GT_NROWS], aoff = r[GT_AOFF], boff = r[GT_BOFF], doff = r[GT_DOFF];
    if (r[GT_WPARAM] < 0 || r[GT_WPARAM] >= nparams) return false;
    if (r[GT_AIMPARAM] < 0 || r[GT_AIMPARAM] >= nparams) return false;
    if (r[GT_FLAGS] & GT_FLAG_DIAG) {  // columns c0 .. c0+nr-1 of the unknowns, coefficient list
      if ((r[GT_FLAGS] & GT_FLAG_P) || nr < 0 || aoff < 0 || aoff + nr > no || boff < 0 ||
          boff + nr > t.h(H_NDIAGCOEF))
        return false;
      continue;
    }
    if (nr < 0 || aoff < 0 || aoff + nr > rtot) return false;
    if (doff < 0 || doff + nr > rtot) return false;
    if ((r[GT_FLAGS] & GT_FLAG_P) && (boff < 0 || boff + nr > rtot)) return false;
  }
  return true;
}

bool check_limits(const Tables& t) {
  const int64_t nc = t.h(H_NC), nparams = t.h(H_NPARAMS), rtot = t.h(H_RTOT), nlax = t.h(H_NLAX);
  const int32_t* lim = t.at(H_OFF_LIMIT);
  const int32_t* lax = t.at(H_OFF_LAX);
  const int32_t* rowlimit = t.at(H_OFF_ROWLIMIT);
  for (int64_t l = 0; l < t.h(H_NLIMIT); ++l) {
    const int32_t* r = lim + l * LM_WORDS;
    const int64_t out0 = r[LM_OUT0], nr = r[LM_NROWS], na = r[LM_NAXES], lax0 = r[LM_LAX0];
    if (nr < 0 || na < 0 || out0 < 0 || out0 + nr > nc) return false;
    if (lax0 < 0 || lax0 + na > nlax) return false;
    const int64_t ar = r[LM_ARROW_ROWS], cr = r[LM_CENTER_ROWS], er = r[LM_EXTREME_ROWS];
    if ((ar != 1 && ar != nr) || (cr != 1 && cr != nr) || (er != 1 && er != nr)) return false;
    if (r[LM_ARROW_P] < 0 || r[LM_ARROW_P] + ar * na > nparams) return false;
    if (r[LM_CENTER_P] < 0 || r[LM_CENTER_P] + cr * na > nparams) return false;
    if (r[LM_EXTREME_P] < 0 || r[LM_EXTREME_P] + er > nparams) return false;
    for (int64_t a = 0; a < na; ++a) {
      const int32_t* x = lax + (lax0 + a) * LX_WORDS;
      const int64_t rows = x[LX_ROWS], rowoff = x[LX_ROWOFF];
      if ((rows != 1 && rows != nr) || rowoff < 0 || rowoff + rows > rtot) return false;
    }
    for (int64_t k = 0; k < nr; ++k)
      if (rowlimit[out0 + k] != l) return false;
  }
  return true;
}

}  // namespace

int validate_plan(const int32_t* it, const double* h_dtab, size_t n_itab, size_t n_dtab) {
  const int rc = check_header(it, n_itab, n_dtab);
  if (rc != MPCASM_OK) return rc;
  const Tables t = {it, h_dtab, (int64_t)n_itab, (int64_t)n_dtab};
  const bool ok = check_sections(t) && check_fused(t) && check_preview_program(t) && check_resident(t) &&
                  check_tiled(t) && check_sweep(t) && check_segments_and_rows(t) && check_gterms(t) &&
                  check_limits(t);
  return ok ? MPCASM_OK : MPCASM_ERR_PLAN;
}

void plan_view(const int32_t* it, PlanDev* out) {
  PlanDev& d = *out;
  // the fields that are header words, from the field list; the derived ones below
#define MPCASM_COPY(f, W) d.f = it[H_##W];
#define MPCASM_DERIVED(f)
  MPCASM_PLAN_INT_FIELDS(MPCASM_COPY, MPCASM_DERIVED)
#undef MPCASM_COPY
#undef MPCASM_DERIVED
  d.t_nbrow = d.t_ci_ok ? it[d.off_t_brow0 + d.nbase] : 0;
  d.rs_src16 = 0;
  if (d.rs_ok && d.rs_unit == 16)
    for (int64_t i = 0; i < (int64_t)d.rs_nchunk * 64; ++i) {
      const int st = it[d.off_rs_inmeta + 2 * i];
      if (st < d.nsrc) d.rs_src16 |= 1u << st;
    }
  d.ndiag = 0;
  d.rs_sym_any = 1;
  for (int g = 0; g < it[H_NGTERM]; ++g) {
    const int32_t* r = it + it[H_OFF_GTERM] + g * GT_WORDS;
    if (r[GT_FLAGS] & GT_FLAG_DIAG) ++d.ndiag;
    if ((r[GT_FLAGS] & GT_FLAG_P) && r[GT_AOFF] != r[GT_BOFF]) d.rs_sym_any = 0;
  }
  // the per-column table of the diagonal gterms holds them all when no column carries more than
  // RS_DIAG_MAX (its sections are laid out for every plan)
  d.rs_diag_table = 1;
  {
    std::vector<int> on(std::max(d.no, 1), 0);
    for (int g = 0; g < it[H_NGTERM]; ++g) {
      const int32_t* r = it + it[H_OFF_GTERM] + g * GT_WORDS;
      if (!(r[GT_FLAGS] & GT_FLAG_DIAG)) continue;
      for (int k = 0; k < r[GT_NROWS]; ++k)
        if (++on[r[GT_AOFF] + k] > RS_DIAG_MAX) d.rs_diag_table = 0;
    }
    if (it[H_OFF_RS_DPAR] % 4 || it[H_DOFF_RS_DCOEF] % 2) d.rs_diag_table = 0;
  }
  d.max_axes = 0;
  for (int l = 0; l < it[H_NLIMIT]; ++l) {
    const int na = it[it[H_OFF_LIMIT] + l * LM_WORDS + LM_NAXES];
    if (na > d.max_axes) d.max_axes = na;
  }
  // the op table is read as int2: keep its word offset even (the compiler pads it)
  if (d.fused_ok && (d.off_op & 1)) d.fused_ok = 0;
}

}  // namespace mpcasm
