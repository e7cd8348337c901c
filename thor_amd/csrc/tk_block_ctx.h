// tk_block_ctx.h - neighbour context of a coding block: availability, get_mv_pred, get_mv_cands, find_contexts.
#pragma once
#include "tk_block_ws.h"

namespace tk {
// ---------------------------------------------------------------------------------
// availability (common_block.h:52-95)
// ---------------------------------------------------------------------------------
TK_DEV int upright_avail(int ypos, int xpos, int bw, int bh, int fw, int sb) {
  int a = (ypos > 0) && (xpos + bw < fw);
  int size = bw > bh ? bw : bh;
  for (int s2 = size; s2 < sb; s2 *= 2)
    if ((ypos % (s2 << 1)) == s2 && (xpos % s2) == (s2 - size)) a = 0;
  return a;
}
TK_DEV int downleft_avail(int ypos, int xpos, int bw, int bh, int fh, int sb) {
  int a = (xpos > 0) && (ypos + bh < fh);
  int size = bw > bh ? bw : bh;
  if ((ypos % sb) == (sb - size) && (xpos % sb) == 0) a = 0;
  for (int s2 = 2 * size; s2 <= sb; s2 *= 2)
    if ((ypos % s2) == (s2 - size) && (xpos % s2) > 0) a = 0;
  return a;
}

TK_DEV InterPred zero_pred() {
  InterPred z;
  z.mv0 = mk_mv(0, 0);
  z.mv1 = mk_mv(0, 0);
  z.ref0 = z.ref1 = 0;
  z.dir = 0;
  z.pad = 0;
  return z;
}
TK_DEV InterPred cell_pred(const DbCell& c) {
  InterPred p;
  p.mv0 = c.mv0;
  p.mv1 = c.mv1;
  p.ref0 = c.ref0;
  p.ref1 = c.ref1;
  p.dir = c.dir;
  p.pad = 0;
  return p;
}

// get_mv_pred (inter_prediction.c:413-526): median of three neighbours' mv0.
TK_DEV mv_t get_mv_pred(const DbCell* cells, int cs, int ypos, int xpos, int fw, int fh, int size, int sb) {
  const int bsz = size / kMinPb;
  const int bi = (ypos / kMinPb) * cs + xpos / kMinPb;
  const int up0 = bi - cs, up1 = bi - cs + (bsz - 1) / 2, up2 = bi - cs + bsz - 1;
  const int l0 = bi - 1, l1 = bi + cs * ((bsz - 1) / 2) - 1, l2 = bi + cs * (bsz - 1) - 1;
  const int dl = bi + cs * bsz - 1, ur = bi - cs + bsz, ul = bi - cs - 1;
  const int U = ypos > 0, L = xpos > 0;
  const int UR = upright_avail(ypos, xpos, size, size, fw, sb);
  const int DL = downleft_avail(ypos, xpos, size, size, fh, sb);
  mv_t a = mk_mv(0, 0), b = a, c = a;
  if (U == 0 && UR == 0 && L == 0 && DL == 0) {
  } else if (U == 1 && UR == 0 && L == 0 && DL == 0) { a = cells[up0].mv0; b = cells[up1].mv0; c = cells[up2].mv0; }
  else if (U == 1 && UR == 1 && L == 0 && DL == 0) { a = cells[up0].mv0; b = cells[up2].mv0; c = cells[ur].mv0; }
  else if (U == 0 && UR == 0 && L == 1 && DL == 0) { a = cells[l0].mv0; b = cells[l1].mv0; c = cells[l2].mv0; }
  else if (U == 1 && UR == 0 && L == 1 && DL == 0) { a = cells[ul].mv0; b = cells[up2].mv0; c = cells[l2].mv0; }
  else if (U == 1 && UR == 1 && L == 1 && DL == 0) { a = cells[up0].mv0; b = cells[ur].mv0; c = cells[l2].mv0; }
  else if (U == 0 && UR == 0 && L == 1 && DL == 1) { a = cells[l0].mv0; b = cells[l2].mv0; c = cells[dl].mv0; }
  else if (U == 1 && UR == 0 && L == 1 && DL == 1) { a = cells[up2].mv0; b = cells[l0].mv0; c = cells[dl].mv0; }
  else if (U == 1 && UR == 1 && L == 1 && DL == 1) { a = cells[up0].mv0; b = cells[ur].mv0; c = cells[l0].mv0; }
  mv_t p;
  p.x = a.x < b.x ? tmin(b.x, tmax(a.x, c.x)) : tmin(a.x, tmax(b.x, c.x));
  p.y = a.y < b.y ? tmin(b.y, tmax(a.y, c.y)) : tmin(a.y, tmax(b.y, c.y));
  return p;
}

// get_mv_skip / get_mv_merge (LIMITED_SKIP variant; inter_prediction.c:528-834): identical rules.
TK_DEV int get_mv_cands(const DbCell* cells, int cs, int ypos, int xpos, int fw, int fh, int size, int sb,
                        InterPred* out) {
  const int bsz = size / kMinPb;
  const int bi = (ypos / kMinPb) * cs + xpos / kMinPb;
  int up0 = bi - cs, up2 = bi - cs + bsz - 1;
  int l0 = bi - 1, l2 = bi + cs * (bsz - 1) - 1;
  const int ur = bi - cs + bsz;
  const int U = ypos > 0, L = xpos > 0;
  const int UR = upright_avail(ypos, xpos, size, size, fw, sb);
  if (ypos + size > fh) l2 = l0;
  if (xpos + size > fw) up2 = up0;
  InterPred tmp[2];
  tmp[0] = L ? cell_pred(cells[l2]) : zero_pred();
  tmp[1] = UR ? cell_pred(cells[ur]) : (U ? cell_pred(cells[up2]) : zero_pred());
  out[0] = tmp[0];
  int n = 1;
  // duplicate test (inter_prediction.c:816-826); dir == -1 plays the reference's (uint32)-1
  const InterPred& q = tmp[1];
  const InterPred& o = out[0];
  int dup = q.mv0.x == o.mv0.x && q.mv0.y == o.mv0.y && q.ref0 == o.ref0 && q.mv1.x == o.mv1.x &&
            q.mv1.y == o.mv1.y && q.ref1 == o.ref1 && (q.dir == o.dir || q.dir == -1);
  if (!dup) out[n++] = tmp[1];
  return n;
}

// find_block_contexts (common_block.c:283-309)
TK_DEV void find_contexts(const DbCell* cells, int cs, int ypos, int xpos, int fh, int fw, int size, int enable,
                          SynCtx* s) {
  if (ypos >= kMinBlk && xpos >= kMinBlk && ypos + size < fh && xpos + size < fw && enable && size <= 128) {
    const int bi = (ypos / kMinPb) * cs + xpos / kMinPb;
    const DbCell& up = cells[bi - cs];
    const DbCell& le = cells[bi - 1];
    int split = (up.size < size) + (le.size < size);
    s->ctx_cbp = ((up.cbp & 1) != 0) + ((le.cbp & 1) != 0);
    int cbp2 = (up.cbp != 0) + (le.cbp != 0);
    s->ctx_index = 3 * split + cbp2;
  } else {
    s->ctx_cbp = -1;
    s->ctx_index = -1;
  }
}
}  // namespace tk
