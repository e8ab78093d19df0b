// The steps of one work item of the streaming expand + depthwise kernels (k_xdw_stream.hip, k_xdw_wreg.hip): which of them either role has
// work in.  One rule, used by the kernels' step loops and by the host's count (expand_dw_steps, ams_k_expand_dw_steps); every value is
// uniform over a block, so on the device it lives in scalar registers.
//
// An item is a segment of SH x SW pixels of a sub-image, laid out in raster order with one pad column on each side (row pitch Wp = SW + 2)
// and one halo row above and below: position p = row * Wp + col, row in [0, SH + 2), stands for pixel (i0 - 1 + row, j0 - 1 + col).
// E-step t writes the expanded values of positions [t STEP, (t + 1) STEP) into the ring; D-step t — it runs beside E-step t + 1 — takes the
// centres [t STEP - Wp - 1, (t + 1) STEP - Wp - 1), whose last tap E-step t wrote.  Three rectangles of (row, col) decide everything:
//   inside: the positions that are pixels of the feature map                      -> an E-step that meets it COMPUTES (and so does every
//           step between two that do)
//   read:   rows 0 .. rows + 1, columns 0 .. cols + 1: what the stored centres read -> an E-step that meets only it writes ZEROS (the
//           depthwise conv's padding), one that meets neither is IDLE and leaves its ring slots as they are
//   stored: rows 1 .. rows, columns 1 .. cols: the centres whose result is kept   -> a D-step that meets it is ACTIVE
// (rows, cols: the item's real size, min(SH, Hs - i0) x min(SW, Ws - j0); inside is part of read.)  The item ends with the D-step of its
// last stored centre: T_item = that step + 1, for both roles, so their barrier counts agree.  An item that is not live has no step at all.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AMS_XDW_HD __host__ __device__ inline
#else
#define AMS_XDW_HD inline
#endif

namespace ams {

enum XdwEClass { XDW_E_IDLE = 0, XDW_E_ZERO = 1, XDW_E_COMPUTE = 2 };

// rows r0 .. r1, columns c0 .. c1 (r1 < -2 when empty), and the steps t0 .. t1 of its first and last position.  Between two rows of a
// rectangle lie Wp - (c1 - c0 + 1) positions: where that is less than a step — every plan the launchers pick by themselves — each step from
// t0 to t1 meets the rectangle and two compares decide; only a narrow last column strip leaves gaps a whole step fits into (`gaps`), and
// then the step's first position is tested against the rows
struct XdwRect { int r0, r1, c0, c1, t0, t1; bool gaps; };

struct XdwItemSteps {
    int Wp, STEP, qS, rS;                            // STEP = qS * Wp + rS
    int T_item;
    XdwRect inside, read, stored;
};

// Hs x Ws: the item's sub-image; (i0, j0): the segment's first pixel in it
AMS_XDW_HD XdwItemSteps xdw_item_steps(int Wp, int STEP, int SH, int Hs, int Ws, int i0, int j0) {
    constexpr int EMPTY = -(1 << 20);
    const int SW = Wp - 2;
    const bool live = i0 < Hs && j0 < Ws;
    const int rows = SH < Hs - i0 ? SH : Hs - i0, cols = SW < Ws - j0 ? SW : Ws - j0;
    XdwItemSteps s;
    s.Wp = Wp; s.STEP = STEP; s.qS = STEP / Wp; s.rS = STEP - s.qS * Wp;
    s.T_item = live ? (rows * Wp + cols + Wp + 1) / STEP + 1 : 0;
    // lag: a D-step takes the centres Wp + 1 positions behind the E-step of the same index
    const auto rect = [&](int r0, int r1, int c0, int c1, int lag) {
        XdwRect r{r0, live ? r1 : EMPTY, c0, c1, 1, 0, false};
        if (live) { r.t0 = (r0 * Wp + c0 + lag) / STEP; r.t1 = (r1 * Wp + c1 + lag) / STEP; r.gaps = Wp - (c1 - c0 + 1) >= STEP; }
        return r;
    };
    s.inside = rect(i0 == 0 ? 1 : 0, SH + 1 < Hs - i0 ? SH + 1 : Hs - i0, j0 == 0 ? 1 : 0, SW + 1 < Ws - j0 ? SW + 1 : Ws - j0, 0);
    s.read = rect(0, rows + 1, 0, cols + 1, 0);
    s.stored = rect(1, rows, 1, cols, Wp + 1);
    return s;
}

// the first position of a step (E) or its first centre (D), carried from step to step without a division
struct XdwWalk { int row, col; };
AMS_XDW_HD XdwWalk xdw_e_start() { return XdwWalk{0, 0}; }
AMS_XDW_HD XdwWalk xdw_d_start(int Wp) { return XdwWalk{-2, Wp - 1}; }      // position -Wp - 1
AMS_XDW_HD void xdw_advance(XdwWalk& w, const XdwItemSteps& s) {
    w.row += s.qS; w.col += s.rS;
    if (w.col >= s.Wp) { w.col -= s.Wp; ++w.row; }
}

// does step t, the run of STEP positions that starts at w, meet the rectangle?
AMS_XDW_HD bool xdw_meets(int t, const XdwWalk& w, const XdwRect& r, const XdwItemSteps& s) {
    if (!r.gaps) return (t >= r.t0) & (t <= r.t1);
    int dist;                                        // from w to the rectangle's first position at or behind it
    if (w.row > r.r1) return false;
    if (w.row < r.r0) dist = (r.r0 - w.row) * s.Wp + r.c0 - w.col;
    else if (w.col <= r.c1) dist = w.col < r.c0 ? r.c0 - w.col : 0;
    else if (w.row < r.r1) dist = s.Wp - w.col + r.c0;
    else return false;
    return dist < s.STEP;
}

// The compute steps are ALL the steps from the first to the last that meets `inside`, so that they follow each other and each can request
// the operands of the next: with gaps between the rows (above) that takes in steps that hold no pixel — they compute zeros, as every
// position outside the feature map does
AMS_XDW_HD int xdw_e_class(int t, const XdwWalk& e, const XdwItemSteps& s) {
    return ((t >= s.inside.t0) & (t <= s.inside.t1)) ? XDW_E_COMPUTE : (xdw_meets(t, e, s.read, s) ? XDW_E_ZERO : XDW_E_IDLE);
}
AMS_XDW_HD bool xdw_d_active(int t, const XdwWalk& d, const XdwItemSteps& s) { return xdw_meets(t, d, s.stored, s); }

}  // namespace ams
