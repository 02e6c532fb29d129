// gol_copy.h — board-to-board copies (gol_copy_window / gol_copy, include/golhip.h):
// the cells of a run of storage columns of one row, in any storage form (byte,
// 2-word groups, 4-word groups), merged into a run of another row in any storage
// form, at any relative column shift.  Plain __host__ __device__ code on top of
// gol_digest.h (units, linear words, masks) and gol_bits.h (interleave, the merge
// masks), so a stand-alone host program (tests/fake_hip/copy_check.cpp) proves the
// row routine against the per-cell definition; the kernel (gol_copy.hip) evaluates
// the same pieces per lane.
//
// Storage column p of the SOURCE run [spc0, spc0 + ncols) is storage column p + d
// of the DESTINATION run [dpc0, dpc0 + ncols), d = dpc0 - spc0 = 32·dq + s
// (0 <= s < 32).  In linear words (bit j of word i = storage column 32i + j)
//     D[i] = S[i - dq] << s | S[i - dq - 1] >> (32 - s)          (s = 0: S[i - dq])
// so the ND linear words of destination unit q need the ND + 1 (s = 0: ND) source
// words from i0 = ND·q - dq - (s ? 1 : 0): at most CopyPair::MAXU whole source
// units from u0 = floor(i0 / NS).  Source units outside the run's own
// [first, last] are NOT read: they hold no cell of the run (`have`, as put_bits
// treats packed words), so a run that ends in the last unit of an allocation reads
// nothing behind it.  The source words are not masked to the run: every bit they
// carry beyond it lands outside the destination run, where the merge masks
// (BitsPutMask: keep = the run's bits, live = those below active_cols) drop it:
//     w = (w & ~keep) | (op(w, S) & live)
// Same storage form and d a multiple of the unit's columns: the storage words of
// source unit q - d / COLS are merged as they are (`direct`).
#pragma once
#include "gol_bits.h"

namespace gol {

// gol_copy_window's ops (GOL_COPY_* of include/golhip.h)
enum { kCopyReplace = 0, kCopyOr = 1, kCopyXor = 2 };

template <int GS, int GD> struct CopyPair {
    static constexpr int NS = DigestUnit<GS>::NL, ND = DigestUnit<GD>::NL;
    static constexpr int WS = DigestUnit<GS>::WORDS, WD = DigestUnit<GD>::WORDS;
    // ND + 1 consecutive words from any offset inside a unit of NS words
    static constexpr int MAXU = (NS - 1 + ND) / NS + 1;
};

GOL_DIGEST_HD int64_t copy_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// What the two runs mean for destination unit q, computed once and kept down the rows.
template <int GS, int GD> struct CopyUnit {
    BitsPutMask<GD> m;
    int64_t u0;                         // first source unit of the covering range
    int o;                              // the first needed source word is word o of unit u0
    int s;                              // the funnel shift
    bool direct;                        // storage words are merged as they are (one source unit)
    bool have[CopyPair<GS, GD>::MAXU];  // unit u0 + k is needed and one of the run's own
    bool covered;                       // the run replaces every bit of the unit
};

template <int GS, int GD>
GOL_DIGEST_HD CopyUnit<GS, GD> copy_unit_of(int64_t q, int64_t spc0, int64_t dpc0, int64_t ncols, int64_t active_cols) {
    typedef CopyPair<GS, GD> P;
    CopyUnit<GS, GD> cu;
    const BitsUnit<GD> bu = bits_unit_of<GD>(q, dpc0, dpc0, ncols);
    cu.m = bits_put_mask_of<GD>(q, bu, active_cols);
    cu.covered = true;
    for (int k = 0; k < P::WD; ++k) cu.covered = cu.covered && cu.m.keep[k] == 0xffffffffu;
    const int64_t d = dpc0 - spc0;
    const int64_t first = spc0 / DigestUnit<GS>::COLS, last = (spc0 + ncols - 1) / DigestUnit<GS>::COLS;
    cu.direct = GS == GD && d % DigestUnit<GD>::COLS == 0;
    int n;   // source words needed from (u0, o)
    if (cu.direct) {
        cu.u0 = q - d / DigestUnit<GD>::COLS;
        cu.o = 0;
        cu.s = 0;
        n = 1;   // (unit k = 0 only)
    } else {
        const int64_t dq = d >> 5;   // arithmetic shift: floor
        cu.s = (int)(d & 31);
        const int64_t i0 = (int64_t)P::ND * q - dq - (cu.s ? 1 : 0);
        cu.u0 = copy_floor_div(i0, P::NS);
        cu.o = (int)(i0 - cu.u0 * P::NS);
        n = P::ND + (cu.s ? 1 : 0);
    }
    for (int k = 0; k < P::MAXU; ++k)
        cu.have[k] = k * P::NS <= cu.o + n - 1 && cu.u0 + k >= first && cu.u0 + k <= last;
    return cu;
}

// One destination unit of one row: xs = the storage words of source units
// u0 .. u0 + MAXU - 1 (zeros where !have), w = the destination unit's storage words
// (any value where covered and op = REPLACE: it is not used).
template <int GS, int GD>
GOL_DIGEST_HD void copy_unit(const uint32_t (*xs)[CopyPair<GS, GD>::WS], uint32_t *w, const CopyUnit<GS, GD> &cu, int op) {
    typedef CopyPair<GS, GD> P;
    uint32_t S[P::WD];
    if (GS == GD && cu.direct) {
        for (int k = 0; k < P::WD; ++k) S[k] = xs[0][k < P::WS ? k : 0];
    } else {
        uint32_t SL[P::MAXU * P::NS], W[P::ND + 1], L[P::ND];
        for (int k = 0; k < P::MAXU; ++k) digest_linear<GS>(xs[k], SL + k * P::NS);
        // word o + t of SL by constant indices only (a variable index would put SL in scratch)
        for (int t = 0; t <= P::ND; ++t) {
            W[t] = 0u;
            if (P::NS == 1) {
                if (t < P::MAXU) W[t] = SL[t];
            } else {
                for (int i = t; i < P::MAXU * P::NS && i < t + P::NS; ++i)
                    if (i == cu.o + t) W[t] = SL[i];
            }
        }
        for (int t = 0; t < P::ND; ++t) L[t] = cu.s ? (W[t + 1] << cu.s) | (W[t] >> (32 - cu.s)) : W[t];
        bits_interleave<GD>(L, S);
    }
    for (int k = 0; k < P::WD; ++k) {
        const uint32_t v = op == kCopyOr ? w[k] | S[k] : op == kCopyXor ? w[k] ^ S[k] : S[k];
        w[k] = (w[k] & ~cu.m.keep[k]) | (v & cu.m.live[k]);
    }
}

// The row routine (host reference of what a wave's lanes do together): the cells
// of storage columns [spc0, spc0 + ncols) of src_row are merged under `op` into
// storage columns [dpc0, dpc0 + ncols) of dst_row; destination columns >=
// active_cols are stored as 0; no other cell of dst_row changes.  Of src_row only
// the units that hold cells of the run are read; dst_row is accessed in whole
// units (rows are padded to them).  The rows may be one row when the two runs are
// disjoint: a merge changes no bit outside its run.
template <int GS, int GD>
GOL_DIGEST_HD void copy_row(const void *src_row, int64_t spc0, void *dst_row, int64_t dpc0, int64_t ncols,
                            int64_t active_cols, int op) {
    typedef CopyPair<GS, GD> P;
    if (ncols <= 0) return;
    const uint32_t *sw = static_cast<const uint32_t *>(src_row);
    uint32_t *dw = static_cast<uint32_t *>(dst_row);
    for (int64_t q = dpc0 / DigestUnit<GD>::COLS; q <= (dpc0 + ncols - 1) / DigestUnit<GD>::COLS; ++q) {
        const CopyUnit<GS, GD> cu = copy_unit_of<GS, GD>(q, spc0, dpc0, ncols, active_cols);
        uint32_t xs[P::MAXU][P::WS], w[P::WD];
        for (int k = 0; k < P::MAXU; ++k)
            for (int v = 0; v < P::WS; ++v) xs[k][v] = cu.have[k] ? sw[(cu.u0 + k) * P::WS + v] : 0u;
        const bool read = !(cu.covered && op == kCopyReplace);
        for (int v = 0; v < P::WD; ++v) w[v] = read ? dw[q * P::WD + v] : 0u;
        copy_unit<GS, GD>(xs, w, cu, op);
        for (int v = 0; v < P::WD; ++v) dw[q * P::WD + v] = w[v];
    }
}

}  // namespace gol
