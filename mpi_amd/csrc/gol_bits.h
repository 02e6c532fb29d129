// gol_bits.h — 1-bit-per-cell board I/O (gol_download_bits* / gol_upload_bits*,
// include/golhip.h): storage words of every layout <-> packed rows, MSB first
// (column j of a window is bit 7 - (j & 7) of byte j >> 3: numpy's packbits, a
// PBM P4 raster).  Plain __host__ __device__ code on top of gol_digest.h's
// canonicalisation (units, linear words, window masks, the column shift), so a
// stand-alone host program (tests/fake_hip/bits_check.cpp) proves the row
// routines against the per-cell definition; the kernels (gol_bits.hip) evaluate
// the same pieces per lane.
//
// A packed row is handled as u32 words in memory order: word w holds bytes
// 4w .. 4w + 3, i.e. window columns [32w, 32w + 32).  The CANONICAL word of those
// columns (bit j = column 32w + j, gol_digest.h) and the packed word differ by
// bits_out_word: every byte bit-reversed in place.  Download: unit -> linear
// words -> mask -> shift up by s -> NL + 1 canonical words -> bits_out_word.
// Upload: the same steps backwards, ending in a masked merge into the unit.
#pragma once
#include "gol_digest.h"

namespace gol {

// Canonical word <-> the u32 whose little-endian bytes are the MSB-first packed
// bytes: bit 8i + b <-> bit 8i + 7 - b (a 32-bit bit reverse and a byte swap).
// An involution.
GOL_DIGEST_HD uint32_t bits_out_word(uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bswap32(__builtin_bitreverse32(c));
#else
    c = ((c >> 1) & 0x55555555u) | ((c & 0x55555555u) << 1);
    c = ((c >> 2) & 0x33333333u) | ((c & 0x33333333u) << 2);
    return ((c >> 4) & 0x0f0f0f0fu) | ((c & 0x0f0f0f0fu) << 4);
#endif
}

// The unit's NL linear words -> its storage words: digest_linear<G> backwards
// (every exchange is its own inverse, so the same exchanges in reverse order).
// G = 0: one word -> 32 cell bytes (0/1), four per dword: a nibble n times
// 1 + 2^7 + 2^14 + 2^21 puts bit i of n on bit 8i (the four terms share no bit).
template <int G>
GOL_DIGEST_HD void bits_interleave(const uint32_t *L, uint32_t *w) {
    if (G == 2) {
        for (int g = 0; g < 2; ++g) {
            uint32_t a = L[2 * g], b = L[2 * g + 1];
            digest_swap<4>(a, b);
            digest_swap<3>(a, b);
            digest_swap<2>(a, b);
            digest_swap<1>(a, b);
            digest_swap<0>(a, b);
            w[2 * g] = a;
            w[2 * g + 1] = b;
        }
    } else if (G == 4) {
        uint32_t r0 = L[0], r2 = L[1], r1 = L[2], r3 = L[3];
        digest_swap<3>(r1, r3);
        digest_swap<3>(r0, r2);
        digest_swap<1>(r1, r3);
        digest_swap<1>(r0, r2);
        digest_swap<4>(r2, r3);
        digest_swap<4>(r0, r1);
        digest_swap<2>(r2, r3);
        digest_swap<2>(r0, r1);
        digest_swap<0>(r2, r3);
        digest_swap<0>(r0, r1);
        w[0] = r0;
        w[1] = r1;
        w[2] = r2;
        w[3] = r3;
    } else {
        for (int k = 0; k < 8; ++k) w[k] = (((L[0] >> (4 * k)) & 15u) * 0x00204081u) & 0x01010101u;
    }
}

// NL + 1 canonical words -> NL linear words: digest_shift<NL> backwards (down by s).
template <int NL>
GOL_DIGEST_HD void bits_unshift(const uint32_t *C, int s, uint32_t *L) {
    for (int t = 0; t < NL; ++t) L[t] = s ? (C[t] >> s) | (C[t + 1] << (32 - s)) : C[t];
}

// What a run [pc0, pc0 + ncols) (storage columns; pc0 = window column lc_rel0)
// means for unit q, computed once and kept down the rows.
template <int G> struct BitsUnit {
    uint32_t mask[DigestUnit<G>::NL];   // linear words: the run's columns
    int64_t w0;                         // packed word of canonical word 0: NL·q + dq
    int s;
};
template <int G>
GOL_DIGEST_HD BitsUnit<G> bits_unit_of(int64_t q, int64_t pc0, int64_t lc_rel0, int64_t ncols) {
    constexpr int NL = DigestUnit<G>::NL;
    const DigestShift h = digest_shift_of(pc0, lc_rel0);
    BitsUnit<G> u;
    for (int t = 0; t < NL; ++t) u.mask[t] = digest_mask(NL * q + t, pc0, pc0 + ncols);
    u.w0 = NL * q + h.dq;
    u.s = h.s;
    return u;
}

// Download, one unit of one row: its storage words -> NL + 1 packed words (word t
// belongs at packed word u.w0 + t; word NL is zero when s = 0).
template <int G>
GOL_DIGEST_HD void bits_get_unit(const uint32_t *w, const BitsUnit<G> &u, uint32_t *P) {
    constexpr int NL = DigestUnit<G>::NL;
    uint32_t L[NL], C[NL + 1];
    digest_linear<G>(w, L);
    for (int t = 0; t < NL; ++t) L[t] &= u.mask[t];
    digest_shift<NL>(L, u.s, C);
    for (int t = 0; t <= NL; ++t) P[t] = bits_out_word(C[t]);
}

// Upload, one unit: the merge masks in the unit's STORAGE words, computed once per
// unit.  keep = the bits of the run (they are replaced), live = those of them
// below active_cols (they take the packed value; the others are stored as 0).
// Byte layout: a cell's whole byte is replaced.
template <int G> struct BitsPutMask {
    uint32_t keep[DigestUnit<G>::WORDS], live[DigestUnit<G>::WORDS];
};
template <int G>
GOL_DIGEST_HD BitsPutMask<G> bits_put_mask_of(int64_t q, const BitsUnit<G> &u, int64_t active_cols) {
    constexpr int NL = DigestUnit<G>::NL, W = DigestUnit<G>::WORDS;
    uint32_t a[NL];
    for (int t = 0; t < NL; ++t) a[t] = u.mask[t] & digest_mask(NL * q + t, 0, active_cols);
    BitsPutMask<G> m;
    bits_interleave<G>(u.mask, m.keep);
    bits_interleave<G>(a, m.live);
    if (G == 0)
        for (int k = 0; k < W; ++k) m.keep[k] *= 0xffu;   // 0x01 per cell -> the cell's byte
    return m;
}

// Upload, one unit of one row: NL + 1 packed words (as bits_get_unit numbers them)
// merged into the unit's storage words.
template <int G>
GOL_DIGEST_HD void bits_put_unit(uint32_t *w, const BitsUnit<G> &u, const BitsPutMask<G> &m, const uint32_t *P) {
    constexpr int NL = DigestUnit<G>::NL, W = DigestUnit<G>::WORDS;
    uint32_t C[NL + 1], L[NL], S[W];
    for (int t = 0; t <= NL; ++t) C[t] = bits_out_word(P[t]);
    bits_unshift<NL>(C, u.s, L);
    bits_interleave<G>(L, S);
    for (int k = 0; k < W; ++k) w[k] = (w[k] & ~m.keep[k]) | (S[k] & m.live[k]);
}

// The packed words a run touches: [first, last].
GOL_DIGEST_HD int64_t bits_first_word(int64_t lc_rel0) { return lc_rel0 >> 5; }
GOL_DIGEST_HD int64_t bits_last_word(int64_t lc_rel0, int64_t ncols) { return (lc_rel0 + ncols - 1) >> 5; }

// The row routines (host reference of what a wave's lanes do together).  Storage
// columns [pc0, pc0 + ncols) of one row <-> window columns from lc_rel0 (>= 0) of
// the packed row `out` / `in`, which holds whole u32 words up to
// bits_last_word(lc_rel0, ncols).  The storage row must be accessible in whole
// units (rows are padded to them).
//
// get: the run's bits are OR-ed into `out` (the caller clears it: neighbouring
// units meet in one word, and so do several runs of one window).
template <int G>
GOL_DIGEST_HD void bits_get_row(const void *row, int64_t pc0, int64_t lc_rel0, int64_t ncols, uint32_t *out) {
    typedef DigestUnit<G> U;
    if (ncols <= 0) return;
    const uint32_t *words = static_cast<const uint32_t *>(row);
    const int64_t lo = bits_first_word(lc_rel0), hi = bits_last_word(lc_rel0, ncols);
    for (int64_t q = pc0 / U::COLS; q <= (pc0 + ncols - 1) / U::COLS; ++q) {
        const BitsUnit<G> u = bits_unit_of<G>(q, pc0, lc_rel0, ncols);
        uint32_t P[U::NL + 1];
        bits_get_unit<G>(words + q * U::WORDS, u, P);
        for (int t = 0; t <= U::NL; ++t)
            if (u.w0 + t >= lo && u.w0 + t <= hi) out[u.w0 + t] |= P[t];   // (outside: no cell of the run, P[t] = 0)
    }
}

// put: a masked merge.  Cells outside the run keep their value; the run's cells
// take the packed bits, columns >= active_cols (storage columns) are stored as 0.
// Bits of `in` outside the run's columns (pad bits, other runs) are ignored.
template <int G>
GOL_DIGEST_HD void bits_put_row(void *row, int64_t pc0, int64_t lc_rel0, int64_t ncols, int64_t active_cols,
                                const uint32_t *in) {
    typedef DigestUnit<G> U;
    if (ncols <= 0) return;
    uint32_t *words = static_cast<uint32_t *>(row);
    const int64_t lo = bits_first_word(lc_rel0), hi = bits_last_word(lc_rel0, ncols);
    for (int64_t q = pc0 / U::COLS; q <= (pc0 + ncols - 1) / U::COLS; ++q) {
        const BitsUnit<G> u = bits_unit_of<G>(q, pc0, lc_rel0, ncols);
        const BitsPutMask<G> m = bits_put_mask_of<G>(q, u, active_cols);
        uint32_t P[U::NL + 1];
        for (int t = 0; t <= U::NL; ++t) P[t] = u.w0 + t >= lo && u.w0 + t <= hi ? in[u.w0 + t] : 0u;
        bits_put_unit<G>(words + q * U::WORDS, u, m, P);
    }
}

}  // namespace gol
