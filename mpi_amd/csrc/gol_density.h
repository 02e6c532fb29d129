// gol_density.h — per-tile live-cell counts (gol_density*, include/golhip.h):
// the row routine, on top of the canonicalisation of gol_digest.h (units, linear
// words, window masks, the funnel shift; included, not copied).  Plain
// __host__ __device__ code: a stand-alone host program
// (tests/fake_hip/density_check.cpp) proves it against the per-cell definition,
// and the kernel (gol_kernels.hip, density_kernel) evaluates the same routines
// per lane.
//
// A window starts at logical column col0 (a multiple of 32) and is cut into
// tiles of tile_cols columns (a multiple of 32), so every canonical 32-column
// word w belongs to exactly one tile column, (32w - col0) / tile_cols.  Where
// the digest weighs a canonical word, the map takes its popcount.  A popcount
// does not care where a bit sits inside its word or its unit, so a unit that is
// whole (every mask full), unshifted (s = 0) and inside one tile is counted on
// its storage words as they are: density_unit_whole, no de-interleave.
#pragma once
#include "gol_digest.h"

namespace gol {

GOL_DIGEST_HD uint32_t density_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// Tile column of canonical word w.  Only words with a cell of the window in them
// are asked for in earnest (w >= col0 / 32); a word before the window has count 0
// and is never added anywhere.
GOL_DIGEST_HD int64_t density_tile_of(int64_t w, int64_t col0, int64_t tile_cols) {
    return (32 * w - col0) / tile_cols;
}

// Live cells of a whole unit from its storage words, no de-interleave: the bit
// layouts' words are a permutation of the unit's cells; 32 cell bytes (0/1) add
// up byte-wise (at most 8 per byte field), then across the four fields.
template <int G>
GOL_DIGEST_HD uint32_t density_unit_whole(const uint32_t *w) {
    if (G) return density_popc(w[0]) + density_popc(w[1]) + density_popc(w[2]) + density_popc(w[3]);
    uint32_t x = 0;
    for (int k = 0; k < 8; ++k) x += w[k] & 0x01010101u;
    return (x * 0x01010101u) >> 24;
}

// The general path: cnt[t] += live cells of canonical word t of the unit
// (t = 0 .. NL), with the window's masks and shift, as digest_unit.
template <int G>
GOL_DIGEST_HD void density_unit(const uint32_t *w, const uint32_t *mask, int s, uint32_t *cnt) {
    constexpr int NL = DigestUnit<G>::NL;
    uint32_t L[NL], C[NL + 1];
    digest_linear<G>(w, L);
    for (int t = 0; t < NL; ++t) L[t] &= mask[t];
    digest_shift<NL>(L, s, C);
    for (int t = 0; t < NL; ++t) cnt[t] += density_popc(C[t]);
    if (s) cnt[NL] += density_popc(C[NL]);   // (no shift: nothing reaches the next word)
}

// May unit q take density_unit_whole?  Its masks (NL of them) and the tile
// columns tc[0 .. NL] of its canonical words are at hand.
template <int G>
GOL_DIGEST_HD bool density_is_whole(const uint32_t *mask, int s, const int64_t *tc) {
    constexpr int NL = DigestUnit<G>::NL;
    if (s != 0 || tc[0] != tc[NL - 1]) return false;
    for (int t = 0; t < NL; ++t)
        if (mask[t] != 0xffffffffu) return false;
    return true;
}

// The row routine (host reference of what a wave's lanes do together): storage
// columns [pc0, pc0 + ncols) of one row, logical columns from lc0, in a window
// that starts at logical column col0 with tiles of tile_cols columns:
// tiles[j] += live cells of the run in tile column j (0 <= j < ntiles; the
// caller's window guarantees that range for every cell of the run).
// The row must be readable in whole units (rows are padded to them).
template <int G>
GOL_DIGEST_HD void density_row(const void *row, int64_t pc0, int64_t lc0, int64_t ncols, int64_t col0,
                               int64_t tile_cols, uint32_t *tiles, int64_t ntiles) {
    typedef DigestUnit<G> U;
    if (ncols <= 0) return;
    const DigestShift h = digest_shift_of(pc0, lc0);
    const uint32_t *words = static_cast<const uint32_t *>(row);
    for (int64_t q = pc0 / U::COLS; q <= (pc0 + ncols - 1) / U::COLS; ++q) {
        uint32_t mask[U::NL], cnt[U::NL + 1];
        int64_t tc[U::NL + 1];
        for (int t = 0; t < U::NL; ++t) mask[t] = digest_mask(U::NL * q + t, pc0, pc0 + ncols);
        for (int t = 0; t <= U::NL; ++t) {
            tc[t] = density_tile_of(U::NL * q + h.dq + t, col0, tile_cols);
            cnt[t] = 0u;
        }
        if (density_is_whole<G>(mask, h.s, tc)) cnt[0] = density_unit_whole<G>(words + q * U::WORDS);
        else density_unit<G>(words + q * U::WORDS, mask, h.s, cnt);
        for (int t = 0; t <= U::NL; ++t)
            if (cnt[t] && tc[t] >= 0 && tc[t] < ntiles) tiles[tc[t]] += cnt[t];
    }
}

}  // namespace gol
