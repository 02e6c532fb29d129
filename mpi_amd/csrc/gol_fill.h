// gol_fill.h — the counter-based random fill (gol_fill_random*, include/golhip.h):
// a seeded soup at any density, defined by a formula on GLOBAL coordinates the way
// the digest is, so every layout, group width, depth, boundary storage, slab count
// and rank context writes the same cells with no communication.  Plain
// __host__ __device__ code on top of gol_bits.h's masked merge, so a stand-alone
// host program (tests/fake_hip/fill_check.cpp) proves the row routine against the
// per-cell definition; the kernel (gol_fill.hip) evaluates the same pieces per lane.
//
// All arithmetic is mod 2^64, sm = splitmix64's output function (digest_sm):
//   K        = sm(seed)
//   h(r,w,j) = sm( sm(K + r) + 16·w + j )          r = global row, w = global column >> 5, j = 0 .. 15
//   plane 2j (r,w) = low 32 bits of h(r,w,j),  plane 2j+1 (r,w) = high 32 bits
//   X(r,c)   = Σ_i 2^i · bit (c & 31) of plane i (r, c >> 5)                (uniform in [0, 2^32))
//   cell (r,c) is live  iff  X(r,c) < T             0 <= T <= 2^32
// Bit-sliced over the 32 columns of a word, X < T is evaluated from the lowest
// plane up, lt = 0 to start: bit i of T set: lt = ~plane_i | lt, else lt = ~plane_i & lt.
// Planes below the lowest set bit of T leave lt = 0, so they — and the sm calls that
// produce only them — are skipped: density 1/2 costs one sm per word (half of whose
// bits are used), a full 32-bit threshold 16.
#pragma once
#include "gol_bits.h"

namespace gol {

constexpr uint64_t kFillFull = 1ull << 32;   // T = 2^32: every cell

GOL_DIGEST_HD uint64_t fill_key(uint64_t seed) { return digest_sm(seed); }
GOL_DIGEST_HD uint64_t fill_row_key(uint64_t K, int64_t r) { return digest_sm(K + (uint64_t)r); }

// First hash a threshold needs (j of its lowest set bit's plane); 16: none (T = 0 or 2^32).
GOL_DIGEST_HD int fill_first_hash(uint64_t T) {
    if (T == 0 || T >= kFillFull) return 16;
    int p = 0;
    while (!((T >> p) & 1u)) ++p;
    return p >> 1;
}

// One plane of the comparison: m = all ones when the plane's bit of T is set, else 0.
//   m = ~0: ~p | lt        m = 0: ~p & lt
GOL_DIGEST_HD uint32_t fill_plane(uint32_t lt, uint32_t p, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
    // one three-input bit operation; the table of m ? ~p | lt : ~p & lt over (p, lt, m) = (0xF0, 0xCC, 0xAA)
    return __builtin_amdgcn_bitop3_b32(p, lt, m, 0x8e);
#else
    return (~p & (lt | m)) | (lt & m);
#endif
}

// The canonical word (bit j = column 32w + j) of global word w of a row with key
// R = fill_row_key(K, r); j0 = fill_first_hash(T), 0 < T < 2^32.
GOL_DIGEST_HD uint32_t fill_word_keyed(uint64_t R, uint32_t T, int j0, int64_t w) {
    const uint64_t base = R + 16u * (uint64_t)w;
    uint32_t lt = 0u;
    for (int j = j0; j < 16; ++j) {
        const uint64_t h = digest_sm(base + (uint64_t)j);
        lt = fill_plane(lt, (uint32_t)h, 0u - ((T >> (2 * j)) & 1u));   // (a plane below T's lowest bit: lt stays 0)
        lt = fill_plane(lt, (uint32_t)(h >> 32), 0u - ((T >> (2 * j + 1)) & 1u));
    }
    return lt;
}

GOL_DIGEST_HD uint32_t fill_word(uint64_t K, uint64_t T, int64_t r, int64_t w) {
    if (T == 0) return 0u;
    if (T >= kFillFull) return 0xffffffffu;
    return fill_word_keyed(fill_row_key(K, r), (uint32_t)T, fill_first_hash(T), w);
}

// bits_put_unit on canonical words (C[t] belongs at global word u.w0 + t): no
// MSB-first bytes on the way.
template <int G>
GOL_DIGEST_HD void fill_put_unit(uint32_t *w, const BitsUnit<G> &u, const BitsPutMask<G> &m, const uint32_t *C) {
    constexpr int NL = DigestUnit<G>::NL, W = DigestUnit<G>::WORDS;
    uint32_t L[NL], S[W];
    bits_unshift<NL>(C, u.s, L);
    bits_interleave<G>(L, S);
    for (int k = 0; k < W; ++k) w[k] = (w[k] & ~m.keep[k]) | (S[k] & m.live[k]);
}

// The row routine (host reference of what a wave's lanes do together): storage
// columns [pc0, pc0 + ncols) of global row r, which are GLOBAL logical columns from
// lc0 (passed as bits_unit_of's window column, so a unit's packed word index is
// the global word).  Cells outside the run keep their value; storage columns
// >= active_cols are stored as 0.  The row must be accessible in whole units.
template <int G>
GOL_DIGEST_HD void fill_put_row(void *row, int64_t pc0, int64_t lc0, int64_t ncols, int64_t active_cols, uint64_t K,
                                uint64_t T, int64_t r) {
    typedef DigestUnit<G> U;
    if (ncols <= 0) return;
    uint32_t *words = static_cast<uint32_t *>(row);
    for (int64_t q = pc0 / U::COLS; q <= (pc0 + ncols - 1) / U::COLS; ++q) {
        const BitsUnit<G> u = bits_unit_of<G>(q, pc0, lc0, ncols);
        const BitsPutMask<G> m = bits_put_mask_of<G>(q, u, active_cols);
        uint32_t C[U::NL + 1];
        for (int t = 0; t <= U::NL; ++t) C[t] = fill_word(K, T, r, u.w0 + t);
        fill_put_unit<G>(words + q * U::WORDS, u, m, C);
    }
}

}  // namespace gol
