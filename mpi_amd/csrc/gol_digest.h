// gol_digest.h — the layout-independent 128-bit board digest (gol_digest*,
// include/golhip.h): the hash arithmetic and the canonicalisation of storage
// words.  Everything here is plain __host__ __device__ code, so a stand-alone
// host program (tests/fake_hip/digest_check.cpp) proves the de-interleave, the
// masks and the column shift against the per-cell definition; the kernel
// (gol_kernels.hip, digest_kernel) evaluates the same routines per lane.
//
// All arithmetic is mod 2^64.  With sm = splitmix64's output function,
//   A_i(r) = sm(4r + i) | 1,  B_i(w) = sm(4w + 2 + i) | 1            (i = 0, 1)
//   h_i(r, c) = A_i(r) · B_i(c >> 5) · 2^(c & 31)
//   digest_i  = Σ h_i(r, c) over the live cells (r, c), GLOBAL coordinates
// i.e. per row Σ_w B_i(w)·W(r, w) times A_i(r), W(r, w) the row's canonical
// 32-column word (bit j = column 32w + j).  The empty board gives (0, 0);
// digests of disjoint windows add; two boards that differ inside one canonical
// word differ in both lanes (odd · odd · (0 < x < 2^32) != 0 mod 2^64).
// Anything else is probabilistic: the digest is not cryptographic.
//
// Storage is read in UNITS: 4 u32 words of a bit row (two 2-word groups or one
// 4-word group, 128 storage columns) or 32 cell bytes of a byte row.  A unit
// becomes NL "linear" words (bit j of linear word u = storage column 32u + j;
// NL = 4 resp. 1), masked to the window's storage columns [pc0, pc1); storage
// column p is logical column p + d, so with d = 32·dq + s (0 <= s < 32) the
// NL linear words of unit q contribute NL + 1 canonical words
// NL·q + dq .. NL·q + dq + NL: a funnel shift by s between neighbours.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GOL_DIGEST_HD __host__ __device__ __forceinline__
#else
#define GOL_DIGEST_HD inline
#endif

namespace gol {

GOL_DIGEST_HD uint64_t digest_sm(uint64_t x) {   // splitmix64; digest_sm(0) = 0xE220A8397B1DCDAF
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
GOL_DIGEST_HD uint64_t digest_A(int i, int64_t r) { return digest_sm(4 * (uint64_t)r + (uint64_t)i) | 1u; }
GOL_DIGEST_HD uint64_t digest_B(int i, int64_t w) { return digest_sm(4 * (uint64_t)w + 2u + (uint64_t)i) | 1u; }

// Linear words per unit and storage columns per unit.  G: 0 = byte layout, else
// the bit layout's group width.
template <int G> struct DigestUnit {
    static constexpr int NL = G ? 4 : 1;
    static constexpr int COLS = 32 * NL;
    static constexpr int BYTES = G ? 16 : 32;   // of the row a unit occupies
    static constexpr int WORDS = BYTES / 4;
};

// Exchange bit B of the in-word bit index with the index of the word pair
// (a, b): bit p of b (p without bit B) <-> bit p + 2^B of a.
template <int B>
GOL_DIGEST_HD void digest_swap(uint32_t &a, uint32_t &b) {
    constexpr uint32_t m = B == 0 ? 0x55555555u : B == 1 ? 0x33333333u : B == 2 ? 0x0f0f0f0fu
                         : B == 3 ? 0x00ff00ffu : 0x0000ffffu;
    const uint32_t t = ((a >> (1 << B)) ^ b) & m;
    b ^= t;
    a ^= t << (1 << B);
}

// The unit's storage words -> its NL linear words.
//  G = 2: a group (x, y) holds column 2j + w in word w, bit j: the 6 index bits
//         (w | j4..j0) rotate left by one, five exchanges through the word index.
//  G = 4: column 4j + w in word w, bit j: the 7 index bits (w1 w0 | j4..j0)
//         rotate left by two; as exchanges through index bit w0: with j0, j2,
//         j4, w1 (a renaming of words), j1, j3.
//  G = 0: 32 cell bytes (0/1) -> one word.
template <int G>
GOL_DIGEST_HD void digest_linear(const uint32_t *w, uint32_t *L) {
    if (G == 2) {
        for (int g = 0; g < 2; ++g) {
            uint32_t a = w[2 * g], b = w[2 * g + 1];
            digest_swap<0>(a, b);
            digest_swap<1>(a, b);
            digest_swap<2>(a, b);
            digest_swap<3>(a, b);
            digest_swap<4>(a, b);
            L[2 * g] = a;
            L[2 * g + 1] = b;
        }
    } else if (G == 4) {
        uint32_t r0 = w[0], r1 = w[1], r2 = w[2], r3 = w[3];
        digest_swap<0>(r0, r1);
        digest_swap<0>(r2, r3);
        digest_swap<2>(r0, r1);
        digest_swap<2>(r2, r3);
        digest_swap<4>(r0, r1);
        digest_swap<4>(r2, r3);
        // exchange of the two word-index bits: words 1 and 2 trade places
        digest_swap<1>(r0, r2);
        digest_swap<1>(r1, r3);
        digest_swap<3>(r0, r2);
        digest_swap<3>(r1, r3);
        L[0] = r0;
        L[1] = r2;
        L[2] = r1;
        L[3] = r3;
    } else {
        // two dwords at a time: cell bytes b0..b3 of the first in bit 0, of the second in
        // bit 4 of a byte; times 2^24 + 2^17 + 2^10 + 2^3 every one of the 8 cell bits
        // lands on a bit of the top byte of its own (no two terms meet, so no carries)
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) {
            const uint32_t y = (w[2 * k] & 0x01010101u) | ((w[2 * k + 1] & 0x01010101u) << 4);
            v |= ((y * 0x01020408u) >> 24) << (8 * k);
        }
        L[0] = v;
    }
}

// Bits of linear word u (storage columns [32u, 32u + 32)) inside [pc0, pc1).
GOL_DIGEST_HD uint32_t digest_mask(int64_t u, int64_t pc0, int64_t pc1) {
    const int64_t lo = pc0 - 32 * u, hi = pc1 - 32 * u;
    if (hi <= 0 || lo >= 32) return 0u;
    const uint32_t above = lo <= 0 ? 0xffffffffu : 0xffffffffu << lo;
    const uint32_t below = hi >= 32 ? 0xffffffffu : ~(0xffffffffu << hi);
    return above & below;
}

// NL masked linear words, shifted up by s columns (0 <= s < 32): NL + 1 canonical words.
template <int NL>
GOL_DIGEST_HD void digest_shift(const uint32_t *L, int s, uint32_t *C) {
    if (s == 0) {
        for (int t = 0; t < NL; ++t) C[t] = L[t];
        C[NL] = 0u;
        return;
    }
    C[0] = L[0] << s;
    for (int t = 1; t < NL; ++t) C[t] = (L[t] << s) | (L[t - 1] >> (32 - s));
    C[NL] = L[NL - 1] >> (32 - s);
}

// The column shift of a window: storage column p is logical column p + d.
struct DigestShift {
    int64_t dq;   // floor(d / 32)
    int s;        // d mod 32, 0 .. 31
};
GOL_DIGEST_HD DigestShift digest_shift_of(int64_t pc0, int64_t lc0) {
    const int64_t d = lc0 - pc0;
    DigestShift h;
    h.dq = d >> 5;   // arithmetic shift: floor
    h.s = (int)(d & 31);
    return h;
}

// Unit q of a row (its storage words at `w`): sum[i] += Σ B_i(word)·(canonical word),
// with the window's masks and shift.  Bu[i][t] = B_i(NL·q + dq + t), t = 0 .. NL.
template <int G>
GOL_DIGEST_HD void digest_unit(const uint32_t *w, const uint32_t *mask, int s, const uint64_t (*Bu)[5],
                               uint64_t sum[2]) {
    constexpr int NL = DigestUnit<G>::NL;
    uint32_t L[NL], C[NL + 1];
    digest_linear<G>(w, L);
    for (int t = 0; t < NL; ++t) L[t] &= mask[t];
    digest_shift<NL>(L, s, C);
    for (int i = 0; i < 2; ++i) {
        for (int t = 0; t < NL; ++t) sum[i] += Bu[i][t] * (uint64_t)C[t];
        if (s) sum[i] += Bu[i][NL] * (uint64_t)C[NL];   // (no shift: nothing reaches the next word)
    }
}

// The row routine (host reference of what a wave's lanes do together): storage
// columns [pc0, pc0 + ncols) of one row, logical columns from lc0:
// sum[i] = Σ_w B_i(w)·W(w) over those cells (the caller applies A_i(r)).
// The row must be readable in whole units (rows are padded to them).
template <int G>
GOL_DIGEST_HD void digest_row(const void *row, int64_t pc0, int64_t lc0, int64_t ncols, uint64_t sum[2]) {
    typedef DigestUnit<G> U;
    sum[0] = sum[1] = 0;
    if (ncols <= 0) return;
    const DigestShift h = digest_shift_of(pc0, lc0);
    const uint32_t *words = static_cast<const uint32_t *>(row);
    for (int64_t q = pc0 / U::COLS; q <= (pc0 + ncols - 1) / U::COLS; ++q) {
        uint32_t mask[U::NL];
        uint64_t Bu[2][5];
        for (int t = 0; t < U::NL; ++t) mask[t] = digest_mask(U::NL * q + t, pc0, pc0 + ncols);
        for (int i = 0; i < 2; ++i)
            for (int t = 0; t <= U::NL; ++t) Bu[i][t] = digest_B(i, U::NL * q + h.dq + t);
        digest_unit<G>(words + q * U::WORDS, mask, h.s, Bu, sum);
    }
}

}  // namespace gol
