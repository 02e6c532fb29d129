// gol_rule.h — outer-totalistic ("life-like", B/S notation) rules on the bit
// board: the table builder and the rule stage of the rule-generic register
// pipeline (gol_kernels.hip, bit_rule_kernel).  Everything here is plain
// __host__ __device__ code, so a stand-alone host program
// (tests/fake_hip/rule_stage_check.cpp) proves the stage exhaustively; on the
// host the three-input v_bitop3_b32 is emulated from its truth table.
//
// A rule is two 9-bit masks: bit n of `birth` = a dead cell with n live
// neighbours (of 8) is born, bit n of `survive` = a live cell with n live
// neighbours stays alive.  B0 is not a rule here (the outside of the grid is
// permanently dead).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GOL_RULE_HD __host__ __device__ __forceinline__
#else
#define GOL_RULE_HD inline
#endif

namespace gol {

constexpr uint32_t kRuleBits = 0x1ffu;                 // neighbour counts 0..8
constexpr uint32_t kLifeBirth = 1u << 3;               // B3
constexpr uint32_t kLifeSurvive = (1u << 2) | (1u << 3);   // S23

// The launch argument of the rule-generic kernels.
struct RuleMasks {
    uint32_t birth, survive;
};

GOL_RULE_HD bool rule_valid(uint32_t birth, uint32_t survive) {
    return !((birth | survive) & ~kRuleBits) && !(birth & 1u);
}

// f(a, b, c) by truth table over a = 0xF0, b = 0xCC, c = 0xAA: one v_bitop3_b32.
template <int TT>
GOL_RULE_HD uint32_t rule_bitop3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
#else
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i)
        if ((TT >> i) & 1) r |= ((i & 4) ? a : ~a) & ((i & 2) ? b : ~b) & ((i & 1) ? c : ~c);
    return r;
#endif
}

// The stage sees, per cell, the 9-sum including the cell itself,
// S = o + 2u + 4w + 8z in 0..9 (z set means S is 8 or 9, so u = w = 0 there),
// and evaluates  alive ? survive[S-1] : birth[S]  as two XOR-of-monomials
// (algebraic normal form) polynomials over the 10 monomials
//   1, o, u, ou, w, ow, uw, ouw   (index = o + 2u + 4w)   and   z (8), oz (9).
// A coefficient is a wave-uniform word, 0 or ~0, and each term is ONE
// instruction with ONE scalar operand: acc = (M_i & k_i) ^ acc.
//  - dead cells: S = 9 cannot occur, so f(9) is chosen to make the oz
//    coefficient 0; the constant term is birth bit 0, which is never set.
//    Monomials 1..8: 8 coefficients.
//  - live cells: S = 0 cannot occur, so f(0) = 0 makes the constant term 0.
//    Monomials 1..9: 9 coefficients.
// 17 coefficients for the 2^17 rules: none is redundant.
struct RuleTable {
    uint32_t d[9];    // d[i], i = 1..8 (d[0] unused, 0)
    uint32_t a[10];   // a[i], i = 1..9 (a[0] unused, 0)
};

// Moebius transform of an 8-entry truth table (bit S = f(S)): bit i of the
// result is the coefficient of monomial i.
GOL_RULE_HD uint32_t rule_anf8(uint32_t t) {
    t ^= (t & 0x55u) << 1;
    t ^= (t & 0x33u) << 2;
    t ^= (t & 0x0fu) << 4;
    return t & 0xffu;
}

GOL_RULE_HD RuleTable rule_table(uint32_t birth, uint32_t survive) {
    RuleTable T;
    // dead: f(S) = birth[S], S = 0..8
    const uint32_t cd = rule_anf8(birth & 0xfeu);
    // f(8) = c0 ^ cz with c0 = 0
    const uint32_t dz = (birth >> 8) & 1u;
    // live: f(S) = survive[S-1], S = 1..9; f(0) = 0
    const uint32_t fa = (survive << 1) & 0x3ffu;
    const uint32_t ca = rule_anf8(fa & 0xffu);
    const uint32_t az = (fa >> 8) & 1u;                               // f(8) = cz
    const uint32_t aoz = ((fa >> 9) ^ (ca >> 1) ^ az) & 1u;          // f(9) = co ^ cz ^ coz
    T.d[0] = T.a[0] = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 1; i < 8; ++i) {
        T.d[i] = 0u - ((cd >> i) & 1u);
        T.a[i] = 0u - ((ca >> i) & 1u);
    }
    T.d[8] = 0u - dz;
    T.a[8] = 0u - az;
    T.a[9] = 0u - aoz;
    return T;
}

// acc ^ (m & k)
GOL_RULE_HD uint32_t rule_term(uint32_t m, uint32_t k, uint32_t acc) { return rule_bitop3<0x6A>(m, k, acc); }

// The rule stage on bit-sliced horizontal 3-sums of the rows above (a), at (b)
// and below (c), as life_bits takes them.  MASKED: `mask` = 0 forces the cell
// dead (columns outside the grid).
template <bool MASKED>
GOL_RULE_HD uint32_t rule_bits(const RuleTable &T, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0,
                               uint32_t c1, uint32_t alive, uint32_t mask) {
    const uint32_t o = rule_bitop3<0x96>(a0, b0, c0);    // vertical adders, as life_bits
    const uint32_t co = rule_bitop3<0xE8>(a0, b0, c0);
    const uint32_t p = rule_bitop3<0x96>(a1, b1, c1);
    const uint32_t q = rule_bitop3<0xE8>(a1, b1, c1);
    const uint32_t u = co ^ p;
    const uint32_t w = rule_bitop3<0x78>(q, co, p);      // q ^ (co & p)
    const uint32_t z = rule_bitop3<0x80>(q, co, p);      // q & co & p
    const uint32_t ou = o & u, ow = o & w, uw = u & w;
    const uint32_t ouw = rule_bitop3<0x80>(o, u, w);
    const uint32_t oz = o & z;
    uint32_t D = o & T.d[1];
    D = rule_term(u, T.d[2], D);
    D = rule_term(ou, T.d[3], D);
    D = rule_term(w, T.d[4], D);
    D = rule_term(ow, T.d[5], D);
    D = rule_term(uw, T.d[6], D);
    D = rule_term(ouw, T.d[7], D);
    D = rule_term(z, T.d[8], D);
    uint32_t A = o & T.a[1];
    A = rule_term(u, T.a[2], A);
    A = rule_term(ou, T.a[3], A);
    A = rule_term(w, T.a[4], A);
    A = rule_term(ow, T.a[5], A);
    A = rule_term(uw, T.a[6], A);
    A = rule_term(ouw, T.a[7], A);
    A = rule_term(z, T.a[8], A);
    A = rule_term(oz, T.a[9], A);
    const uint32_t r = rule_bitop3<0xCA>(alive, A, D);   // alive ? A : D
    return MASKED ? (r & mask) : r;
}

} // namespace gol
