// gol_rule.h — outer-totalistic ("life-like", B/S notation) rules on the bit
// board: the table builder and the rule stage of the rule-generic register
// pipeline (gol_kernels.hip, bit_rule_kernel).  Everything here is plain
// __host__ __device__ code, so a stand-alone host program
// (tests/fake_hip/rule_stage_check.cpp) proves the stage exhaustively; on the
// host the three-input v_bitop3_b32 is emulated from its truth table.  Second
// half: the stage of the kernels compiled for one rule each (bit_crule_kernel),
// its constexpr synthesiser and the list of those rules, proven likewise
// (tests/fake_hip/rule_const_check.cpp).
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

// ------------------------------------------------------------ compiled rules
// A rule known at compile time needs no coefficient words: v_bitop3_b32 takes
// its truth table as an immediate, so the rule becomes the immediates of one
// fixed circuit over the vertical adders' outputs.  With S = o + 2co + 2p + 4q
// (the 9-sum including the cell, 0..9 for every (o, co, p, q)) the result is
//   alive ? survive[S-1] : birth[S]
// computed as four tables over (co, p, q), one per (alive, o), and three 0xCA
// selects by o, o and alive: 4 adders + 4 tables + 3 selects = 11 bitop3 per
// word for every rule, one AND more under a column mask.  The two inputs no
// board produces (a live cell with S = 0, a dead cell with S = 9) read 0.
struct RuleConst {
    uint32_t tt[2][2];   // tt[alive][o]: the truth table over a = co, b = p, c = q
};

constexpr uint32_t rule_const_tt(uint32_t birth, uint32_t survive, int alive, int o) {
    uint32_t t = 0;
    for (int i = 0; i < 8; ++i) {
        const int S = o + 2 * ((i >> 2) & 1) + 2 * ((i >> 1) & 1) + 4 * (i & 1);
        const uint32_t f = alive ? (S ? (survive >> (S - 1)) & 1u : 0u) : ((birth & kRuleBits) >> S) & 1u;
        t |= f << i;
    }
    return t;
}

constexpr RuleConst rule_const(uint32_t birth, uint32_t survive) {
    return RuleConst{{{rule_const_tt(birth, survive, 0, 0), rule_const_tt(birth, survive, 0, 1)},
                      {rule_const_tt(birth, survive, 1, 0), rule_const_tt(birth, survive, 1, 1)}}};
}

// rule_bitop3 with the table as a value: host code only (the check program
// evaluates the synthesised immediates of every rule through it).
inline uint32_t rule_bitop3_rt(uint32_t tt, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i)
        if ((tt >> i) & 1) r |= ((i & 4) ? a : ~a) & ((i & 2) ? b : ~b) & ((i & 1) ? c : ~c);
    return r;
}

// The circuit of rule_const_bits below over runtime immediates (host only).
inline uint32_t rule_const_eval(const RuleConst &C, bool masked, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                uint32_t c0, uint32_t c1, uint32_t alive, uint32_t mask) {
    const uint32_t o = rule_bitop3_rt(0x96, a0, b0, c0);
    const uint32_t co = rule_bitop3_rt(0xE8, a0, b0, c0);
    const uint32_t p = rule_bitop3_rt(0x96, a1, b1, c1);
    const uint32_t q = rule_bitop3_rt(0xE8, a1, b1, c1);
    const uint32_t d0 = rule_bitop3_rt(C.tt[0][0], co, p, q), d1 = rule_bitop3_rt(C.tt[0][1], co, p, q);
    const uint32_t l0 = rule_bitop3_rt(C.tt[1][0], co, p, q), l1 = rule_bitop3_rt(C.tt[1][1], co, p, q);
    const uint32_t D = rule_bitop3_rt(0xCA, o, d1, d0);
    const uint32_t A = rule_bitop3_rt(0xCA, o, l1, l0);
    const uint32_t r = rule_bitop3_rt(0xCA, alive, A, D);
    return masked ? (r & mask) : r;
}

// The compiled stage, on the life_bits arguments.
template <uint32_t BIRTH, uint32_t SURVIVE, bool MASKED>
GOL_RULE_HD uint32_t rule_const_bits(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t c0, uint32_t c1,
                                     uint32_t alive, uint32_t mask) {
    static_assert(!((BIRTH | SURVIVE) & ~kRuleBits) && !(BIRTH & 1u), "not a rule (bits above 8, or B0)");
    constexpr RuleConst C = rule_const(BIRTH, SURVIVE);
    const uint32_t o = rule_bitop3<0x96>(a0, b0, c0);    // vertical adders, as life_bits
    const uint32_t co = rule_bitop3<0xE8>(a0, b0, c0);
    const uint32_t p = rule_bitop3<0x96>(a1, b1, c1);
    const uint32_t q = rule_bitop3<0xE8>(a1, b1, c1);
    const uint32_t d0 = rule_bitop3<(int)C.tt[0][0]>(co, p, q), d1 = rule_bitop3<(int)C.tt[0][1]>(co, p, q);
    const uint32_t l0 = rule_bitop3<(int)C.tt[1][0]>(co, p, q), l1 = rule_bitop3<(int)C.tt[1][1]>(co, p, q);
    const uint32_t D = rule_bitop3<0xCA>(o, d1, d0);     // o ? d1 : d0
    const uint32_t A = rule_bitop3<0xCA>(o, l1, l0);
    const uint32_t r = rule_bitop3<0xCA>(alive, A, D);   // alive ? A : D
    return MASKED ? (r & mask) : r;
}

// Masks from the digits of B/S notation: rule_mask("36") = B36.
constexpr uint32_t rule_mask(const char *digits) {
    uint32_t m = 0;
    for (; *digits; ++digits) m |= 1u << (*digits - '0');
    return m;
}

// The rules with kernels of their own (gol_kernels.hip, bit_crule_kernel): the
// one list that the kernels, rule_compiled_index and gol_compiled_rule expand.
// B3/S23 is not on it: it has its tuned kernels.
#define GOL_COMPILED_RULES(X)                      \
    X("HighLife", "36", "23")                      \
    X("Day & Night", "3678", "34678")              \
    X("Seeds", "2", "")                            \
    X("Life without Death", "3", "012345678")      \
    X("Replicator", "1357", "1357")                \
    X("2x2", "36", "125")                          \
    X("Maze", "3", "12345")                        \
    X("DryLife", "37", "23")                       \
    X("Pedestrian Life", "38", "23")               \
    X("Diamoeba", "35678", "5678")                 \
    X("Morley", "368", "245")                      \
    X("Anneal", "4678", "35678")

struct CompiledRule {
    const char *name;
    uint32_t birth, survive;
};
#define GOL_COMPILED_RULE_ENTRY(name, b, s) {name, rule_mask(b), rule_mask(s)},
constexpr CompiledRule kCompiledRules[] = {GOL_COMPILED_RULES(GOL_COMPILED_RULE_ENTRY)};
#undef GOL_COMPILED_RULE_ENTRY
constexpr int kCompiledRuleCount = (int)(sizeof(kCompiledRules) / sizeof(kCompiledRules[0]));

// Index of a rule on the list, -1 when it is not listed.
inline int rule_compiled_index(uint32_t birth, uint32_t survive) {
    for (int i = 0; i < kCompiledRuleCount; ++i)
        if (kCompiledRules[i].birth == birth && kCompiledRules[i].survive == survive) return i;
    return -1;
}

} // namespace gol
