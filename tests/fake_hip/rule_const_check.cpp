// Exhaustive host check of the compiled-rule stage (mpi_amd/csrc/gol_rule.h).
//  1. The synthesiser: for every valid (birth, survive) pair — 2^17 — the
//     immediates of rule_const(), evaluated through the emulated bitop3 with
//     runtime tables (rule_const_eval), over every combination of the stage's
//     seven input bits (a0, a1, b0, b1, c0, c1, alive), packed bit-parallel
//     into four 32-bit words: the result equals
//     alive ? survive >> n & 1 : birth >> n & 1  (n the neighbour count, so
//     S = n + alive) and equals rule_bits, under an all-ones column mask, and
//     is 0 under mask = 0.
//  2. The template: for every rule of GOL_COMPILED_RULES, the instantiation
//     rule_const_bits<BIRTH, SURVIVE, MASKED> itself gives the same.
// Combinations that no board produces (a live cell whose own row sum is 0, a
// dead cell whose own row sum is 3) are not compared.  Also: the list's masks
// are rules, none is B3/S23, none is listed twice, and rule_compiled_index
// finds each and nothing else.  Built with -fsanitize=address,undefined by build().
#include <cstdint>
#include <cstdio>

#include "gol_rule.h"

using namespace gol;

static uint32_t in[7][4];
static int nbr[128];
static long checked_tpl = 0, bad = 0;

template <uint32_t BIRTH, uint32_t SURVIVE>
static void check_template(const char *name) {
    for (int w = 0; w < 4; ++w) {
        const uint32_t full = rule_const_bits<BIRTH, SURVIVE, true>(in[0][w], in[1][w], in[2][w], in[3][w], in[4][w],
                                                                    in[5][w], in[6][w], 0xffffffffu);
        const uint32_t plain = rule_const_bits<BIRTH, SURVIVE, false>(in[0][w], in[1][w], in[2][w], in[3][w], in[4][w],
                                                                      in[5][w], in[6][w], 0u);
        const uint32_t dead = rule_const_bits<BIRTH, SURVIVE, true>(in[0][w], in[1][w], in[2][w], in[3][w], in[4][w],
                                                                    in[5][w], in[6][w], 0u);
        const uint32_t generic = rule_bits<false>(rule_table(BIRTH, SURVIVE), in[0][w], in[1][w], in[2][w], in[3][w],
                                                  in[4][w], in[5][w], in[6][w], 0u);
        if (dead != 0u) ++bad;
        for (int b = 0; b < 32; ++b) {
            const int c = 32 * w + b, n = nbr[c];
            if (n < 0) continue;
            const uint32_t want = ((c >> 6) & 1) ? (SURVIVE >> n) & 1u : (BIRTH >> n) & 1u;
            ++checked_tpl;
            if (((full >> b) & 1u) != want || ((plain >> b) & 1u) != want || ((generic >> b) & 1u) != want) {
                if (++bad <= 10) std::printf("template mismatch: %s combination %d (n = %d): want %u\n", name, c, n, want);
            }
        }
    }
}

int main() {
    // combination c (0..127): bit 0 a0, 1 a1, 2 b0, 3 b1, 4 c0, 5 c1, 6 alive; word c / 32, bit c % 32
    for (int c = 0; c < 128; ++c) {
        for (int b = 0; b < 7; ++b)
            if ((c >> b) & 1) in[b][c / 32] |= 1u << (c % 32);
        const int ha = (c & 1) + 2 * ((c >> 1) & 1), hb = ((c >> 2) & 1) + 2 * ((c >> 3) & 1),
                  hc = ((c >> 4) & 1) + 2 * ((c >> 5) & 1), alive = (c >> 6) & 1;
        nbr[c] = ((alive && hb == 0) || (!alive && hb == 3)) ? -1 : ha + hb + hc - alive;
    }
    long checked = 0;
    for (uint32_t birth = 0; birth < 512; birth += 2)
        for (uint32_t survive = 0; survive < 512; ++survive) {
            const RuleConst C = rule_const(birth, survive);
            const RuleTable T = rule_table(birth, survive);
            for (int a = 0; a < 2; ++a)
                for (int o = 0; o < 2; ++o)
                    if (C.tt[a][o] > 0xffu) {
                        std::printf("immediate above 8 bits: birth %#x survive %#x\n", birth, survive);
                        return 1;
                    }
            for (int w = 0; w < 4; ++w) {
                const uint32_t full = rule_const_eval(C, true, in[0][w], in[1][w], in[2][w], in[3][w], in[4][w],
                                                      in[5][w], in[6][w], 0xffffffffu);
                const uint32_t plain = rule_const_eval(C, false, in[0][w], in[1][w], in[2][w], in[3][w], in[4][w],
                                                       in[5][w], in[6][w], 0u);
                const uint32_t dead = rule_const_eval(C, true, in[0][w], in[1][w], in[2][w], in[3][w], in[4][w],
                                                      in[5][w], in[6][w], 0u);
                const uint32_t generic = rule_bits<true>(T, in[0][w], in[1][w], in[2][w], in[3][w], in[4][w],
                                                         in[5][w], in[6][w], 0xffffffffu);
                if (dead != 0u) ++bad;
                for (int b = 0; b < 32; ++b) {
                    const int c = 32 * w + b, n = nbr[c];
                    if (n < 0) continue;
                    const uint32_t want = ((c >> 6) & 1) ? (survive >> n) & 1u : (birth >> n) & 1u;
                    ++checked;
                    if (((full >> b) & 1u) != want || ((plain >> b) & 1u) != want || ((generic >> b) & 1u) != want) {
                        if (++bad <= 10)
                            std::printf("mismatch: birth %#x survive %#x combination %d (n = %d): want %u\n", birth,
                                        survive, c, n, want);
                    }
                }
            }
        }
    // the list: every entry a rule, none B3/S23, none twice; the lookup finds each at its index
    int listed = 0;
#define CHECK_LISTED(name, b, s)                                                                  \
    {                                                                                             \
        constexpr uint32_t B = rule_mask(b), S = rule_mask(s);                                    \
        check_template<B, S>(name);                                                               \
        if (!rule_valid(B, S) || (B == kLifeBirth && S == kLifeSurvive) ||                        \
            rule_compiled_index(B, S) != listed || kCompiledRules[listed].birth != B ||           \
            kCompiledRules[listed].survive != S) {                                                \
            std::printf("bad list entry %d (%s)\n", listed, name);                                \
            ++bad;                                                                                \
        }                                                                                         \
        ++listed;                                                                                 \
    }
    GOL_COMPILED_RULES(CHECK_LISTED)
#undef CHECK_LISTED
    if (listed != kCompiledRuleCount || rule_compiled_index(kLifeBirth, kLifeSurvive) != -1 ||
        rule_compiled_index(1u << 1, 1u << 8) != -1 || rule_compiled_index(0u, 0u) != -1) {
        std::printf("rule_compiled_index: wrong count or a stand-in for an unlisted rule\n");
        ++bad;
    }
    std::printf("rule const: %ld synthesised cases checked, %ld template cases checked (%d rules), %ld bad\n", checked,
                checked_tpl, listed, bad);
    return bad ? 1 : 0;
}
