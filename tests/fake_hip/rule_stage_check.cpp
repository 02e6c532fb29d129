// Exhaustive host check of the rule stage (mpi_amd/csrc/gol_rule.h): for every
// valid (birth, survive) pair — 2^17: 8 birth bits, B0 excluded, and 9 survive
// bits — and every combination of the stage's seven input bits
// (a0, a1, b0, b1, c0, c1, alive), packed bit-parallel into four 32-bit words,
// the stage's result equals  alive ? survive >> n & 1 : birth >> n & 1  with n
// the neighbour count, under an all-ones column mask, and 0 under mask = 0.
// Combinations that no board produces (a live cell whose own row sum is 0, a
// dead cell whose own row sum is 3) are not compared.  Built with -fsanitize=address,undefined by build().
#include <cstdint>
#include <cstdio>

#include "gol_rule.h"

int main() {
    using namespace gol;
    // combination c (0..127): bit 0 a0, 1 a1, 2 b0, 3 b1, 4 c0, 5 c1, 6 alive; word c / 32, bit c % 32
    uint32_t in[7][4] = {};
    int nbr[128];
    for (int c = 0; c < 128; ++c) {
        for (int b = 0; b < 7; ++b)
            if ((c >> b) & 1) in[b][c / 32] |= 1u << (c % 32);
        const int ha = (c & 1) + 2 * ((c >> 1) & 1), hb = ((c >> 2) & 1) + 2 * ((c >> 3) & 1),
                  hc = ((c >> 4) & 1) + 2 * ((c >> 5) & 1), alive = (c >> 6) & 1;
        nbr[c] = ((alive && hb == 0) || (!alive && hb == 3)) ? -1 : ha + hb + hc - alive;
    }
    long checked = 0, bad = 0;
    for (uint32_t birth = 0; birth < 512; birth += 2)
        for (uint32_t survive = 0; survive < 512; ++survive) {
            if (!rule_valid(birth, survive)) {
                std::printf("rule_valid rejects B%#x S%#x\n", birth, survive);
                return 1;
            }
            const RuleTable T = rule_table(birth, survive);
            for (int w = 0; w < 4; ++w) {
                const uint32_t full = rule_bits<true>(T, in[0][w], in[1][w], in[2][w], in[3][w], in[4][w], in[5][w],
                                                      in[6][w], 0xffffffffu);
                const uint32_t plain = rule_bits<false>(T, in[0][w], in[1][w], in[2][w], in[3][w], in[4][w],
                                                        in[5][w], in[6][w], 0u);
                const uint32_t dead = rule_bits<true>(T, in[0][w], in[1][w], in[2][w], in[3][w], in[4][w], in[5][w],
                                                      in[6][w], 0u);
                if (dead != 0u) ++bad;
                for (int b = 0; b < 32; ++b) {
                    const int c = 32 * w + b, n = nbr[c];
                    if (n < 0) continue;
                    const uint32_t want = ((c >> 6) & 1) ? (survive >> n) & 1u : (birth >> n) & 1u;
                    ++checked;
                    if (((full >> b) & 1u) != want || ((plain >> b) & 1u) != want) {
                        if (++bad <= 10)
                            std::printf("mismatch: birth %#x survive %#x combination %d (n = %d): want %u\n", birth,
                                        survive, c, n, want);
                    }
                }
            }
        }
    if (rule_valid(1u, 0u) || rule_valid(1u << 9, 0u) || rule_valid(0u, 1u << 9)) {
        std::printf("rule_valid accepts B0 or a bit above 8\n");
        return 1;
    }
    std::printf("rule stage: %ld cases checked, %ld bad\n", checked, bad);
    return bad ? 1 : 0;
}
