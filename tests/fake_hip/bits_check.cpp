// Stand-alone proof of the packed-bit row routines (mpi_amd/csrc/gol_bits.h)
// against the per-cell definition: window column j of a packed row is bit
// 7 - (j & 7) of byte j >> 3.  For G = 0, 2, 4:
//  - bits_interleave<G> undoes digest_linear<G> on every single-cell unit and on
//    10^4 random units;
//  - bits_get_row / bits_put_row for every column shift 0 .. 31 with negative and
//    positive word offsets, run lengths 1 .. 33, 63 .. 65, 127 .. 129, 255 .. 257
//    and 300: get ORs exactly the run's cells into a cleared row (and leaves
//    foreign bits of a pre-filled row alone); put changes exactly the run's
//    cells, ignores every bit of the packed row outside the run, stores columns
//    >= active_cols as 0; get after put returns the input;
//  - bits_out_word against the byte/bit definition.
// Built with -fsanitize=address,undefined by __graft_entry__.build(); prints
// "ok" (tests/test_bits_cpu.py).  Rows are built from the layout's own
// definition (include/golhip.h: column 32G·g + G·j + w in word G·g + w, bit j),
// not with the runtime's helpers; packed rows have exact sizes, so a word
// touched outside [first, last] is AddressSanitizer's to find.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gol_bits.h"

using namespace gol;

namespace {
constexpr int kRowCols = 768;   // storage columns of a test row (whole units for every layout)

template <int G>
std::vector<uint32_t> store_row(const std::vector<uint8_t> &cells) {
    std::vector<uint32_t> row(G ? kRowCols / 32 : kRowCols / 4, 0u);
    for (int p = 0; p < kRowCols; ++p) {
        if (G == 0) {
            reinterpret_cast<uint8_t *>(row.data())[p] = cells[p];
        } else if (cells[p]) {
            const int g = p / (32 * G), j = (p % (32 * G)) / G, w = p % G;
            row[G * g + w] |= 1u << j;
        }
    }
    return row;
}

template <int G>
std::vector<uint8_t> load_row(const std::vector<uint32_t> &row) {
    std::vector<uint8_t> cells(kRowCols);
    for (int p = 0; p < kRowCols; ++p) {
        if (G == 0) {
            cells[p] = reinterpret_cast<const uint8_t *>(row.data())[p];
        } else {
            const int g = p / (32 * G), j = (p % (32 * G)) / G, w = p % G;
            cells[p] = (row[G * g + w] >> j) & 1u;
        }
    }
    return cells;
}

// the per-cell definition, on the bytes of a packed row
void set_bit(std::vector<uint32_t> &packed, int64_t j, int v) {
    uint8_t *b = reinterpret_cast<uint8_t *>(packed.data());
    const uint8_t m = (uint8_t)(1u << (7 - (j & 7)));
    b[j >> 3] = (uint8_t)(v ? b[j >> 3] | m : b[j >> 3] & ~m);
}
int get_bit(const std::vector<uint32_t> &packed, int64_t j) {
    return (reinterpret_cast<const uint8_t *>(packed.data())[j >> 3] >> (7 - (j & 7))) & 1;
}

template <int G>
bool check_interleave(std::mt19937_64 &rng) {
    typedef DigestUnit<G> U;
    auto round_trip = [](const uint32_t *x) {
        uint32_t L[U::NL], y[U::WORDS];
        digest_linear<G>(x, L);
        bits_interleave<G>(L, y);
        return std::memcmp(x, y, sizeof y) == 0;
    };
    for (int p = 0; p < U::COLS; ++p) {
        uint32_t x[U::WORDS] = {};
        if (G == 0) reinterpret_cast<uint8_t *>(x)[p] = 1;
        else x[p / 32] = 1u << (p % 32);   // every single bit of the unit's storage words
        if (!round_trip(x)) {
            std::printf("MISMATCH G=%d interleave of the single bit %d\n", G, p);
            return false;
        }
    }
    for (int rep = 0; rep < 10000; ++rep) {
        uint32_t x[U::WORDS];
        for (auto &v : x) v = G ? (uint32_t)rng() : (uint32_t)rng() & 0x01010101u;
        if (!round_trip(x)) {
            std::printf("MISMATCH G=%d interleave of random unit %d\n", G, rep);
            return false;
        }
    }
    return true;
}

template <int G>
long check_layout(std::mt19937_64 &rng) {
    if (!check_interleave<G>(rng)) return -1;
    long cases = 0;
    std::vector<int> lens;
    for (int n = 1; n <= 33; ++n) lens.push_back(n);
    for (int n : {63, 64, 65, 127, 128, 129, 255, 256, 257, 300}) lens.push_back(n);
    std::vector<uint8_t> cells(kRowCols), fresh(kRowCols);
    for (auto &c : cells) c = rng() % 2 == 0;
    for (auto &c : fresh) c = rng() % 2 == 0;
    const std::vector<uint32_t> row = store_row<G>(cells);
    // d = lc_rel0 - pc0: every shift with word offsets dq = -2 .. 1 (lc_rel0 >= 0 permitting)
    for (int d = -64; d <= 63; ++d)
        for (int pc0 : {0, 1, 31, 97, 128, 383})
            for (int n : lens) {
                const int64_t lc = (int64_t)pc0 + d;
                if (lc < 0) continue;
                const int64_t nw = bits_last_word(lc, n) + 1;
                auto bad = [&](const char *what) {
                    std::printf("MISMATCH G=%d %s shift=%d pc0=%d ncols=%d\n", G, what, d, pc0, n);
                    return -1L;
                };
                // get into a cleared row: the run's cells and nothing else
                std::vector<uint32_t> got(nw, 0u), want(nw, 0u);
                bits_get_row<G>(row.data(), pc0, lc, n, got.data());
                for (int c = 0; c < n; ++c) set_bit(want, lc + c, cells[pc0 + c]);
                if (got != want) return bad("get");
                // ... and it only ORs: foreign bits of a filled row stay
                std::vector<uint32_t> got1(nw, 0u);
                for (int64_t j = 0; j < 32 * nw; ++j)
                    if (j < lc || j >= lc + n) set_bit(got1, j, 1);
                std::vector<uint32_t> want1 = got1;
                bits_get_row<G>(row.data(), pc0, lc, n, got1.data());
                for (int c = 0; c < n; ++c) set_bit(want1, lc + c, cells[pc0 + c]);
                if (got1 != want1) return bad("get (or)");
                // put: packed input with every bit outside the run set (pad bits, other runs)
                for (int64_t active : {(int64_t)kRowCols, (int64_t)pc0 + n - 1, (int64_t)pc0 + n / 2, (int64_t)pc0}) {
                    std::vector<uint32_t> in(nw, ~0u);
                    for (int c = 0; c < n; ++c) set_bit(in, lc + c, fresh[pc0 + c]);
                    std::vector<uint32_t> tgt = row;
                    bits_put_row<G>(tgt.data(), pc0, lc, n, active, in.data());
                    std::vector<uint8_t> exp = cells;
                    for (int c = 0; c < n; ++c) exp[pc0 + c] = pc0 + c < active ? fresh[pc0 + c] : 0;
                    if (load_row<G>(tgt) != exp) return bad("put");
                    if (active == kRowCols) {
                        std::vector<uint32_t> back(nw, 0u), wantb(nw, 0u);
                        bits_get_row<G>(tgt.data(), pc0, lc, n, back.data());
                        for (int c = 0; c < n; ++c) set_bit(wantb, lc + c, fresh[pc0 + c]);
                        if (back != wantb) return bad("get after put");
                    }
                    ++cases;
                }
            }
    return cases;
}

bool check_out_word(std::mt19937_64 &rng) {
    for (int rep = 0; rep < 10000 + 32; ++rep) {
        const uint32_t c = rep < 32 ? 1u << rep : (uint32_t)rng();
        std::vector<uint32_t> want(1, 0u);
        for (int j = 0; j < 32; ++j) set_bit(want, j, (c >> j) & 1u);
        if (bits_out_word(c) != want[0] || bits_out_word(want[0]) != c) {
            std::printf("MISMATCH bits_out_word(%08x)\n", c);
            return false;
        }
    }
    return true;
}
}  // namespace

int main() {
    std::mt19937_64 rng(24680);
    if (!check_out_word(rng)) return 1;
    const long n0 = check_layout<0>(rng), n2 = check_layout<2>(rng), n4 = check_layout<4>(rng);
    if (n0 < 0 || n2 < 0 || n4 < 0) return 1;
    std::printf("ok %ld cases\n", n0 + n2 + n4);
    return 0;
}
