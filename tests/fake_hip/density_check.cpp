// Stand-alone proof of the density map's row routine (mpi_amd/csrc/gol_density.h)
// against the per-cell definition: tile column of logical column c is
// (c - col0) / tile_cols.  Every column shift s = 0 .. 31 with negative and
// positive word offsets dq, partial first and last units, tile widths 32 .. 160,
// window origins 0, 32 and 96; the path that counts a whole unit on its storage
// words (density_unit_whole) is taken wherever density_is_whole allows and is
// also checked directly against the general path.
// Built with -fsanitize=address,undefined by __graft_entry__.build(); prints
// "ok" (tests/test_density_cpu.py).  Rows are built from the layout's own
// definition (include/golhip.h: column 32G·g + G·j + w in word G·g + w, bit j),
// not with the runtime's helpers.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "gol_density.h"

using namespace gol;

namespace {
constexpr int kRowCols = 640;   // storage columns of a test row (whole units for every layout)

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

long whole_taken = 0;   // cases in which at least one unit took density_unit_whole

// would density_row take the whole-unit path for some unit of this run?
template <int G>
bool takes_whole(int64_t pc0, int64_t lc0, int64_t n, int64_t col0, int64_t tw) {
    typedef DigestUnit<G> U;
    const DigestShift h = digest_shift_of(pc0, lc0);
    for (int64_t q = pc0 / U::COLS; q <= (pc0 + n - 1) / U::COLS; ++q) {
        uint32_t mask[U::NL];
        int64_t tc[U::NL + 1];
        for (int t = 0; t < U::NL; ++t) mask[t] = digest_mask(U::NL * q + t, pc0, pc0 + n);
        for (int t = 0; t <= U::NL; ++t) tc[t] = density_tile_of(U::NL * q + h.dq + t, col0, tw);
        if (density_is_whole<G>(mask, h.s, tc)) return true;
    }
    return false;
}

template <int G>
long check_layout(std::mt19937_64 &rng) {
    long cases = 0;
    std::vector<int> lens;
    for (int n = 1; n <= 33; n += n < 4 ? 1 : 7) lens.push_back(n);
    for (int n : {31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 200, 255, 256, 257, 300}) lens.push_back(n);
    for (int rep = 0; rep < 2; ++rep) {
        std::vector<uint8_t> cells(kRowCols);
        for (auto &c : cells) c = rep == 1 ? 1 : (rng() % 2 == 0);   // half live, all live
        const std::vector<uint32_t> row = store_row<G>(cells);
        for (int d = -63; d <= 63; ++d)
            for (int pc0 : {0, 1, 31, 64, 97, 128, 300})
                for (int64_t col0 : {0, 32, 96})
                    for (int64_t tw : {32, 64, 96, 128, 160}) {
                        const int64_t lc0 = (int64_t)pc0 + d + (rep == 1 ? 4096 : 128);
                        if (lc0 < col0) continue;
                        for (int n : lens) {
                            const int64_t ntiles = (lc0 + n - col0 + tw - 1) / tw;
                            // exact sizes: a write past the last tile is AddressSanitizer's to find
                            std::vector<uint32_t> got(ntiles, 7u), want(ntiles, 7u);
                            density_row<G>(row.data(), pc0, lc0, n, col0, tw, got.data(), ntiles);
                            for (int c = 0; c < n; ++c) want[(lc0 + c - col0) / tw] += cells[pc0 + c];
                            if (got != want) {
                                std::printf("MISMATCH G=%d shift=%d pc0=%d ncols=%d col0=%d tile_cols=%d\n", G, d, pc0, n,
                                            (int)col0, (int)tw);
                                return -1;
                            }
                            whole_taken += takes_whole<G>(pc0, lc0, n, col0, tw);
                            ++cases;
                        }
                    }
    }
    // the whole-unit count against the general path under full masks, unit by unit
    for (int rep = 0; rep < 200; ++rep) {
        std::vector<uint8_t> cells(kRowCols);
        for (auto &c : cells) c = rng() % 3 == 0;
        const std::vector<uint32_t> row = store_row<G>(cells);
        const uint32_t full[4] = {~0u, ~0u, ~0u, ~0u};
        for (int q = 0; q < kRowCols / DigestUnit<G>::COLS; ++q) {
            uint32_t cnt[5] = {0, 0, 0, 0, 0};
            density_unit<G>(row.data() + q * DigestUnit<G>::WORDS, full, 0, cnt);
            if (density_unit_whole<G>(row.data() + q * DigestUnit<G>::WORDS) != cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4]) {
                std::printf("MISMATCH G=%d whole unit %d\n", G, q);
                return -1;
            }
        }
    }
    return cases;
}
}  // namespace

int main() {
    std::mt19937_64 rng(54321);
    const long n0 = check_layout<0>(rng);
    const long w0 = whole_taken;
    const long n2 = check_layout<2>(rng);
    const long w2 = whole_taken - w0;
    const long n4 = check_layout<4>(rng);
    const long w4 = whole_taken - w0 - w2;
    if (n0 < 0 || n2 < 0 || n4 < 0) return 1;
    if (w0 == 0 || w2 == 0 || w4 == 0) {
        std::printf("MISMATCH the whole-unit path was never taken (%ld %ld %ld)\n", w0, w2, w4);
        return 1;
    }
    std::printf("ok %ld cases, %ld through the whole-unit path\n", n0 + n2 + n4, whole_taken);
    return 0;
}
