// Stand-alone proof of the digest's row routine (mpi_amd/csrc/gol_digest.h): the
// de-interleave of 2- and 4-word groups, the byte pack, the window masks and the
// funnel shift, against the per-cell definition
//   Σ A_i(r) · B_i(c >> 5) · 2^(c & 31) over the live cells.
// Built with -fsanitize=address,undefined by __graft_entry__.build(); prints
// "ok" (tests/test_digest_cpu.py).  Rows are built from the layout's own
// definition (include/golhip.h: column 32G·g + G·j + w in word G·g + w, bit j),
// not with the runtime's helpers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gol_digest.h"

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

template <int G>
long check_layout(std::mt19937_64 &rng) {
    long cases = 0;
    for (int rep = 0; rep < 2; ++rep) {
        std::vector<uint8_t> cells(kRowCols);
        const unsigned density = rep == 0 ? 2 : 1;   // half live, all live
        for (auto &c : cells) c = density == 1 ? 1 : (rng() % density == 0);
        const std::vector<uint32_t> row = store_row<G>(cells);
        for (int d = -63; d <= 63; ++d)
            for (int pc0 : {0, 1, 31, 33, 64, 97, 127, 129, 300}) {
                const int64_t lc0 = (int64_t)pc0 + d + (rep == 1 ? 4096 : 0);
                if (lc0 < 0) continue;
                for (int n = 1; n <= 200; ++n) {
                    uint64_t got[2], want[2] = {0, 0};
                    digest_row<G>(row.data(), pc0, lc0, n, got);
                    for (int c = 0; c < n; ++c)
                        if (cells[pc0 + c])
                            for (int i = 0; i < 2; ++i)
                                want[i] += digest_B(i, (lc0 + c) >> 5) << ((lc0 + c) & 31);
                    if (got[0] != want[0] || got[1] != want[1]) {
                        std::printf("MISMATCH G=%d shift=%d pc0=%d ncols=%d: %016llx %016llx, want %016llx %016llx\n", G,
                                    d, pc0, n, (unsigned long long)got[0], (unsigned long long)got[1],
                                    (unsigned long long)want[0], (unsigned long long)want[1]);
                        return -1;
                    }
                    ++cases;
                }
            }
    }
    return cases;
}

// one live cell through the row routine and A: the issue's known answers
template <int G>
bool known(int64_t r, int64_t c, uint64_t d0, uint64_t d1) {
    std::vector<uint8_t> cells(kRowCols, 0);
    cells[c] = 1;
    const std::vector<uint32_t> row = store_row<G>(cells);
    uint64_t sum[2];
    digest_row<G>(row.data(), 0, 0, kRowCols, sum);
    return digest_A(0, r) * sum[0] == d0 && digest_A(1, r) * sum[1] == d1;
}
}  // namespace

int main() {
    if (digest_sm(0) != 0xE220A8397B1DCDAFull) {
        std::printf("MISMATCH splitmix64(0)\n");
        return 1;
    }
    std::mt19937_64 rng(12345);
    const long n0 = check_layout<0>(rng), n2 = check_layout<2>(rng), n4 = check_layout<4>(rng);
    if (n0 < 0 || n2 < 0 || n4 < 0) return 1;
    bool k = true;
    k = k && known<0>(0, 0, 0x30dfcfac066b1a81ull, 0x8bd9e2c2a0c0adadull);
    k = k && known<2>(0, 0, 0x30dfcfac066b1a81ull, 0x8bd9e2c2a0c0adadull);
    k = k && known<4>(0, 0, 0x30dfcfac066b1a81ull, 0x8bd9e2c2a0c0adadull);
    k = k && known<0>(3, 70, 0xce34d829b13d1840ull, 0xa18d6f5a3f8398c0ull);
    k = k && known<2>(3, 70, 0xce34d829b13d1840ull, 0xa18d6f5a3f8398c0ull);
    k = k && known<4>(3, 70, 0xce34d829b13d1840ull, 0xa18d6f5a3f8398c0ull);
    if (!k) {
        std::printf("MISMATCH known answers\n");
        return 1;
    }
    std::printf("ok %ld cases\n", n0 + n2 + n4);
    return 0;
}
