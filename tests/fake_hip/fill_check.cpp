// Stand-alone proof of the random fill's row routine (mpi_amd/csrc/gol_fill.h)
// against the per-cell definition of include/golhip.h: X(r, c) is assembled cell by
// cell from all 32 planes (no plane skip, no bit slicing), and cell (r, c) is live
// iff X < T.  For G = 0, 2, 4:
//  - every T of {0, 1, 2^k (k = 0 .. 32), 2^32 - 1, 0x55555555, 3·2^29} with every
//    column shift 0 .. 31, runs that start and end inside a unit, and active_cols
//    above, inside and at the start of the run;
//  - the geometry of bits_check (shifts -64 .. 63 from six storage columns, run
//    lengths 1 .. 33, 63 .. 65, 127 .. 129, 255 .. 257, 300; four active_cols) with T
//    taking turns, on two rows and at global columns near 0 and above 2^33:
// fill_put_row gives exactly the definition's cells in the run, 0 at storage
// columns >= active_cols, and leaves every cell outside the run untouched.
// fill_word is also checked against the definition word by word.  Built with
// -fsanitize=address,undefined by __graft_entry__.build(); prints "ok"
// (tests/test_fill_cpu.py).  Rows are built from the layout's own definition
// (include/golhip.h: column 32G·g + G·j + w in word G·g + w, bit j).
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "gol_fill.h"

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

// the definition, written out on its own (splitmix64 included)
uint64_t sm(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t X_def(uint64_t seed, int64_t r, int64_t c) {
    const uint64_t K = sm(seed), w = (uint64_t)c >> 5;
    uint64_t x = 0;
    for (int i = 0; i < 32; ++i) {
        const uint64_t h = sm(sm(K + (uint64_t)r) + 16 * w + (uint64_t)(i >> 1));
        const uint32_t plane = i & 1 ? (uint32_t)(h >> 32) : (uint32_t)h;
        x += (uint64_t)((plane >> (c & 31)) & 1u) << i;
    }
    return x;
}
// X is independent of T: computed once per (row, column)
std::map<std::pair<int64_t, int64_t>, uint64_t> x_cache;
constexpr uint64_t kSeed = 0x0123456789abcdefull;
uint64_t X(int64_t r, int64_t c) {
    auto it = x_cache.find({r, c});
    if (it != x_cache.end()) return it->second;
    return x_cache[{r, c}] = X_def(kSeed, r, c);
}

std::vector<uint64_t> thresholds() {
    std::vector<uint64_t> t = {0};
    for (int k = 0; k <= 32; ++k) t.push_back(1ull << k);
    t.push_back((1ull << 32) - 1);
    t.push_back(0x55555555ull);
    t.push_back(3ull << 29);
    return t;
}

template <int G>
bool one_case(const std::vector<uint32_t> &row, const std::vector<uint8_t> &cells, int pc0, int64_t lc, int n,
              int64_t active, uint64_t T, int64_t r) {
    std::vector<uint32_t> tgt = row;
    fill_put_row<G>(tgt.data(), pc0, lc, n, active, fill_key(kSeed), T, r);
    std::vector<uint8_t> exp = cells;
    for (int c = 0; c < n; ++c) exp[pc0 + c] = pc0 + c < active ? X(r, lc + c) < T : 0;
    if (load_row<G>(tgt) == exp) return true;
    std::printf("MISMATCH G=%d pc0=%d lc=%lld ncols=%d active=%lld T=%llx row=%lld\n", G, pc0, (long long)lc, n,
                (long long)active, (unsigned long long)T, (long long)r);
    return false;
}

template <int G>
long check_layout(std::mt19937_64 &rng) {
    long cases = 0;
    const std::vector<uint64_t> Ts = thresholds();
    std::vector<uint8_t> cells(kRowCols);
    for (auto &c : cells) c = rng() % 2 == 0;
    const std::vector<uint32_t> row = store_row<G>(cells);
    const int64_t rows[2] = {0, 123456789012ll}, far = (1ll << 33) + 64;
    // every T: shifts 0 .. 31, runs that start and end inside a unit, active_cols above / inside / at the run
    for (uint64_t T : Ts)
        for (int s = 0; s < 32; ++s)
            for (int pc0 : {1, 97, 383})
                for (int n : {1, 31, 33, 129, 300}) {
                    const int64_t lc = pc0 + s + (s & 1 ? far : 0);
                    for (int64_t active : {(int64_t)kRowCols, (int64_t)pc0 + n / 2, (int64_t)pc0}) {
                        if (!one_case<G>(row, cells, pc0, lc, n, active, T, rows[s & 1])) return -1;
                        ++cases;
                    }
                }
    // the geometry of bits_check, T taking turns
    std::vector<int> lens;
    for (int n = 1; n <= 33; ++n) lens.push_back(n);
    for (int n : {63, 64, 65, 127, 128, 129, 255, 256, 257, 300}) lens.push_back(n);
    size_t turn = 0;
    for (int d = -64; d <= 63; ++d)
        for (int pc0 : {0, 1, 31, 97, 128, 383})
            for (int n : lens) {
                const int64_t lc = (int64_t)pc0 + d + (d & 2 ? far : 0);
                if (lc < 0) continue;
                for (int64_t active : {(int64_t)kRowCols, (int64_t)pc0 + n - 1, (int64_t)pc0 + n / 2, (int64_t)pc0}) {
                    if (!one_case<G>(row, cells, pc0, lc, n, active, Ts[turn++ % Ts.size()], rows[d & 1])) return -1;
                    ++cases;
                }
            }
    return cases;
}

// fill_word (the plane skip, bit-sliced) against the definition, word by word
bool check_words() {
    for (uint64_t T : thresholds())
        for (int64_t r : {(int64_t)0, (int64_t)77, (int64_t)123456789012ll})
            for (int64_t w : {(int64_t)0, (int64_t)1, (int64_t)36, (int64_t)((1ll << 28) + 2)}) {
                uint32_t want = 0;
                for (int j = 0; j < 32; ++j) want |= (uint32_t)(X(r, 32 * w + j) < T) << j;
                if (fill_word(fill_key(kSeed), T, r, w) != want) {
                    std::printf("MISMATCH fill_word T=%llx r=%lld w=%lld\n", (unsigned long long)T, (long long)r,
                                (long long)w);
                    return false;
                }
            }
    return true;
}
}  // namespace

int main() {
    std::mt19937_64 rng(13579);
    if (!check_words()) return 1;
    const long n0 = check_layout<0>(rng), n2 = check_layout<2>(rng), n4 = check_layout<4>(rng);
    if (n0 < 0 || n2 < 0 || n4 < 0) return 1;
    std::printf("ok %ld cases\n", n0 + n2 + n4);
    return 0;
}
