// Stand-alone proof of the board-to-board copy's row routine
// (mpi_amd/csrc/gol_copy.h, copy_row<GS, GD>) against the per-cell definition:
// destination storage column dpc0 + j becomes op(old value, source storage column
// spc0 + j) for 0 <= j < ncols, columns >= active_cols are stored as 0, no other
// cell of the destination row changes and the source row does not change.
// For all 9 pairs (GS, GD) of {byte, 2-word groups, 4-word groups} and all 3 ops:
//  - every relative shift d = dpc0 - spc0 in -160 .. 160 (every residue mod 32,
//    multiples of 32 and of 128 for the direct path, more than one unit crossing
//    either way);
//  - run lengths 1, 31, 32, 33, 127, 128, 129 and 300 from source columns 1, 37 and
//    130 (runs that start and end inside a unit, in the first unit of the row too);
//  - active_cols beyond the row, in the middle of the run and at its first column;
//  - one row as source and destination with disjoint runs that share units.
// Built with -fsanitize=address,undefined by __graft_entry__.build(); prints "ok"
// (tests/test_copy_cpu.py).  Rows are built from the layout's own definition
// (include/golhip.h: column 32G·g + G·j + w in word G·g + w, bit j), not with the
// runtime's helpers, and both rows are allocated exactly to the last unit their
// run touches: a unit read or written outside the run's own is AddressSanitizer's
// to find (before the first unit too: the runs from column 1 reach below unit 0).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "gol_copy.h"

using namespace gol;

namespace {
constexpr int kRowCols = 768;   // storage columns of a test row (whole units for every layout)

// units [0, nunits) of the row that holds `cells`
template <int G>
std::vector<uint32_t> store_row(const std::vector<uint8_t> &cells, int64_t nunits) {
    std::vector<uint32_t> row(nunits * DigestUnit<G>::WORDS, 0u);
    for (int64_t p = 0; p < nunits * DigestUnit<G>::COLS; ++p) {
        if (G == 0) {
            reinterpret_cast<uint8_t *>(row.data())[p] = cells[p];
        } else if (cells[p]) {
            const int64_t g = p / (32 * G), j = (p % (32 * G)) / G, w = p % G;
            row[G * g + w] |= 1u << j;
        }
    }
    return row;
}

template <int G>
std::vector<uint8_t> load_row(const std::vector<uint32_t> &row) {
    std::vector<uint8_t> cells(row.size() / DigestUnit<G>::WORDS * DigestUnit<G>::COLS);
    for (size_t p = 0; p < cells.size(); ++p) {
        if (G == 0) {
            cells[p] = reinterpret_cast<const uint8_t *>(row.data())[p];
        } else {
            const size_t g = p / (32 * G), j = (p % (32 * G)) / G, w = p % G;
            cells[p] = (row[G * g + w] >> j) & 1u;
        }
    }
    return cells;
}

uint8_t apply(int op, uint8_t old, uint8_t s) { return op == kCopyOr ? old | s : op == kCopyXor ? old ^ s : s; }

template <int GS, int GD>
long check_pair(std::mt19937_64 &rng) {
    long cases = 0;
    std::vector<uint8_t> scells(kRowCols), dcells(kRowCols);
    for (auto &c : scells) c = rng() % 2 == 0;
    for (auto &c : dcells) c = rng() % 2 == 0;
    for (int spc0 : {1, 37, 130})
        for (int n : {1, 31, 32, 33, 127, 128, 129, 300}) {
            const std::vector<uint32_t> src = store_row<GS>(scells, (spc0 + n - 1) / DigestUnit<GS>::COLS + 1);
            for (int d = -160; d <= 160; ++d) {
                const int dpc0 = spc0 + d;
                if (dpc0 < 0) continue;
                const int64_t dunits = (dpc0 + n - 1) / DigestUnit<GD>::COLS + 1;
                const std::vector<uint32_t> dst0 = store_row<GD>(dcells, dunits);
                for (int op : {kCopyReplace, kCopyOr, kCopyXor})
                    for (int64_t active : {(int64_t)kRowCols, (int64_t)dpc0 + n / 2, (int64_t)dpc0}) {
                        std::vector<uint32_t> tgt = dst0, s = src;
                        copy_row<GS, GD>(s.data(), spc0, tgt.data(), dpc0, n, active, op);
                        std::vector<uint8_t> exp(dcells.begin(), dcells.begin() + dunits * DigestUnit<GD>::COLS);
                        for (int c = 0; c < n; ++c)
                            exp[dpc0 + c] = dpc0 + c < active ? apply(op, dcells[dpc0 + c], scells[spc0 + c]) : 0;
                        if (load_row<GD>(tgt) != exp || s != src) {
                            std::printf("MISMATCH GS=%d GD=%d op=%d d=%d spc0=%d ncols=%d active=%lld\n", GS, GD, op, d,
                                        spc0, n, (long long)active);
                            return -1;
                        }
                        ++cases;
                    }
            }
        }
    return cases;
}

// one row as source and destination: disjoint runs that share units
template <int G>
long check_same_row(std::mt19937_64 &rng) {
    long cases = 0;
    std::vector<uint8_t> cells(kRowCols);
    for (auto &c : cells) c = rng() % 2 == 0;
    const std::vector<uint32_t> row0 = store_row<G>(cells, kRowCols / DigestUnit<G>::COLS);
    for (int spc0 : {5, 100, 333})
        for (int n : {1, 20, 45, 128})
            for (int dpc0 : {spc0 + n, spc0 + n + 1, spc0 + n + 31, spc0 + n + 128, spc0 - n, spc0 - n - 33, 0})
                for (int op : {kCopyReplace, kCopyOr, kCopyXor}) {
                    if (dpc0 < 0 || (dpc0 < spc0 + n && spc0 < dpc0 + n)) continue;
                    std::vector<uint32_t> row = row0;
                    copy_row<G, G>(row.data(), spc0, row.data(), dpc0, n, kRowCols, op);
                    std::vector<uint8_t> exp = cells;
                    for (int c = 0; c < n; ++c) exp[dpc0 + c] = apply(op, cells[dpc0 + c], cells[spc0 + c]);
                    if (load_row<G>(row) != exp) {
                        std::printf("MISMATCH same row G=%d op=%d spc0=%d dpc0=%d ncols=%d\n", G, op, spc0, dpc0, n);
                        return -1;
                    }
                    ++cases;
                }
    return cases;
}
}  // namespace

int main() {
    std::mt19937_64 rng(13579);
    long total = 0;
    const long n[] = {check_pair<0, 0>(rng), check_pair<0, 2>(rng), check_pair<0, 4>(rng),
                      check_pair<2, 0>(rng), check_pair<2, 2>(rng), check_pair<2, 4>(rng),
                      check_pair<4, 0>(rng), check_pair<4, 2>(rng), check_pair<4, 4>(rng),
                      check_same_row<0>(rng), check_same_row<2>(rng), check_same_row<4>(rng)};
    for (long v : n) {
        if (v < 0) return 1;
        total += v;
    }
    std::printf("ok %ld cases\n", total);
    return 0;
}
