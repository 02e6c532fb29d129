// Stand-alone host check of csrc/gol_rle.h (built with AddressSanitizer + UBSan by
// __graft_entry__.build(), run as a program by tests/test_rle_cpu.py).
//  - the row routines and the three passes (row pass, row scan, write pass) on host
//    memory, in one block and in blocks of 1 and 3 rows with the carries between them,
//    against an encoder written here cell by cell: hand-built rows (runs of 1 .. 1000,
//    runs across the word and span seams, all-live rows of 32 / 64 / 33 / 1 columns,
//    leading and inner empty rows, the all-dead window), rows of 2 passes + 33 columns,
//    random soups;
//  - the parser: every output cut into chunks of 1, 2, 7 and 4096 bytes and into row
//    blocks of 1, 5 and all rows must give the cells back; truncations at every byte
//    and every body byte replaced by each of "09 x$!" must end in success or in
//    (offset, reason), never in a sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gol_rle.h"

using namespace gol;

namespace {

struct Board {
    int64_t nrows, ncols;
    std::vector<uint8_t> cells;
    Board(int64_t r, int64_t c) : nrows(r), ncols(c), cells((size_t)(r * c), 0) {}
    uint8_t &at(int64_t r, int64_t c) { return cells[(size_t)(r * ncols + c)]; }
    uint8_t at(int64_t r, int64_t c) const { return cells[(size_t)(r * ncols + c)]; }
    void run(int64_t r, int64_t c0, int64_t n) {
        for (int64_t c = c0; c < c0 + n; ++c) at(r, c) = 1;
    }
    Board window(int64_t r0, int64_t c0, int64_t nr, int64_t nc) const {
        Board w(nr, nc);
        for (int64_t r = 0; r < nr; ++r)
            for (int64_t c = 0; c < nc; ++c) w.at(r, c) = at(r0 + r, c0 + c);
        return w;
    }
};

int failures = 0;
void expect(bool ok, const char *what, int64_t a = 0, int64_t b = 0) {
    if (ok) return;
    if (++failures <= 20) printf("FAIL %s (%lld, %lld)\n", what, (long long)a, (long long)b);
}

// the format's definition, cell by cell
std::string encode_cells(const Board &b) {
    const int L = 70 / (1 + (int)std::to_string(std::max<int64_t>({b.nrows, b.ncols, 1})).size());
    std::string out;
    int64_t index = 0, last = -1;
    auto token = [&](int64_t n, char tag) {
        if (n >= 2) out += std::to_string(n);
        out += tag;
        if (index % L == L - 1 || tag == '!') out += '\n';
        ++index;
    };
    for (int64_t r = 0; r < b.nrows; ++r) {
        int64_t end = b.ncols;
        while (end > 0 && !b.at(r, end - 1)) --end;
        if (!end) continue;
        const int64_t gap = last < 0 ? r : r - last;
        if (gap > 0) token(gap, '$');
        last = r;
        for (int64_t c = 0; c < end;) {
            int64_t e = c;
            while (e < end && b.at(r, e) == b.at(r, c)) ++e;
            token(e - c, b.at(r, c) ? 'o' : 'b');
            c = e;
        }
    }
    token(1, '!');
    return out;
}

std::vector<uint32_t> pack(const Board &b, int64_t *pitch_words) {
    const int64_t pw = (b.ncols + 31) / 32;
    std::vector<uint32_t> p((size_t)(b.nrows * pw), 0u);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(p.data());
    for (int64_t r = 0; r < b.nrows; ++r)
        for (int64_t c = 0; c < b.ncols; ++c)
            if (b.at(r, c)) bytes[r * pw * 4 + (c >> 3)] |= (uint8_t)(0x80u >> (c & 7));
    *pitch_words = pw;
    return p;
}

// the three passes, block after block, the carries on the "host"
std::string encode_passes(const Board &b, int64_t block_rows) {
    const int L = rle_line_tokens(b.nrows, b.ncols), D = rle_digits(std::max<int64_t>({b.nrows, b.ncols, 1}));
    int64_t pw = 0;
    const std::vector<uint32_t> packed = pack(b, &pw);
    std::string out;
    int64_t last_row = -1, tok = 0;
    for (int64_t r0 = 0; r0 < b.nrows; r0 += block_rows) {
        const int64_t nr = std::min(block_rows, b.nrows - r0);
        std::vector<uint32_t> ntok((size_t)nr), nraw((size_t)nr), dcount((size_t)nr);
        std::vector<int64_t> tix((size_t)nr), off((size_t)nr);
        RleRecord rec;
        const uint32_t *rows = packed.data() + r0 * pw;
        rle_row_pass_host(rows, pw, nr, b.ncols, ntok.data(), nraw.data());
        rle_row_scan_host(ntok.data(), nraw.data(), nr, r0, last_row, tok, L, dcount.data(), tix.data(), off.data(), &rec);
        expect(rec.bytes >= 0 && rec.bytes <= rle_rows_bound(nr, b.ncols, L, D), "block bytes within the bound", rec.bytes,
               rle_rows_bound(nr, b.ncols, L, D));
        std::vector<char> text((size_t)rec.bytes, '?');   // exactly the record's bytes: ASan sees a byte too many
        rle_write_pass_host(rows, pw, nr, b.ncols, ntok.data(), dcount.data(), tix.data(), off.data(), L, text.data());
        out.append(text.data(), text.size());
        last_row = rec.last_row;
        tok = rec.tokens;
    }
    out += "!\n";
    return out;
}

// the parser over `body`, fed in chunks, filling row blocks; the cells or (offset, reason)
struct Parsed {
    bool ok;
    int64_t offset;
    Board cells;
};
Parsed parse(const std::string &body, int64_t x, int64_t y, int64_t chunk, int64_t block_rows) {
    Parsed out{false, -1, Board(y, x)};
    RleParser ps(x, y, 0);
    const int64_t pitch = (x + 31) / 32 * 4;
    int64_t at = 0;
    auto pump = [&]() -> RleParser::Status {   // until the parser wants a block, ends or fails
        for (;;) {
            if (ps.done()) return RleParser::kDone;
            if (at >= (int64_t)body.size()) return ps.finish();
            const int64_t n = std::min<int64_t>(chunk, (int64_t)body.size() - at);
            std::vector<char> piece(body.begin() + at, body.begin() + at + n);   // a buffer of its own: no read past it
            int64_t used = 0;
            const RleParser::Status st = ps.feed(piece.data(), n, &used);
            expect(used >= 0 && used <= n, "feed consumes within its buffer", used, n);
            at += used;
            if (st != RleParser::kMore) return st;
        }
    };
    for (int64_t r0 = 0; r0 < y; r0 += block_rows) {
        const int64_t nr = std::min(block_rows, y - r0);
        std::vector<uint8_t> rows((size_t)(nr * pitch), 0);
        ps.set_block(rows.data(), pitch, r0, nr);
        const RleParser::Status st = pump();
        if (st == RleParser::kError) {
            out.offset = ps.error_offset();
            return out;
        }
        bool any = false;
        for (int64_t r = 0; r < nr; ++r)
            for (int64_t c = 0; c < x; ++c) {
                const uint8_t v = rows[(size_t)(r * pitch + (c >> 3))] >> (7 - (c & 7)) & 1;
                out.cells.at(r0 + r, c) = v;
                any = any || v;
            }
        expect(any == ps.live(), "live() tells whether the block holds a live cell", r0);
    }
    ps.set_block(nullptr, 0, y, 0);
    const RleParser::Status st = pump();
    if (st == RleParser::kError) {
        out.offset = ps.error_offset();
        return out;
    }
    expect(st == RleParser::kDone, "the parser ends at '!'");
    out.ok = true;
    return out;
}

int boards_checked = 0;
void check_board(const Board &b, bool mutate) {
    ++boards_checked;
    const std::string want = encode_cells(b);
    for (int64_t br : {b.nrows > 0 ? b.nrows : 1, (int64_t)1, (int64_t)3}) {
        const std::string got = encode_passes(b, br);
        expect(got == want, "passes == per-cell encoder", b.nrows, b.ncols);
    }
    size_t line = 0, longest = 0;
    for (char ch : want) {
        line = ch == '\n' ? 0 : line + 1;
        longest = std::max(longest, line);
    }
    expect(longest <= 70, "no line above 70 characters", (int64_t)longest);
    if (b.nrows == 0 || b.ncols == 0) return;
    for (int64_t chunk : {1, 2, 7, 4096})
        for (int64_t br : {(int64_t)1, (int64_t)5, b.nrows}) {
            if (want.size() > 100000 && chunk < 7) continue;   // (the long rows: the big chunks only)
            const Parsed p = parse(want, b.ncols, b.nrows, chunk, br);
            expect(p.ok && p.cells.cells == b.cells, "parse(encode) gives the cells back", chunk, br);
        }
    if (!mutate) return;
    for (size_t cut = 0; cut < want.size(); ++cut) {
        const Parsed p = parse(want.substr(0, cut), b.ncols, b.nrows, 7, 5);
        const bool after_bang = cut > 0 && want.find('!') < cut;
        expect(p.ok == after_bang && (p.ok || p.offset == (int64_t)cut), "a truncation ends at its last byte", (int64_t)cut,
               p.offset);
    }
    for (size_t i = 0; i < want.size(); ++i)
        for (char ch : std::string("09 x$!")) {
            std::string m = want;
            m[i] = ch;
            const Parsed p = parse(m, b.ncols, b.nrows, 2, 1);
            expect(p.ok || (p.offset >= 0 && p.offset <= (int64_t)m.size()), "a mutation ends in success or an offset",
                   (int64_t)i, p.offset);
            if (ch == 'x' && i < want.find('!')) expect(!p.ok && p.offset == (int64_t)i, "an alien byte is reported where it is", (int64_t)i, p.offset);
        }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

}  // namespace

int main() {
    // lane routines
    expect(rle_digits(0) == 1 && rle_digits(9) == 1 && rle_digits(10) == 2 && rle_digits(2147483648ll) == 10, "digits");
    expect(rle_token_bytes(1) == 1 && rle_token_bytes(2) == 2 && rle_token_bytes(1000) == 5, "token bytes");
    expect(rle_line_tokens(9, 36) == 23 && rle_line_tokens(131072, 131072) == 10 && rle_line_tokens(0, 0) == 35, "L");
    expect(rle_newlines(0, 23, 23) == 1 && rle_newlines(22, 1, 23) == 1 && rle_newlines(23, 22, 23) == 0, "newlines");
    {
        char t[16];
        expect(rle_put_token(t, 1, 'o', false) == 1 && t[0] == 'o', "token o");
        expect(rle_put_token(t, 1000, 'b', true) == 6 && std::string(t, 6) == "1000b\n", "token 1000b");
        expect(rle_transitions(0x80000001u, 0u) == 0x80000003u && rle_transitions(1u, 0x80000000u) == 2u, "transitions");
    }
    // the hand-built board: 40 x 2100
    Board h(40, 2100);
    {
        int64_t c = 3;
        for (int64_t n : {1, 2, 9, 10, 99, 100, 999}) h.run(3, c, n), c += n + 2;   // rows 0..2 empty: a leading 3$
        h.run(4, 5, 1000);
        for (int64_t seam : {32, 64, 128, 2048}) h.run(5, seam - 1, 2);
        h.run(6, 0, 7);                 // live from column 0
        h.at(7, 2099) = 1;              // live only in its last column
        h.run(8, 0, 2100);              // all live
        h.run(10, 500, 3);              // a gap of 1 empty row
        h.run(13, 31, 1);               // 2
        h.run(24, 0, 33);               // 10
        h.run(36, 2047, 53);            // 11
        h.at(39, 2099) = 1;             // the last row and column
    }
    check_board(h, false);
    for (int64_t n : {32, 64, 33, 1}) check_board(h.window(8, 0, 1, n), true);
    check_board(h.window(0, 0, 3, 64), false);         // all dead: "!"
    check_board(h.window(3, 1, 37, 131), false);
    check_board(h.window(5, 31, 9, 96), false);
    check_board(h.window(0, 0, 8, 40), true);
    check_board(h.window(20, 2040, 20, 60), true);     // a single live cell at the window's last row and column
    check_board(Board(0, 0), false);
    check_board(Board(0, 5), false);
    check_board(Board(5, 0), false);
    // rows of two workgroup passes and 33 columns
    {
        Board l(3, 2 * kRlePassCols + 33);
        for (int64_t c = 0; c < l.ncols; ++c) l.at(0, c) = rnd() & 1;
        l.run(1, 32760, 16);
        l.at(2, 0) = 1;
        l.at(2, l.ncols - 1) = 1;
        check_board(l, false);
        Board full(1, kRlePassCols);   // a transition at position ncols, in a word the row does not have
        full.run(0, 0, full.ncols);
        check_board(full, false);
    }
    // soups
    for (int i = 0; i < 60; ++i) {
        const int64_t nr = 1 + rnd() % 12, nc = 1 + rnd() % (i % 3 ? 200 : 700);
        const uint32_t p = (uint32_t[]){0u, 1u << 20, 1u << 28, 1u << 30, 3u << 30, 0xffffffffu}[i % 6];
        Board s(nr, nc);
        for (auto &v : s.cells) v = ((uint64_t)rnd() << 1) < p || p == 0xffffffffu;
        check_board(s, nc < 40 && nr < 5);
    }
    // the header line
    {
        int64_t x, y, ra, rl, body;
        const std::string a = "#C a comment\n#CXRLE Pos=3,4\nx = 36, y = 9, rule = B3/S23\nbo!";
        expect(rle_header_scan(a.data(), (int64_t)a.size(), true, &x, &y, &ra, &rl, &body) == 0 && x == 36 && y == 9 &&
                   a.substr((size_t)ra, (size_t)rl) == "B3/S23" && a.substr((size_t)body) == "bo!", "header");
        const std::string b = "x=3,y=2\n";
        expect(rle_header_scan(b.data(), (int64_t)b.size(), true, &x, &y, &ra, &rl, &body) == 0 && x == 3 && y == 2 &&
                   rl == 0 && body == 8, "header with free spacing");
        for (size_t cut = 0; cut < a.size(); ++cut) {   // a stream: every prefix asks for more or is complete
            const int r = rle_header_scan(a.data(), (int64_t)cut, false, &x, &y, &ra, &rl, &body);
            expect(r == (cut < a.size() - 3 ? 1 : 0), "header prefix", (int64_t)cut, r);
        }
        const std::string bad = "x = 3, z = 2\n";
        expect(rle_header_scan(bad.data(), (int64_t)bad.size(), true, &x, &y, &ra, &rl, &body) == -1 && body == 7,
               "malformed header offset", body);
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok: %d boards\n", boards_checked);
    return 0;
}
