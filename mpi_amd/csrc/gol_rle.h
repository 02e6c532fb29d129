// gol_rle.h — RLE pattern text (gol_format_rle / gol_write_rle / gol_parse_rle /
// gol_read_rle, include/golhip.h).  The format is the one DESIGN.md §3 "RLE
// pattern files" fixes byte for byte:
//
//   x = <ncols>, y = <nrows>, rule = B<digits>/S<digits>\n
//   <tokens>!\n
//
// A token is an optional decimal count n >= 2 and a tag: b (dead run), o (live
// run), $ (end of row), ! (end of pattern).  A non-empty row contributes its
// maximal runs from column 0 up to its last live cell; a `$` token of count
// r_k - r_{k-1} stands before the tokens of the k-th non-empty row (count r_0
// before the first, when r_0 > 0).  Tokens are numbered in stream order and a
// '\n' follows every token whose index is L - 1 (mod L), L = 70 / (1 + D), D the
// decimal digits of max(nrows, ncols, 1); one more follows `!` unless it just got
// one.  Line breaks depend on token indices only, so prefix sums place every byte.
//
// The encoder reads PACKED rows (gol_bits.h: MSB-first bytes, one row of whole u32
// words per window row, pad bits 0), which launch_get_bits produces from every
// storage form.  Three passes, the launch boundaries being the only hand-off:
//   row pass   per row: token count, token bytes (no newlines)
//   row scan   per row: its `$` count, first token index, byte offset; block totals
//   write pass the row pass's traversal again, every token stored at its offset
// The per-lane pieces below are __host__ __device__: the kernels (gol_rle.hip)
// evaluate them per lane with workgroup scans in between, the rle_*_host routines
// evaluate the same pieces lane after lane, and the stand-alone host program
// (tests/fake_hip/rle_check.cpp) proves them against a per-cell encoder.
//
// A lane owns a SPAN of kRleSpanWords canonical words = 128 positions; a workgroup
// pass of 256 lanes covers 32768 positions.  Position p in 0 .. ncols is a
// TRANSITION when cell p differs from cell p - 1 (cells left of column 0 and from
// ncols on are dead), so positions fill ncols / 32 + 1 words: a row whose last
// cell is live has one at p = ncols.  A transition at p > 0 ends the run
// [prev, p), prev being the transition before it or 0: tag `o` when cell p is dead.
//
// The parser at the end of the file is host-only and has no HIP types.
#pragma once
#include <stdint.h>
#include <string.h>

#include "gol_bits.h"

namespace gol {

constexpr int kRleSpanWords = 4;                            // canonical words per lane
constexpr int kRleLanes = 256;                              // lanes per workgroup pass
constexpr int64_t kRlePassCols = 32LL * kRleSpanWords * kRleLanes;   // 32768 positions per pass
constexpr int64_t kRleMaxCount = 1LL << 31;                 // the largest count the parser reads

GOL_DIGEST_HD int rle_digits(int64_t n) {
    int d = 1;
    while (n >= 10) {
        n /= 10;
        ++d;
    }
    return d;
}
// bytes of a token of count n >= 1 (the count is omitted when it is 1)
GOL_DIGEST_HD int rle_token_bytes(int64_t n) { return n >= 2 ? rle_digits(n) + 1 : 1; }
// tokens per line
GOL_DIGEST_HD int rle_line_tokens(int64_t nrows, int64_t ncols) {
    int64_t m = nrows > ncols ? nrows : ncols;
    if (m < 1) m = 1;
    return 70 / (1 + rle_digits(m));
}
// newlines that follow the tokens [a, a + n)
GOL_DIGEST_HD int64_t rle_newlines(int64_t a, int64_t n, int L) { return (a + n) / L - a / L; }
// the most bytes the tokens of `nrows` rows of `ncols` cells can take, newlines included: a run of
// n cells costs at most n bytes, a row adds one `$` token, a newline follows every L-th token
GOL_DIGEST_HD int64_t rle_rows_bound(int64_t nrows, int64_t ncols, int L, int D) {
    return nrows * (ncols + 1 + D) + nrows * (ncols + 1) / L + 1;
}

// Stores a token (digits, tag, newline if asked) at dst; returns its bytes.
GOL_DIGEST_HD int rle_put_token(char *dst, int64_t n, char tag, bool newline) {
    int k = 0;
    if (n >= 2) {
        const int d = rle_digits(n);
        for (int i = d - 1; i >= 0; --i) {
            dst[i] = (char)('0' + n % 10);
            n /= 10;
        }
        k = d;
    }
    dst[k++] = tag;
    if (newline) dst[k++] = '\n';
    return k;
}

// Canonical word i of a packed row (bit j = column 32i + j); words past the row and
// the pad bits of its last word read as dead cells.
GOL_DIGEST_HD uint32_t rle_row_word(const uint32_t *packed, int64_t i, int64_t ncols) {
    if (i < 0 || 32 * i >= ncols) return 0u;
    uint32_t c = bits_out_word(packed[i]);
    if (ncols - 32 * i < 32) c &= (1u << (ncols - 32 * i)) - 1u;
    return c;
}
// transitions of a word: bit j set when cell 32i + j differs from its left neighbour
GOL_DIGEST_HD uint32_t rle_transitions(uint32_t c, uint32_t left) { return c ^ ((c << 1) | (left >> 31)); }

// What a lane holds of a row: words [w0, w0 + kRleSpanWords) of cells and transitions.
struct RleSpan {
    uint32_t c[kRleSpanWords], t[kRleSpanWords];
    int64_t p0;   // position of bit 0 of word 0
};
GOL_DIGEST_HD RleSpan rle_span_load(const uint32_t *packed, int64_t w0, int64_t ncols) {
    RleSpan s;
    s.p0 = 32 * w0;
    uint32_t left = rle_row_word(packed, w0 - 1, ncols);
    for (int k = 0; k < kRleSpanWords; ++k) {
        s.c[k] = rle_row_word(packed, w0 + k, ncols);
        s.t[k] = rle_transitions(s.c[k], left);
        left = s.c[k];
    }
    return s;
}
// the span's last transition position, -1 if it has none (what the max-scan carries)
GOL_DIGEST_HD int64_t rle_span_last(const RleSpan &s) {
    for (int k = kRleSpanWords - 1; k >= 0; --k)
        if (s.t[k]) return s.p0 + 32 * k + 31 - __builtin_clz(s.t[k]);
    return -1;
}
// fn(run length, tag) for every token the span's transitions end, in order; prev = the last
// transition before the span (0 if none).
template <typename F>
GOL_DIGEST_HD void rle_span_tokens(const RleSpan &s, int64_t prev, F &&fn) {
    for (int k = 0; k < kRleSpanWords; ++k) {
        uint32_t t = s.t[k];
        while (t) {
            const int b = __builtin_ctz(t);
            t &= t - 1;
            const int64_t p = s.p0 + 32 * k + b;
            if (p > 0) fn(p - prev, ((s.c[k] >> b) & 1u) ? 'b' : 'o');
            prev = p;
        }
    }
}
GOL_DIGEST_HD void rle_span_count(const RleSpan &s, int64_t prev, int64_t *ntok, int64_t *nraw) {
    int64_t n = 0, b = 0;
    rle_span_tokens(s, prev, [&](int64_t len, char) {
        ++n;
        b += rle_token_bytes(len);
    });
    *ntok = n;
    *nraw = b;
}
// Write pass, one span: its tokens, the first of them at dst and m = its global index mod L
// (newlines are a matter of the index mod L only).
GOL_DIGEST_HD void rle_span_write(const RleSpan &s, int64_t prev, int m, int L, char *dst) {
    rle_span_tokens(s, prev, [&](int64_t len, char tag) {
        const bool nl = m == L - 1;
        dst += rle_put_token(dst, len, tag, nl);
        m = nl ? 0 : m + 1;
    });
}

// spans of a row: its ncols / 32 + 1 words of positions in lanes of kRleSpanWords
GOL_DIGEST_HD int64_t rle_row_spans(int64_t ncols) { return (ncols / 32 + 1 + kRleSpanWords - 1) / kRleSpanWords; }

// Row scan, one row.  R = its window row, prev_row = the last non-empty row before it (-1: none),
// ntok / nraw = the row pass's counts.  The row's `$` count (0: no `$` token), its tokens and raw
// bytes with the `$` token.
struct RleRowHead {
    int64_t dcount, tokens, raw;
};
GOL_DIGEST_HD RleRowHead rle_row_head(int64_t R, int64_t prev_row, int64_t ntok, int64_t nraw) {
    RleRowHead h = {0, 0, 0};
    if (ntok == 0) return h;
    h.dcount = prev_row < 0 ? R : R - prev_row;
    h.tokens = ntok + (h.dcount > 0);
    h.raw = nraw + (h.dcount > 0 ? rle_token_bytes(h.dcount) : 0);
    return h;
}

// What the row scan leaves for the host: the block's bytes (newlines included), the token index
// and the last non-empty row behind the block.
struct RleRecord {
    int64_t bytes, tokens, last_row;
};

// ---- the three passes on host memory (lane after lane; the kernels scan instead) ----
inline void rle_row_pass_host(const uint32_t *packed, int64_t pitch_words, int64_t nrows, int64_t ncols, uint32_t *ntok,
                              uint32_t *nraw) {
    for (int64_t r = 0; r < nrows; ++r) {
        int64_t prev = 0, n = 0, b = 0;
        for (int64_t g = 0; g < rle_row_spans(ncols); ++g) {
            const RleSpan s = rle_span_load(packed + r * pitch_words, g * kRleSpanWords, ncols);
            int64_t dn, db;
            rle_span_count(s, prev, &dn, &db);
            n += dn;
            b += db;
            const int64_t last = rle_span_last(s);
            if (last > prev) prev = last;
        }
        ntok[r] = (uint32_t)n;
        nraw[r] = (uint32_t)b;
    }
}
inline void rle_row_scan_host(const uint32_t *ntok, const uint32_t *nraw, int64_t nrows, int64_t row_base,
                              int64_t last_row, int64_t tok0, int L, uint32_t *dcount, int64_t *tix, int64_t *off,
                              RleRecord *rec) {
    int64_t tok = tok0, raw = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        const RleRowHead h = rle_row_head(row_base + r, last_row, ntok[r], nraw[r]);
        dcount[r] = (uint32_t)h.dcount;
        tix[r] = tok;
        off[r] = raw + rle_newlines(tok0, tok - tok0, L);
        tok += h.tokens;
        raw += h.raw;
        if (ntok[r]) last_row = row_base + r;
    }
    rec->bytes = raw + rle_newlines(tok0, tok - tok0, L);
    rec->tokens = tok;
    rec->last_row = last_row;
}
inline void rle_write_pass_host(const uint32_t *packed, int64_t pitch_words, int64_t nrows, int64_t ncols,
                                const uint32_t *ntok, const uint32_t *dcount, const int64_t *tix, const int64_t *off,
                                int L, char *text) {
    for (int64_t r = 0; r < nrows; ++r) {
        if (!ntok[r]) continue;
        char *base = text + off[r];
        const uint32_t m0 = (uint32_t)(tix[r] % L);   // the row's first token index mod L
        uint32_t j = 0;                               // tokens of the row so far, its `$` included
        int64_t raw = 0;
        if (dcount[r]) {
            raw = rle_put_token(base, dcount[r], '$', m0 == (uint32_t)L - 1) - (m0 == (uint32_t)L - 1);
            ++j;
        }
        int64_t prev = 0;
        for (int64_t q = 0; q < rle_row_spans(ncols); ++q) {
            const RleSpan s = rle_span_load(packed + r * pitch_words, q * kRleSpanWords, ncols);
            int64_t dn, db;
            rle_span_count(s, prev, &dn, &db);
            if (dn) rle_span_write(s, prev, (int)((m0 + j) % (uint32_t)L), L, base + raw + (m0 + j) / (uint32_t)L);
            j += (uint32_t)dn;
            raw += db;
            const int64_t last = rle_span_last(s);
            if (last > prev) prev = last;
        }
    }
}

// ------------------------------------------------------------------ the parser (host only)
// The header line.  Leading lines that start with '#' are skipped; then
// `x = <n> , y = <n> [, rule = <text>]` with free spacing, up to '\n' or the end of the text.
// Returns 0 and the fields (rule_at / rule_len: the rule text, trimmed; rule_len = 0 if none; body:
// the offset behind the line), -1 with *body = the offending offset, or 1 when the text ends inside
// the header line and `final` is not set (a stream: feed more).
inline int rle_header_scan(const char *t, int64_t len, bool final, int64_t *x, int64_t *y, int64_t *rule_at,
                           int64_t *rule_len, int64_t *body) {
    int64_t i = 0;
    for (;;) {   // '#' lines
        if (i >= len) {
            *body = i;
            return final ? -1 : 1;
        }
        if (t[i] != '#') break;
        const void *nl = memchr(t + i, '\n', (size_t)(len - i));
        if (!nl) {
            *body = len;
            return final ? -1 : 1;
        }
        i = static_cast<const char *>(nl) - t + 1;
    }
    const void *nl = memchr(t + i, '\n', (size_t)(len - i));
    if (!nl && !final) return 1;
    const int64_t end = nl ? static_cast<const char *>(nl) - t : len;
    auto blank = [&](int64_t j) { return t[j] == ' ' || t[j] == '\t' || t[j] == '\r'; };
    auto skip = [&]() {
        while (i < end && blank(i)) ++i;
    };
    auto lit = [&](char ch) {
        skip();
        if (i < end && (t[i] == ch || (ch >= 'a' && ch <= 'z' && t[i] == ch - 32))) return ++i, true;
        return false;
    };
    auto number = [&](int64_t *v) {
        skip();
        if (i >= end || t[i] < '0' || t[i] > '9') return false;
        int64_t n = 0;
        for (; i < end && t[i] >= '0' && t[i] <= '9'; ++i) {
            n = n * 10 + (t[i] - '0');
            if (n > kRleMaxCount) return false;
        }
        *v = n;
        return true;
    };
    *rule_at = *rule_len = 0;
    bool ok = lit('x') && lit('=') && number(x) && lit(',') && lit('y') && lit('=') && number(y);
    if (ok) {
        skip();
        if (i < end) {
            ok = lit(',') && lit('r') && lit('u') && lit('l') && lit('e') && lit('=');
            if (ok) {
                skip();
                int64_t e = end;
                while (e > i && blank(e - 1)) --e;
                *rule_at = i;
                *rule_len = e - i;
                if (e == i) ok = false;
                i = end;
            }
        }
    }
    if (!ok) {
        *body = i;
        return -1;
    }
    *body = nl ? end + 1 : end;
    return 0;
}

// The body: a streaming state machine fed buffers of any size (a token may straddle two), filling
// packed MSB-first rows of the x × y box one row BLOCK at a time: the caller hands a cleared block
// [row0, row0 + nrows) of `pitch` bytes per row, feeds until the parser asks for the next block,
// ends or fails, and hands the next.  Live runs are the only thing stored, so a block nothing was
// stored in (live() == false) is all dead.
class RleParser {
public:
    enum Status { kMore, kBlock, kDone, kError };
    RleParser(int64_t x, int64_t y, int64_t offset0) : x_(x), y_(y), pos_(offset0) {}
    void set_block(uint8_t *rows, int64_t pitch, int64_t row0, int64_t nrows) {
        buf_ = rows, pitch_ = pitch, b0_ = row0, b1_ = row0 + nrows, live_ = false;
    }
    bool live() const { return live_; }
    bool done() const { return done_; }
    int64_t error_offset() const { return err_; }
    const char *reason() const { return why_; }
    // the input ended: fine only behind `!`
    Status finish() { return done_ ? kDone : error(pos_, "the text ends before '!'"); }
    // Consumes bytes of [p, p + n): *used of them.  kMore: all consumed, feed the next buffer;
    // kBlock: the next token stores cells behind the block (hand the block that holds row());
    // kDone: `!` was read; kError: error_offset() / reason().
    Status feed(const char *p, int64_t n, int64_t *used) {
        int64_t i = 0;
        Status st = kMore;
        for (; i < n && st == kMore; ++i) {
            const char ch = p[i];
            if (ch >= '0' && ch <= '9') {
                count_ = (have_ ? count_ * 10 : 0) + (ch - '0');
                have_ = true;
                if (count_ > kRleMaxCount) st = error(pos_ + i, "a count above 2^31");
            } else if (ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n') {
                if (have_) st = error(pos_ + i, "white space between a count and its tag");
            } else if (ch == 'b' || ch == 'o' || ch == '$' || ch == '!') {
                if (have_ && (count_ == 0 || ch == '!')) {
                    st = error(pos_ + i, ch == '!' ? "a count before '!'" : "a count of 0");
                    break;
                }
                const int64_t k = have_ ? count_ : 1;
                if (ch == '!') {
                    done_ = true;
                    st = kDone;
                } else if (ch == '$') {
                    if (row_ + k > y_) {
                        st = error(pos_ + i, "a row outside the box");
                        break;
                    }
                    row_ += k, col_ = 0;
                } else {
                    if (row_ >= y_ || col_ + k > x_) {
                        st = error(pos_ + i, row_ >= y_ ? "a run in a row outside the box" : "a run leaves the box");
                        break;
                    }
                    if (ch == 'o') {
                        if (row_ >= b1_) {   // (the count stays; the tag is read again)
                            pos_ += i;
                            *used = i;
                            return kBlock;
                        }
                        set_run(buf_ + (row_ - b0_) * pitch_, col_, k);
                        live_ = true;
                    }
                    col_ += k;
                }
                have_ = false;
            } else {
                st = error(pos_ + i, "a byte that is no count, tag or white space");
            }
        }
        if (st == kError) {
            *used = i;
            return st;
        }
        pos_ += i;
        *used = i;
        return st;
    }
    int64_t row() const { return row_; }

private:
    Status error(int64_t at, const char *why) {
        if (err_ < 0) err_ = at, why_ = why;
        return kError;
    }
    static void set_run(uint8_t *row, int64_t c, int64_t k) {   // columns [c, c + k), MSB first
        int64_t e = c + k;
        while (c < e && (c & 7)) row[c >> 3] |= (uint8_t)(0x80u >> (c & 7)), ++c;
        if (e - c >= 8) {
            memset(row + (c >> 3), 0xff, (size_t)((e - c) >> 3));
            c += (e - c) & ~(int64_t)7;
        }
        while (c < e) row[c >> 3] |= (uint8_t)(0x80u >> (c & 7)), ++c;
    }
    int64_t x_, y_, pos_;
    int64_t row_ = 0, col_ = 0, count_ = 0;
    bool have_ = false, done_ = false, live_ = false;
    uint8_t *buf_ = nullptr;
    int64_t pitch_ = 0, b0_ = 0, b1_ = 0;
    int64_t err_ = -1;
    const char *why_ = "";
};

}  // namespace gol
