"""The RLE pattern text of gol_format_rle / gol_parse_rle in pure Python, on numpy
arrays, written straight from the format's definition ("RLE pattern
files"; include/golhip.h): the yardstick of the RLE tests.

encode(cells, birth, survive) -> bytes      the canonical text of a 2-D 0/1 array
decode(text) -> (cells, info)               what gol_parse_rle accepts; RleError(offset) otherwise
header(text) -> (x, y, rule or None, body)  the header line behind any '#' lines
"""
import re

import numpy as np

LIFE = (1 << 3, (1 << 2) | (1 << 3))
MAX_COUNT = 1 << 31


class RleError(ValueError):
    def __init__(self, offset, why):
        super().__init__(f"malformed RLE at byte {offset}: {why}")
        self.offset = offset


def rule_text(birth, survive):
    digits = lambda m: "".join(str(i) for i in range(9) if m >> i & 1)  # noqa: E731
    return f"B{digits(birth)}/S{digits(survive)}"


def line_tokens(nrows, ncols):
    return 70 // (1 + len(str(max(nrows, ncols, 1))))


def tokens(cells):
    """The token stream of a window, `!` included: (count, tag) pairs."""
    out, last = [], -1
    for r in range(cells.shape[0]):
        live = np.flatnonzero(cells[r])
        if live.size == 0:
            continue
        gap = r if last < 0 else r - last
        if gap > 0:
            out.append((gap, "$"))
        last = r
        row = cells[r, :live[-1] + 1].astype(np.int8)
        # maximal runs from column 0 up to the last live cell
        cuts = np.flatnonzero(np.diff(row)) + 1
        starts = np.concatenate(([0], cuts))
        ends = np.concatenate((cuts, [row.size]))
        for a, e in zip(starts.tolist(), ends.tolist()):
            out.append((e - a, "o" if row[a] else "b"))
    out.append((1, "!"))
    return out


def encode(cells, birth=LIFE[0], survive=LIFE[1]):
    cells = np.asarray(cells)
    nrows, ncols = (cells.shape if cells.ndim == 2 else (0, 0))
    L = line_tokens(nrows, ncols)
    parts = [f"x = {ncols}, y = {nrows}, rule = {rule_text(birth, survive)}\n"]
    toks = tokens(cells) if nrows and ncols else [(1, "!")]
    for i, (n, tag) in enumerate(toks):
        parts.append((str(n) if n >= 2 else "") + tag)
        if i % L == L - 1 or tag == "!":
            parts.append("\n")
    return "".join(parts).encode()


_RULE = re.compile(r"^(?:[Bb]([0-8]*)/[Ss]([0-8]*)|[Ss]([0-8]*)/[Bb]([0-8]*)|([0-8]*)/([0-8]*))$")


def parse_rule(text):
    m = _RULE.match(text)
    if not m:
        return None
    if m.group(1) is not None:
        b, s = m.group(1), m.group(2)
    elif m.group(3) is not None:
        s, b = m.group(3), m.group(4)
    else:
        s, b = m.group(5), m.group(6)
        if not s and not b:
            return None
    if len(set(b)) != len(b) or len(set(s)) != len(s):
        return None
    return sum(1 << int(d) for d in b), sum(1 << int(d) for d in s)


_HEAD = re.compile(rb"[ \t\r]*[xX][ \t\r]*=[ \t\r]*(\d+)[ \t\r]*,[ \t\r]*[yY][ \t\r]*=[ \t\r]*(\d+)[ \t\r]*"
                   rb"(?:,[ \t\r]*[rR][ \t\r]*[uU][ \t\r]*[lL][ \t\r]*[eE][ \t\r]*=[ \t\r]*([^\n]*?))?[ \t\r]*(?:\n|$)")


def header(text):
    """(x, y, (birth, survive) or None, body offset); RleError on a malformed header."""
    i = 0
    while text[i:i + 1] == b"#":
        j = text.find(b"\n", i)
        if j < 0:
            raise RleError(len(text), "no header line")
        i = j + 1
    m = _HEAD.match(text, i)
    if not m:
        raise RleError(i, "malformed header")
    rule = None
    if m.group(3) is not None:
        rule = parse_rule(m.group(3).decode("latin-1"))
        if rule is None:
            raise RleError(m.start(3), "rule text refused")
    return int(m.group(1)), int(m.group(2)), rule, m.end()


def decode(text):
    """The x × y cells of an RLE text and (x, y, rule); RleError(offset) on anything the format's
    reading rules refuse."""
    x, y, rule, i = header(text)
    cells = np.zeros((y, x), np.uint8)
    if x == 0 or y == 0:
        return cells, (x, y, rule)
    row = col = 0
    count = None
    while True:
        if i >= len(text):
            raise RleError(len(text), "the text ends before '!'")
        ch = chr(text[i])
        if ch.isdigit() and ch.isascii():
            count = (count or 0) * 10 + int(ch)
            if count > MAX_COUNT:
                raise RleError(i, "a count above 2^31")
        elif ch in " \t\r\n":
            if count is not None:
                raise RleError(i, "white space between a count and its tag")
        elif ch in "bo$!":
            if count is not None and (count == 0 or ch == "!"):
                raise RleError(i, "a count of 0, or a count before '!'")
            n = 1 if count is None else count
            count = None
            if ch == "!":
                return cells, (x, y, rule)
            if ch == "$":
                if row + n > y:
                    raise RleError(i, "a row outside the box")
                row, col = row + n, 0
            else:
                if row >= y or col + n > x:
                    raise RleError(i, "a run leaves the box")
                if ch == "o":
                    cells[row, col:col + n] = 1
                col += n
        else:
            raise RleError(i, "a byte that is no count, tag or white space")
        i += 1
