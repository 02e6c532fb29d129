// gol — reference-compatible driver for the MI355X engine.
//
//   gol [options] rows cols iteration_gap iterations [time_file] [first]
//
// Keeps the positional CLI of main.cpp:171-220 / main_serial.cpp:115-130, the
// `<timestamp>.gol` main file (main.cpp:131-147), the per-part snapshot files
// `<name>_<iter>_<part>.gol` (main.cpp:106-129) that gol_visualization.py
// stitches, and the `_detailed.out` / `_compact.csv` timing report
// (main.cpp:310-365; values in µs under the reference's "ms" labels).  All
// compute goes through the C ABI of include/golhip.h.
//
// Options
//   --mode mpi|serial|dead|torus
//                           mpi (default): main.cpp semantics on a √P×√P mesh of
//                           --procs P emulated ranks (P=1: dead boundary);
//                           serial: main_serial.cpp semantics (writes gen 0 and
//                           every gap, like the serial program);
//                           dead: textbook non-periodic B3/S23, any rows×cols;
//                           torus: periodic B3/S23 (GOL_TORUS), the cells of dead's
//                           generation 0; rows / gpus and cols at least K.
//   --procs P               emulated MPI ranks for --mode mpi (default 1)
//   --gpus N                row slabs / GPUs (default 1)
//   --layout bit|byte       cell layout (default: bit; byte when --procs P has
//                           blocks of cols/√P not a multiple of 32 columns)
//   -k K                    generations fused per launch (default 1)
//   --rule B36/S23          a life-like rule in B/S notation (gol_parse_rule: also
//                           S23/B36 and the legacy 23/3) instead of B3/S23; with
//                           --mode dead|torus, --layout bit and -k 1..7 (the mpi and
//                           serial modes reproduce the reference, which knows one
//                           rule).  Snapshots and timing files as without it
//   --rule-kernel auto|generic   auto (default): a rule with a kernel compiled for it
//                           (gol_compiled_rule) runs that kernel; generic: every --rule
//                           runs the rule-generic kernel (GOL_OPT_RULE_COMPILED 0).
//                           The boards are the same
//   --save / --no-save      write snapshots every gap generations
//                           (default: on for serial, off for mpi/dead as in main.cpp:208)
//   --seed S                override the srand seed
//   --soup P                start from a random soup of density P (0 <= P <= 1) in place
//                           of the mode's glibc init: gol_fill_random with the threshold
//                           of P (gol_fill_threshold) and seed --seed (default 1), written
//                           on the device.  Every mode and layout; with --gpus N / --rccl
//                           every slab fills its own rows (a cell depends on the seed, P
//                           and its global coordinates only)
//   --resume NAME --from I  continue the run of NAME.gol from its saved
//                           iteration I (part files NAME_I_<p>.gol, read back
//                           on the device); rows/cols/gap/iters default to the
//                           main file's; new snapshots continue under NAME
//   --format gol|pbm|rle    the snapshot parts' format (default gol: the reference's text).
//                           pbm: part files `<name>_<iter>_<part>.pbm`, binary PBM —
//                           "P4\n# gol <firstRow> <lastRow> <firstCol> <lastCol>\n<ncols> <nrows>\n"
//                           (the comment carries the four numbers of the .gol header
//                           lines), then the raster: rows of ceil(ncols / 8) bytes, MSB
//                           first, 1 = live, packed on the device
//                           (gol_download_bits_window) — a sixteenth of the text's
//                           bytes, and any image tool opens it.  With --resume the
//                           parts NAME_I_<p>.pbm are read back (gol_upload_bits_window).
//                           rle: part files `<name>_<iter>_<part>.rle`, each the RLE pattern
//                           (gol_write_rle, encoded on the device) of the rows it holds,
//                           behind a `#CXRLE Pos=<col>,<row>` line with the part's origin,
//                           which RLE readers take for a comment; with --resume the parts
//                           NAME_I_<p>.rle are read back (gol_read_rle) at that origin
//   --pattern FILE[@row,col]  load the RLE pattern FILE onto the starting board (after the
//                           mode's init or --soup; --soup 0 gives an empty board), its
//                           top-left cell at (row, col), default (0, 0); its x × y box is
//                           replaced.  Repeatable, loaded in order.  Without --rule, the
//                           rule the first pattern's header names is set (gol_rle_header).
//                           Under --rccl a pattern's rows must lie within one rank's slab
//   --rccl                  the N row slabs as N RCCL ranks of ONE process: one
//                           rank context (gol_create_rank) and one communicator
//                           per device, each driven by a host thread, halo rows
//                           through ncclSend/ncclRecv (the transport of the
//                           one-process-per-GPU path; the default --gpus N path
//                           keeps the slabs in one context with peer copies).
//                           Rank r runs on device r; RCCL refuses two ranks on
//                           one device, so on one GPU this needs --same-device
//                           with an in-process RCCL stand-in (--rccl-lib)
//   --rccl-lib PATH         bind this RCCL library instead of the system's
//                           (loaded into the global scope before any rank;
//                           tests: tests/shim/libfake_rccl.so)
//   --same-device           --rccl: every rank on device 0
//   --digest                print "digest <generation> <32 hex digits>" (gol_digest,
//                           lane 0 then lane 1) for the starting board, at every
//                           multiple of the gap (a snapshot point, saving or not) and
//                           at the end; with --gpus N / --rccl the slabs' parts
//                           summed.  Without it stdout is unchanged
//   --density T[xU]         write the board's density map (gol_density: live cells per
//                           tile of T rows × U columns; U a multiple of 32, default T)
//                           as `<name>_<iter>.pgm` at every multiple of the gap (a
//                           snapshot point, saving or not) and at the end, and print
//                           "density <generation> <file>".  Binary PGM:
//                           "P5\n<tcols> <trows>\n65535\n", then 16-bit big-endian
//                           samples floor(65535 · count / cells), cells = the clipped
//                           tile's own cell count (edge tiles are not darker).  The map
//                           is enqueued (gol_density_async) ahead of the point's
//                           synchronising call: the run is not drained for it; with
//                           --gpus N / --rccl the contexts' maps are added
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/golhip.h"

namespace {

void die(const char *msg) {
    printf("%s\n", msg);
    exit(1);
}

void check(gol_ctx *c, int rc, const char *what) {
    if (rc != GOL_OK) {
        fprintf(stderr, "%s failed (%d): %s\n", what, rc, c ? gol_last_error(c) : "");
        exit(1);
    }
}

// main.cpp:131-147 / main_serial.cpp:97-113
std::string set_up_program(long rows, long cols, int gap, int iters, int parts) {
    char buf[50];
    time_t raw;
    time(&raw);
    strftime(buf, sizeof buf, "%Y-%m-%d-%H-%M-%S", localtime(&raw));
    std::string name(buf);
    FILE *f = fopen((name + ".gol").c_str(), "w");
    if (!f) die("cannot create main .gol file");
    fprintf(f, "%ld %ld %d %d %d\n", rows, cols, gap, iters, parts);
    fclose(f);
    return name;
}

// main.cpp:106-129: two header lines, then rows of "v\t" tokens.  The body is
// formatted on the device and streamed to the file (gol_write_text).
void write_part(gol_ctx *ctx, const std::string &name, int iter, int part, long first_row, long last_row,
                long first_col, long last_col, int64_t row0, int64_t nrows, int64_t ncols) {
    std::string path = name + "_" + std::to_string(iter) + "_" + std::to_string(part) + ".gol";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die("cannot create part .gol file");
    fprintf(f, "%ld %ld\n%ld %ld\n", first_row, last_row, first_col, last_col);
    fflush(f);
    check(ctx, gol_write_text(ctx, row0, 0, nrows, ncols, fileno(f)), "gol_write_text");
    fclose(f);
}

// Snapshot resume: load part file `path` (either header convention: the origin
// is the first number of each header line, the shape comes from the body).
void read_part(gol_ctx *ctx, const std::string &path) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) die(("cannot open " + path).c_str());
    long r0 = 0, r_end = 0, c0 = 0, c_end = 0;
    if (fscanf(f, "%ld %ld\n%ld %ld", &r0, &r_end, &c0, &c_end) != 4 || fgetc(f) != '\n')
        die(("bad header in " + path).c_str());
    const long off = ftell(f);
    long rowlen = 0;
    for (int ch; (ch = fgetc(f)) != EOF;) {
        ++rowlen;
        if (ch == '\n') break;
    }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fclose(f);
    if (rowlen < 3 || rowlen % 2 == 0 || (size - off) % rowlen != 0) die(("bad body in " + path).c_str());
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0 || lseek(fd, off, SEEK_SET) != off) die(("cannot open " + path).c_str());
    check(ctx, gol_read_text(ctx, r0, c0, (size - off) / rowlen, (rowlen - 1) / 2, fd), path.c_str());
    close(fd);
}

// --format pbm: the part as a binary PBM, the raster downloaded packed in row blocks of
// at most 64 MiB.  The comment line carries write_part's four header numbers.
constexpr int64_t kPbmBlock = 64LL << 20;
void write_part_pbm(gol_ctx *ctx, const std::string &name, int iter, int part, long first_row, long last_row,
                    long first_col, long last_col, int64_t row0, int64_t nrows, int64_t ncols) {
    std::string path = name + "_" + std::to_string(iter) + "_" + std::to_string(part) + ".pbm";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) die("cannot create part .pbm file");
    fprintf(f, "P4\n# gol %ld %ld %ld %ld\n%lld %lld\n", first_row, last_row, first_col, last_col, (long long)ncols,
            (long long)nrows);
    const int64_t rb = gol_bits_row_bytes(ncols), br = std::max<int64_t>(1, kPbmBlock / std::max<int64_t>(1, rb));
    std::vector<uint8_t> buf((size_t)(std::min(br, nrows) * rb));
    for (int64_t a = 0; a < nrows; a += br) {
        const int64_t n = std::min(br, nrows - a);
        check(ctx, gol_download_bits_window(ctx, row0 + a, 0, n, ncols, buf.data(), rb), "gol_download_bits_window");
        if (fwrite(buf.data(), 1, (size_t)(n * rb), f) != (size_t)(n * rb)) die(("cannot write " + path).c_str());
    }
    if (fclose(f) != 0) die(("cannot write " + path).c_str());
}

// Snapshot resume from a .pbm part: the origin is the first and third number of the
// comment, the shape the size line's; the raster must be complete.
void read_part_pbm(gol_ctx *ctx, const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die(("cannot open " + path).c_str());
    long r0 = 0, r_end = 0, c0 = 0, c_end = 0;
    long long ncols = 0, nrows = 0;
    char magic[3] = {0, 0, 0};
    if (fread(magic, 1, 3, f) != 3 || memcmp(magic, "P4\n", 3) != 0 ||
        fscanf(f, "# gol %ld %ld %ld %ld", &r0, &r_end, &c0, &c_end) != 4 || fgetc(f) != '\n' ||
        fscanf(f, "%lld %lld", &ncols, &nrows) != 2 || fgetc(f) != '\n' || r0 < 0 || c0 < 0 || ncols < 1 || nrows < 1)
        die(("bad header in " + path).c_str());
    const long off = ftell(f);
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    const int64_t rb = gol_bits_row_bytes(ncols);
    if (size - off != nrows * rb) die(("bad body in " + path + ": the raster is short or long").c_str());
    fseek(f, off, SEEK_SET);
    const int64_t br = std::max<int64_t>(1, kPbmBlock / rb);
    std::vector<uint8_t> buf((size_t)(std::min<int64_t>(br, nrows) * rb));
    for (int64_t a = 0; a < nrows; a += br) {
        const int64_t n = std::min<int64_t>(br, nrows - a);
        if (fread(buf.data(), 1, (size_t)(n * rb), f) != (size_t)(n * rb)) die(("cannot read " + path).c_str());
        check(ctx, gol_upload_bits_window(ctx, r0 + a, c0, n, ncols, buf.data(), rb), path.c_str());
    }
    fclose(f);
}

// --format rle: the part as an RLE pattern of its own rows, encoded on the device; the leading
// `#CXRLE Pos=<col>,<row>` line (a comment to RLE readers) carries the part's origin.
void write_part_rle(gol_ctx *ctx, const std::string &name, int iter, int part, long first_row, long, long first_col,
                    long, int64_t row0, int64_t nrows, int64_t ncols) {
    std::string path = name + "_" + std::to_string(iter) + "_" + std::to_string(part) + ".rle";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) die("cannot create part .rle file");
    fprintf(f, "#CXRLE Pos=%ld,%ld\n", first_col, first_row);
    fflush(f);
    check(ctx, gol_write_rle(ctx, row0, 0, nrows, ncols, fileno(f)), "gol_write_rle");
    if (fclose(f) != 0) die(("cannot write " + path).c_str());
}

// Snapshot resume from an .rle part: the origin is the `#CXRLE Pos=` line's, the box the header's.
void read_part_rle(gol_ctx *ctx, const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die(("cannot open " + path).c_str());
    long c0 = 0, r0 = 0;
    if (fscanf(f, "#CXRLE Pos=%ld,%ld", &c0, &r0) != 2 || fgetc(f) != '\n' || r0 < 0 || c0 < 0)
        die(("bad header in " + path).c_str());
    fclose(f);
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) die(("cannot open " + path).c_str());
    check(ctx, gol_read_rle(ctx, r0, c0, fd, nullptr, nullptr), path.c_str());
    close(fd);
}

// --pattern FILE[@row,col]: the file's bytes, where it goes, what its header says
struct Pattern {
    std::string path, text;
    int64_t row = 0, col = 0, x = 0, y = 0;
    uint32_t birth = 0, survive = 0;
    int has_rule = 0;
};
Pattern load_pattern(const std::string &arg) {
    Pattern p;
    p.path = arg;
    const size_t at = arg.rfind('@');
    if (at != std::string::npos) {
        long long r = 0, c = 0;
        int used = 0;
        if (sscanf(arg.c_str() + at + 1, "%lld,%lld%n", &r, &c, &used) != 2 || arg[at + 1 + used] || r < 0 || c < 0)
            die("--pattern must be FILE or FILE@row,col");
        p.path = arg.substr(0, at);
        p.row = r;
        p.col = c;
    }
    FILE *f = fopen(p.path.c_str(), "rb");
    if (!f) die(("--pattern: cannot open " + p.path).c_str());
    char buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) p.text.append(buf, n);
    fclose(f);
    if (gol_rle_header(p.text.data(), (int64_t)p.text.size(), &p.x, &p.y, &p.birth, &p.survive, &p.has_rule, nullptr) !=
        GOL_OK)
        die(("--pattern: no RLE header in " + p.path).c_str());
    return p;
}

struct Opts {
    std::string mode = "mpi", layout = "", format = "gol";
    int procs = 1, gpus = 1, k = 1, save = -1;
    long long seed = -1;
    std::string soup;     // --soup P: the starting density (empty: the mode's glibc init)
    std::string resume;   // --resume NAME: continue the run whose main file is NAME.gol
    int from = -1;        // --from ITER: the saved iteration to continue from
    bool rccl = false, same_device = false;
    std::string rccl_lib;
    std::string rule;     // --rule: B/S notation (empty: B3/S23 on the tuned kernels)
    std::string rule_kernel = "auto";   // --rule-kernel: auto | generic
    bool digest = false;  // --digest: print the board's digest at every snapshot point and at the end
    int64_t tile_rows = 0, tile_cols = 0;   // --density T[xU] (0: no map)
    std::vector<std::string> patterns;      // --pattern FILE[@row,col], in order
};

// One rank of --rccl: its context and what it reports.
struct RankRun {
    gol_ctx *ctx = nullptr;
    double dev_ms = 0.0;
    int64_t live = 0, launches = 0;
    std::vector<std::array<uint64_t, 3>> digests;   // --digest: (generation, lane 0, lane 1) of this context's rows
    // --density: (generation, this context's map) per point; a map is filled by the next synchronising call
    std::vector<std::pair<int, std::vector<uint32_t>>> maps;
    std::string err;
};

// --density: binary PGM of a map, 16-bit big-endian samples floor(65535 · count / cells of the clipped tile)
void write_pgm(const std::string &path, const std::vector<uint32_t> &map, int64_t trows, int64_t tcols, long rows,
               long cols, int64_t tile_rows, int64_t tile_cols) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) die(("cannot create " + path).c_str());
    fprintf(f, "P5\n%lld %lld\n65535\n", (long long)tcols, (long long)trows);
    std::vector<uint8_t> line(2 * (size_t)tcols);
    for (int64_t i = 0; i < trows; ++i) {
        const uint64_t h = (uint64_t)std::min<int64_t>(tile_rows, rows - i * tile_rows);
        for (int64_t j = 0; j < tcols; ++j) {
            const uint64_t cells = h * (uint64_t)std::min<int64_t>(tile_cols, cols - j * tile_cols);
            const uint64_t v = 65535ull * map[(size_t)(i * tcols + j)] / cells;
            line[2 * j] = (uint8_t)(v >> 8);
            line[2 * j + 1] = (uint8_t)v;
        }
        if (fwrite(line.data(), 1, line.size(), f) != line.size()) die(("cannot write " + path).c_str());
    }
    fclose(f);
}

// Runs fn(r) for r = 0..n-1 on n host threads at once (the rank calls are
// collective: every rank must be inside gol_create_rank / gol_step together).
template <typename F>
void on_ranks(int n, F fn) {
    std::vector<std::thread> ts;
    for (int r = 0; r < n; ++r) ts.emplace_back([&, r] { fn(r); });
    for (auto &t : ts) t.join();
}

} // namespace

int main(int argc, char **argv) {
    auto t_begin = std::chrono::steady_clock::now();
    Opts o;
    std::vector<const char *> pos;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char * {
            if (i + 1 >= argc) die("missing option value");
            return argv[++i];
        };
        if (a == "--mode") o.mode = next();
        else if (a == "--procs") o.procs = atoi(next());
        else if (a == "--gpus") o.gpus = atoi(next());
        else if (a == "--layout") o.layout = next();
        else if (a == "-k") o.k = atoi(next());
        else if (a == "--rule") o.rule = next();
        else if (a == "--rule-kernel") o.rule_kernel = next();
        else if (a == "--format") o.format = next();
        else if (a == "--save") o.save = 1;
        else if (a == "--no-save") o.save = 0;
        else if (a == "--seed") o.seed = atoll(next());
        else if (a == "--soup") o.soup = next();
        else if (a == "--resume") o.resume = next();
        else if (a == "--from") o.from = atoi(next());
        else if (a == "--rccl") o.rccl = true;
        else if (a == "--rccl-lib") o.rccl_lib = next();
        else if (a == "--same-device") o.same_device = true;
        else if (a == "--digest") o.digest = true;
        else if (a == "--pattern") o.patterns.push_back(next());
        else if (a == "--density") {
            const char *v = next();
            char *end = nullptr;
            o.tile_rows = strtoll(v, &end, 10);
            o.tile_cols = o.tile_rows;
            if (end != v && *end == 'x') {
                const char *u = end + 1;
                o.tile_cols = strtoll(u, &end, 10);
                if (end == u) o.tile_rows = 0;
            }
            if (end == v || *end || o.tile_rows < 1 || o.tile_cols < 32 || o.tile_cols % 32 ||
                o.tile_rows > 0xffffffffll / o.tile_cols)
                die("--density must be T or TxU: tile rows, then tile columns (a multiple of 32, default T), "
                    "at most 2^32 - 1 cells per tile");
        }
        else pos.push_back(argv[i]);
    }
    if (o.format != "gol" && o.format != "pbm" && o.format != "rle") die("--format must be gol, pbm or rle");
    const bool pbm = o.format == "pbm", rle = o.format == "rle";
    std::vector<Pattern> patterns;
    for (const std::string &a : o.patterns) patterns.push_back(load_pattern(a));
    uint64_t soup_threshold = 0;
    if (!o.soup.empty()) {
        char *end = nullptr;
        const double p = strtod(o.soup.c_str(), &end);
        if (end == o.soup.c_str() || *end || gol_fill_threshold(p, &soup_threshold) != GOL_OK)
            die("--soup must be a density between 0 and 1");
    }
    long m_rows = 0, m_cols = 0;
    int m_gap = 0, m_iters = 0, m_parts = 0;
    if (!o.resume.empty()) {
        FILE *mf = fopen((o.resume + ".gol").c_str(), "r");
        if (!mf || fscanf(mf, "%ld %ld %d %d %d", &m_rows, &m_cols, &m_gap, &m_iters, &m_parts) != 5)
            die("--resume: cannot read the main .gol file");
        fclose(mf);
        if (o.from < 0) die("--resume needs --from ITER");
        if (pos.empty()) {
            static std::string a0, a1, a2, a3;
            a0 = std::to_string(m_rows), a1 = std::to_string(m_cols), a2 = std::to_string(m_gap),
            a3 = std::to_string(m_iters);
            pos = {a0.c_str(), a1.c_str(), a2.c_str(), a3.c_str()};
        }
    }
    if (pos.size() < 4 || pos.size() > 6)
        die("This program should be called with four arguments! \nThese should be, the total number of rows; "
            "the total number of columns; the gap between saved iterations and the total number of "
            "iterations, in that order.");
    const long rows = atol(pos[0]), cols = atol(pos[1]);
    const int gap = atoi(pos[2]), iters = atoi(pos[3]);
    std::string time_file;
    int first = pos.size() > 5 ? atoi(pos[5]) : 0;

    int boundary = GOL_DEAD, init = GOL_INIT_STREAM, m = 1;
    uint32_t seed = 1;
    int layout = o.layout == "byte" ? GOL_LAYOUT_BYTE : GOL_LAYOUT_BIT;
    bool save = false;
    if (o.mode == "mpi") {
        // main.cpp:194-199
        const float z = std::sqrt((float)o.procs);
        if (rows <= 0 || rows != cols || z != std::floor(z) || rows % (int)z != 0 || rows / (int)z < 4)
            die("Illegal board size parameter combination!");
        m = (int)z;
        seed = 0;   // block (cx,cy) <- srand(cx·m + cy); srand(0) ≡ srand(1)
        if (m > 1) {
            boundary = GOL_MESH_COMPAT;
            init = GOL_INIT_MESH;
            // the bit layout's device init needs 32-column-aligned mesh blocks
            if (o.layout.empty() && o.soup.empty() && (cols / m) % 32 != 0) layout = GOL_LAYOUT_BYTE;
        }
        save = o.save == 1;   // main.cpp:208 hard-codes save_file = 0
    } else if (o.mode == "serial") {
        if (rows != cols) die("serial mode needs rows == cols");
        boundary = GOL_SERIAL_COMPAT;
        init = GOL_INIT_SERIAL;
        seed = GOL_SERIAL_SEED;   // main_serial.cpp:150
        save = o.save != 0;
    } else if (o.mode == "dead") {
        save = o.save == 1;
    } else if (o.mode == "torus") {
        boundary = GOL_TORUS;
        save = o.save == 1;
    } else {
        die("--mode must be mpi, serial, dead or torus");
    }
    uint32_t birth = 0, survive = 0;
    if (o.rule_kernel != "auto" && o.rule_kernel != "generic") die("--rule-kernel must be auto or generic");
    if (!o.rule.empty()) {
        if (gol_parse_rule(o.rule.c_str(), &birth, &survive) != GOL_OK)
            die("--rule must be in B/S notation, such as B36/S23, S23/B36 or 23/3");
        if (o.mode != "dead" && o.mode != "torus")
            die("--rule needs --mode dead or torus (the mpi and serial modes reproduce the reference program, "
                "which knows B3/S23 only)");
        if (layout != GOL_LAYOUT_BIT) die("--rule needs --layout bit (the byte layout computes B3/S23 only)");
    }
    // --pattern without --rule: the rule the first pattern's header names
    bool pattern_rule = false;
    if (o.rule.empty() && !patterns.empty() && patterns[0].has_rule) {
        birth = patterns[0].birth;
        survive = patterns[0].survive;
        pattern_rule = true;
    }
    if (o.seed >= 0) seed = (uint32_t)o.seed;
    if (gap <= 0 && save) die("iteration_gap must be positive when saving");

    const int parts = o.gpus;
    const int from = o.resume.empty() ? 0 : o.from;
    if (from > iters) die("--from is past the last iteration");
    if (!o.resume.empty() && (m_rows != rows || m_cols != cols)) die("--resume: board size differs from the main file");
    // a resumed run keeps the original name so gol_visualization.py sees one sequence of iterations
    std::string name = o.resume.empty() ? set_up_program(rows, cols, gap, iters, parts) : o.resume;
    if (!o.resume.empty() && parts != m_parts) {
        // the part count of the new snapshots must match the main file
        FILE *mf = fopen((name + ".gol").c_str(), "w");
        if (!mf) die("cannot rewrite the main .gol file");
        fprintf(mf, "%ld %ld %d %d %d\n", rows, cols, gap, std::max(iters, m_iters), parts);
        fclose(mf);
    }
    time_file = pos.size() > 4 ? std::string(pos[4]) : name;

    std::vector<int64_t> row0(parts), nrow(parts);
    for (int p = 0; p < parts; ++p) gol_slab_plan(rows, parts, p, &row0[p], &nrow[p]);
    // --rccl: one rank context per slab; otherwise ONE context holding every slab
    const int nctx = o.rccl ? parts : 1;
    std::vector<RankRun> rk(nctx);
    if (o.rccl) {
        if (!o.rccl_lib.empty() && !dlopen(o.rccl_lib.c_str(), RTLD_NOW | RTLD_GLOBAL))
            die(("--rccl-lib: cannot load " + o.rccl_lib).c_str());
        if (!o.resume.empty() && m_parts != parts) die("--rccl --resume needs the saved run's part count");
    }
    uint8_t uid[GOL_UNIQUE_ID_BYTES];
    if (o.rccl) check(nullptr, gol_get_unique_id(uid), "gol_get_unique_id");
    // part p of a snapshot: the rows of slab p, written by the context holding them
    auto write_snap = [&](gol_ctx *ctx, int iter, int p) {
        const auto part = rle ? write_part_rle : pbm ? write_part_pbm : write_part;
        if (o.mode == "serial" && parts == 1)   // main_serial.cpp:164-167: "0 n" / "0 n"
            part(ctx, name, iter, p, 0, rows, 0, cols, 0, rows, cols);
        else   // main.cpp:255-258: inclusive ranges (gol_visualization.py:33 slices [min, max+1])
            part(ctx, name, iter, p, row0[p], row0[p] + nrow[p] - 1, 0, cols - 1, row0[p], nrow[p], cols);
    };
    // set-up of context i (rank i under --rccl): create, then the board
    auto set_up = [&](int i) {
        gol_ctx *ctx = nullptr;
        if (o.rccl)
            check(nullptr, gol_create_rank(&ctx, rows, cols, i, parts, o.same_device ? 0 : i, uid, layout, boundary,
                                           m, o.k), "gol_create_rank");
        else
            check(nullptr, gol_create(&ctx, rows, cols, o.gpus, layout, boundary, m, o.k), "gol_create");
        rk[i].ctx = ctx;
        if (!o.rule.empty() || pattern_rule)
            check(ctx, gol_set_rule(ctx, birth, survive), "gol_set_rule");   // (-k >= 8: its message)
        if (o.rule_kernel == "generic") check(ctx, gol_set_option(ctx, GOL_OPT_RULE_COMPILED, 0), "GOL_OPT_RULE_COMPILED");
        // launches are counted on the host (gol_kernel_time without GOL_OPT_KERNEL_TIMING): no event pair
        // per launch inside the timed region
        if (o.resume.empty() && !o.soup.empty()) {
            check(ctx, gol_fill_random(ctx, o.seed >= 0 ? (uint64_t)o.seed : 1, soup_threshold), "gol_fill_random");
        } else if (o.resume.empty()) {
            check(ctx, gol_init_glibc(ctx, init, seed), "gol_init_glibc");
        } else {
            for (int p = 0; p < m_parts; ++p)
                if (!o.rccl || p == i)
                    (rle ? read_part_rle : pbm ? read_part_pbm : read_part)(
                        ctx, o.resume + "_" + std::to_string(from) + "_" + std::to_string(p) +
                                 (rle ? ".rle" : pbm ? ".pbm" : ".gol"));
        }
        // --pattern: onto the starting board, in order (a rank loads the patterns whose rows it holds)
        for (size_t j = 0; o.resume.empty() && j < patterns.size(); ++j) {
            const Pattern &pt = patterns[j];
            if (o.rccl) {
                const bool above = pt.row + pt.y <= row0[i], below = pt.row >= row0[i] + nrow[i];
                if (above || below) continue;
                if (pt.row < row0[i] || pt.row + pt.y > row0[i] + nrow[i])
                    die(("--pattern: the rows of " + pt.path + " straddle two ranks' slabs").c_str());
            }
            check(ctx, gol_parse_rle(ctx, pt.row, pt.col, pt.text.data(), (int64_t)pt.text.size(), nullptr, nullptr),
                  pt.path.c_str());
        }
        // main_serial.cpp:171 writes generation 0; main.cpp:285 has that write commented out, which
        // leaves gol_visualization.py without its iteration-0 files, so every saving mode writes it.
        if (save && o.resume.empty())
            for (int p = 0; p < parts; ++p)
                if (!o.rccl || p == i) write_snap(ctx, 0, p);
        check(ctx, gol_sync(ctx, nullptr), "gol_sync");
    };
    // the generation loop of context i (main.cpp:291-305): every rank steps the same generations
    auto run = [&](int i) {
        gol_ctx *ctx = rk[i].ctx;
        double dev_ms = 0.0;
        // --digest: this context's part of the board's digest (gol_digest; the parts add)
        auto take_digest = [&](int gen) {
            uint64_t d[2] = {0, 0};
            check(ctx, gol_digest(ctx, d), "gol_digest");
            rk[i].digests.push_back({(uint64_t)gen, d[0], d[1]});
        };
        if (o.digest) take_digest(from);
        // --density: this context's map (gol_density_async: enqueued here, filled by the next
        // synchronising call; the contexts' maps add)
        const bool density = o.tile_rows > 0;
        auto take_density = [&](int gen) {
            int64_t tr = 0, tc = 0;
            check(ctx, gol_density_dims(rows, cols, o.tile_rows, o.tile_cols, &tr, &tc), "gol_density_dims");
            rk[i].maps.emplace_back(gen, std::vector<uint32_t>((size_t)(tr * tc)));
            check(ctx, gol_density_async(ctx, o.tile_rows, o.tile_cols, rk[i].maps.back().second.data(), tc),
                  "gol_density_async");
        };
        if (save || ((o.digest || density) && gap > 0)) {
            // step straight to the next snapshot (k-generation blocks inside gol_step)
            for (int a = from; a < iters;) {
                const int next = std::min(iters, (a / gap + 1) * gap);
                check(ctx, gol_step(ctx, next - a), "gol_step");
                a = next;
                if (a % gap == 0) {
                    if (density) take_density(a);
                    double ms = 0;
                    check(ctx, gol_sync(ctx, &ms), "gol_sync");
                    dev_ms += ms;
                    for (int p = 0; save && p < parts; ++p)
                        if (!o.rccl || p == i) write_snap(ctx, a, p);
                    if (o.digest) take_digest(a);
                }
            }
        } else {
            check(ctx, gol_step(ctx, iters - from), "gol_step");
        }
        if (density && (rk[i].maps.empty() || rk[i].maps.back().first != iters)) take_density(iters);
        double ms = 0;
        check(ctx, gol_sync(ctx, &ms), "gol_sync");
        rk[i].dev_ms = dev_ms + ms;
        if (o.digest && rk[i].digests.back()[0] != (uint64_t)iters) take_digest(iters);
        double kernel_ms = 0;
        check(ctx, gol_popcount(ctx, &rk[i].live), "gol_popcount");
        check(ctx, gol_kernel_time(ctx, &kernel_ms, &rk[i].launches, 0), "gol_kernel_time");
    };
    if (o.rccl) on_ranks(nctx, set_up);
    else set_up(0);
    auto t_check1 = std::chrono::steady_clock::now();
    if (o.rccl) on_ranks(nctx, run);
    else run(0);
    // the ranks' reduction (main.cpp:319-324): the slowest rank's device time, every rank's cells
    double dev_ms = 0.0;
    int64_t live = 0, launches = 0;
    for (auto &r : rk) {
        dev_ms = std::max(dev_ms, r.dev_ms);
        live += r.live;
        launches += r.launches;
    }
    auto t_end = std::chrono::steady_clock::now();
    if (o.rccl) on_ranks(nctx, [&](int i) { gol_destroy(rk[i].ctx); });
    else gol_destroy(rk[0].ctx);

    // main.cpp:312-364 (µs values, "ms" labels; sums over the emulated parts)
    const long local = (long)std::chrono::duration_cast<std::chrono::microseconds>(t_end - t_begin).count();
    const long nosetup = (long)std::chrono::duration_cast<std::chrono::microseconds>(t_end - t_check1).count();
    const long setup = (long)std::chrono::duration_cast<std::chrono::microseconds>(t_check1 - t_begin).count();
    // main.cpp:341-362 reports the MPI processors; here the emulated ranks of --mode mpi (--procs),
    // which the GPU slabs stand in for.  The GPU count goes to _gcups.csv.
    const int P = o.mode == "mpi" ? o.procs : parts;
    FILE *f = fopen((time_file + "_detailed.out").c_str(), "a");
    if (f) {
        fprintf(f, "Timing results: milliseconds \nsize:%ld by %ld\n%d Processors\n", cols, rows, P);
        fprintf(f, "Full (with setup) \nSingle time (rank 0): %ldms\nAvg single time: %ldms\nSummed time: %ldms\n",
                local, local, local * P);
        fprintf(f, "Without setup \nSingle time (rank 0): %ldms\nAvg single time: %ldms\nSummed time: %ldms\n",
                nosetup, nosetup, nosetup * P);
        fprintf(f, "Setup \nSingle time (rank 0): %ldms\nAvg single time: %ldms\nSummed time: %ldms\n", setup,
                setup, setup * P);
        fprintf(f, "___________________________________________________ \n\n");
        fclose(f);
    }
    f = fopen((time_file + "_compact.csv").c_str(), "a");
    if (f) {
        if (first != 0)
            fprintf(f, "X,Y,#P,full single,full avg,full sum,nosetup single,nosetup avg,nosetup sum,"
                       "setup single ,setup avg ,setup sum \n");
        fprintf(f, "%ld,%ld,%d,%ld,%ld,%ld,%ld,%ld,%ld,%ld,%ld,%ld\n", cols, rows, P, local, local, local * P,
                nosetup, nosetup, nosetup * P, setup, setup, setup * P);
        fclose(f);
    }
    // additions, in a separate file so the reference's formats stay untouched
    const double gcups = (double)rows * cols * (iters - from) / (dev_ms * 1e-3) / 1e9;
    f = fopen((time_file + "_gcups.csv").c_str(), "a");
    if (f) {
        fprintf(f, "%ld,%ld,%d,%d,%s,%d,%.3f,%.3f,%lld,%lld\n", rows, cols, iters, parts,
                layout == GOL_LAYOUT_BIT ? "bit" : "byte", o.k, dev_ms, gcups, (long long)live, (long long)launches);
        fclose(f);
    }
    // --digest: one line per point, the contexts' parts summed (mod 2^64), lane 0 then lane 1
    for (size_t j = 0; o.digest && j < rk[0].digests.size(); ++j) {
        uint64_t d[2] = {0, 0};
        for (auto &r : rk) {
            d[0] += r.digests[j][1];
            d[1] += r.digests[j][2];
        }
        printf("digest %llu %016llx%016llx\n", (unsigned long long)rk[0].digests[j][0], (unsigned long long)d[0],
               (unsigned long long)d[1]);
    }
    // --density: one PGM per point, the contexts' maps added
    for (size_t j = 0; j < rk[0].maps.size(); ++j) {
        std::vector<uint32_t> map = rk[0].maps[j].second;
        for (size_t r = 1; r < rk.size(); ++r)
            for (size_t t = 0; t < map.size(); ++t) map[t] += rk[r].maps[j].second[t];
        int64_t tr = 0, tc = 0;
        gol_density_dims(rows, cols, o.tile_rows, o.tile_cols, &tr, &tc);
        const std::string path = name + "_" + std::to_string(rk[0].maps[j].first) + ".pgm";
        write_pgm(path, map, tr, tc, rows, cols, o.tile_rows, o.tile_cols);
        printf("density %d %s\n", rk[0].maps[j].first, path.c_str());
    }
    printf("0: %s  gens=%d  device %.3f ms  %.1f GCUPS  live=%lld  launches=%lld%s\n", name.c_str(), iters - from,
           dev_ms, gcups, (long long)live, (long long)launches, o.rccl ? "  (rccl ranks)" : "");
    printf("0: all succeeded\n");
    return 0;
}
