// Host-only stand-in for the density launcher (test infrastructure, the companion
// of fake_hip.cpp and fake_hip_digest.cpp: see their headers).  It computes: the
// stand-in's "device" memory is host memory, so the row routine of gol_density.h
// runs here directly and the CPU suite checks the runtime's side of gol_density*
// — per-slab parts and their sum, tiles across slab seams, column runs, the torus
// margin, windows, pending maps — on byte-layout boards, whose uploads and
// downloads are plain copies (tests/test_density_cpu.py), beside the recorded
// schedule (tests/sched_density_check.py).  fake_hip_density_fail_at(n) makes the
// n-th launch from now fail (0: none), so the suite can see what a call that fails
// half-way leaves behind.
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_density.h"
#include "../../mpi_amd/csrc/gol_internal.h"

namespace {
int fail_at = 0;
}
extern "C" void fake_hip_density_fail_at(int n) { fail_at = n; }

namespace gol {
namespace {
template <int G>
void density_rows(const uint8_t *buf, int64_t pitch, int64_t r0, int64_t r1, int64_t trow_off, int64_t pc0, int64_t lc0,
                  int64_t ncols, int64_t col0, int64_t tile_rows, int64_t tile_cols, uint32_t *part, int64_t ti_base,
                  int64_t tcols) {
    for (int64_t r = r0; r < r1; ++r)
        density_row<G>(buf + r * pitch, pc0, lc0, ncols, col0, tile_cols,
                       part + ((trow_off + (r - r0)) / tile_rows - ti_base) * tcols, tcols);
}
}  // namespace

hipError_t launch_density(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t trow_off, int64_t pc0,
                          int64_t lc0, int64_t ncols, int64_t col0, int64_t tile_rows, int64_t tile_cols,
                          uint32_t *part, int64_t ti_base, int64_t ntr, int64_t tcols, int bit_gw, hipStream_t) {
    if (fail_at > 0 && --fail_at == 0) return hipErrorLaunchFailure;
    if (r1 <= r0 || ncols <= 0) return hipSuccess;
    if (trow_off / tile_rows < ti_base || (trow_off + (r1 - r0) - 1) / tile_rows - ti_base >= ntr || lc0 < col0 ||
        (lc0 + ncols - 1 - col0) / tile_cols >= tcols)
        return hipErrorInvalidValue;
    const uint8_t *b = static_cast<const uint8_t *>(buf);
    if (bit_gw == 4)
        density_rows<4>(b, pitch_bytes, r0, r1, trow_off, pc0, lc0, ncols, col0, tile_rows, tile_cols, part, ti_base, tcols);
    else if (bit_gw == 2)
        density_rows<2>(b, pitch_bytes, r0, r1, trow_off, pc0, lc0, ncols, col0, tile_rows, tile_cols, part, ti_base, tcols);
    else
        density_rows<0>(b, pitch_bytes, r0, r1, trow_off, pc0, lc0, ncols, col0, tile_rows, tile_cols, part, ti_base, tcols);
    return hipSuccess;
}
}  // namespace gol
