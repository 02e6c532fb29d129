// Host-only stand-in for the board-to-board copy's launcher (test infrastructure,
// the companion of fake_hip.cpp, fake_hip_bits.cpp and fake_hip_fill.cpp: see their
// headers).  It computes: the stand-in's "device" memory is host memory, so the row
// routine of gol_copy.h runs here directly and the CPU suite checks the runtime's
// side of gol_copy_window — the pairing of slabs and of column runs, seams, the
// torus margin, MESH_COMPAT's blocks, the inactive cells, the argument rules, rank
// contexts (tests/copy_cpu_check.py) — beside the recorded schedule
// (tests/sched_copy_check.py).
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_copy.h"
#include "../../mpi_amd/csrc/gol_internal.h"

namespace gol {

namespace {
template <int GS>
void copy_row_to(int dst_gw, const void *s, int64_t spc0, void *d, int64_t dpc0, int64_t n, int64_t active, int op) {
    if (dst_gw == 4) copy_row<GS, 4>(s, spc0, d, dpc0, n, active, op);
    else if (dst_gw == 2) copy_row<GS, 2>(s, spc0, d, dpc0, n, active, op);
    else copy_row<GS, 0>(s, spc0, d, dpc0, n, active, op);
}
}  // namespace

hipError_t launch_copy_cells(const void *src, int64_t src_pitch_bytes, int64_t sr0, int64_t spc0, int src_gw, void *dst,
                             int64_t dst_pitch_bytes, int64_t dr0, int64_t dpc0, int dst_gw, int64_t nrows,
                             int64_t ncols, int64_t active_cols, int op, hipStream_t) {
    if (nrows <= 0 || ncols <= 0) return hipSuccess;
    const auto gw_ok = [](int g) { return g == 0 || g == 2 || g == 4; };
    if (!src || !dst || sr0 < 0 || dr0 < 0 || spc0 < 0 || dpc0 < 0 || !gw_ok(src_gw) || !gw_ok(dst_gw) ||
        op < kCopyReplace || op > kCopyXor)
        return hipErrorInvalidValue;
    const uint8_t *sb = static_cast<const uint8_t *>(src);
    uint8_t *db = static_cast<uint8_t *>(dst);
    for (int64_t r = 0; r < nrows; ++r) {
        const void *s = sb + (sr0 + r) * src_pitch_bytes;
        void *d = db + (dr0 + r) * dst_pitch_bytes;
        if (src_gw == 4) copy_row_to<4>(dst_gw, s, spc0, d, dpc0, ncols, active_cols, op);
        else if (src_gw == 2) copy_row_to<2>(dst_gw, s, spc0, d, dpc0, ncols, active_cols, op);
        else copy_row_to<0>(dst_gw, s, spc0, d, dpc0, ncols, active_cols, op);
    }
    return hipSuccess;
}
}  // namespace gol
