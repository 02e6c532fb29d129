// Host-only stand-in for the packed-bit launchers (test infrastructure, the
// companion of fake_hip.cpp, fake_hip_digest.cpp and fake_hip_density.cpp: see
// their headers).  It computes: the stand-in's "device" memory is host memory, so
// the row routines of gol_bits.h run here directly and the CPU suite checks the
// runtime's side of gol_download_bits* / gol_upload_bits* — slabs and seams,
// windows, column runs that share packed bytes, the torus margin, pitches, pad
// bits, pending windows — on byte-layout boards, whose byte uploads and downloads
// are plain copies (tests/test_bits_cpu.py), beside the recorded schedule
// (tests/sched_bits_check.py).  fake_hip_bits_fail_at(n) makes the n-th launch
// from now fail (0: none), so the suite can see what a call that fails half-way
// leaves behind.
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_bits.h"
#include "../../mpi_amd/csrc/gol_internal.h"

namespace {
int fail_at = 0;
}
extern "C" void fake_hip_bits_fail_at(int n) { fail_at = n; }

namespace gol {
namespace {
bool args_ok(int64_t r0, int64_t pc0, int64_t lc0, int64_t ncols, const void *packed, int64_t pitch_words, int bit_gw) {
    return r0 >= 0 && pc0 >= 0 && lc0 >= 0 && packed && (bit_gw == 0 || bit_gw == 2 || bit_gw == 4) &&
           bits_last_word(lc0, ncols) < pitch_words;
}
}  // namespace

hipError_t launch_get_bits(const void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t pc0, int64_t lc0,
                           int64_t ncols, uint32_t *out, int64_t out_pitch_words, int bit_gw, hipStream_t) {
    if (fail_at > 0 && --fail_at == 0) return hipErrorLaunchFailure;
    if (r1 <= r0 || ncols <= 0) return hipSuccess;
    if (!args_ok(r0, pc0, lc0, ncols, out, out_pitch_words, bit_gw)) return hipErrorInvalidValue;
    const uint8_t *b = static_cast<const uint8_t *>(buf);
    for (int64_t r = r0; r < r1; ++r) {
        const uint8_t *row = b + r * pitch_bytes;
        uint32_t *o = out + (r - r0) * out_pitch_words;
        if (bit_gw == 4) bits_get_row<4>(row, pc0, lc0, ncols, o);
        else if (bit_gw == 2) bits_get_row<2>(row, pc0, lc0, ncols, o);
        else bits_get_row<0>(row, pc0, lc0, ncols, o);
    }
    return hipSuccess;
}

hipError_t launch_put_bits(void *buf, int64_t pitch_bytes, int64_t r0, int64_t r1, int64_t pc0, int64_t lc0,
                           int64_t ncols, int64_t active_cols, const uint32_t *in, int64_t in_pitch_words, int bit_gw,
                           hipStream_t) {
    if (fail_at > 0 && --fail_at == 0) return hipErrorLaunchFailure;
    if (r1 <= r0 || ncols <= 0) return hipSuccess;
    if (!args_ok(r0, pc0, lc0, ncols, in, in_pitch_words, bit_gw)) return hipErrorInvalidValue;
    uint8_t *b = static_cast<uint8_t *>(buf);
    for (int64_t r = r0; r < r1; ++r) {
        uint8_t *row = b + r * pitch_bytes;
        const uint32_t *i = in + (r - r0) * in_pitch_words;
        if (bit_gw == 4) bits_put_row<4>(row, pc0, lc0, ncols, active_cols, i);
        else if (bit_gw == 2) bits_put_row<2>(row, pc0, lc0, ncols, active_cols, i);
        else bits_put_row<0>(row, pc0, lc0, ncols, active_cols, i);
    }
    return hipSuccess;
}
}  // namespace gol
