// Host-only stand-in for the compiled-rule launcher (test infrastructure, the
// companion of fake_hip.cpp: see its header).  Like every launch there it does
// nothing; which path a context picks for its rule (gol_rule_path) and the
// schedule of a context with a compiled rule set are what the CPU suite
// exercises (tests/test_rule_compiled_cpu.py).
#include <hip/hip_runtime.h>

#include "../../mpi_amd/csrc/gol_internal.h"

namespace gol {
bool bit_crule_supported(int gens, int gw, int rule_index) {
    return gw == 2 && gens >= 1 && gens <= 7 && rule_index >= 0 && rule_index < kCompiledRuleCount;
}
hipError_t launch_bit_crule(const StencilArgs &, int, int, hipStream_t) { return hipSuccess; }
}  // namespace gol
