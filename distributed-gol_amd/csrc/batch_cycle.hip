// batch_cycle.hip -- gol_batch_cycle (batch_cycle.hpp), the exact pass of golhip_batch_search_exact, in
// its two forms: B3/S23's rule step (LifeNext), what a uniform B3/S23 runs on either topology, boxed
// or not; and the table form (RuleTable), every other uniform rule, the catalogue rules included,
// and per-soup rules.  One translation unit for the two: every kernel TU carries the helper kernels
// of stencil_tile.hpp, and the production library has a size to keep (tests/test_boundary.py).
#include "batch_cycle.hpp"

namespace golhip {

hipError_t launch_batch_cycle_life(int W, int R, int nsoups, const BatchCycleParams &cp, hipStream_t s) {
    return launch_batch_cycle_as<LifeNext>(W, R, nsoups, cp, s);
}

hipError_t launch_batch_cycle_table(int W, int R, int nsoups, const BatchCycleParams &cp, hipStream_t s) {
    return launch_batch_cycle_as<RuleTable>(W, R, nsoups, cp, s);
}

}  // namespace golhip
