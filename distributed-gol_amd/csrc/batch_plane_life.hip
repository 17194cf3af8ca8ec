// batch_plane_life.hip -- the plane kernels with B3/S23's rule step (LifeNext), what a uniform B3/S23
// runs on a plane: gol_plane_rule for every board shape and mode, gol_plane_period plain and with
// history, gol_plane_search.  One translation unit for the three: every kernel TU carries the
// helper kernels of stencil_tile.hpp, and the production library has a size to keep.
#include "batch_plane.hpp"

namespace golhip {

hipError_t launch_plane_rule_life(int K, int W, int R, int nboards, const BatchRuleParams &rp, hipStream_t s) {
    return launch_plane_rule_as<LifeNext>(K, W, R, nboards, rp, s);
}

hipError_t launch_plane_period_life(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s) {
    return launch_plane_period_as<LifeNext>(K, W, R, nboards, pp, s);
}

hipError_t launch_plane_search_life(int W, int R, int nsoups, const BatchBoxSearchParams &bp, hipStream_t s) {
    return launch_plane_search_as<LifeNext>(W, R, nsoups, bp, s);
}

}  // namespace golhip
