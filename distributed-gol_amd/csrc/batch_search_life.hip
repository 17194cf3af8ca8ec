// batch_search_life.hip -- gol_batch_search for B3/S23 (LifeNext, gol_batch's rule step): every board
// shape.
#include "batch_search.hpp"

namespace golhip {

hipError_t launch_batch_search_life(int W, int R, int nsoups, const BatchSearchParams &sp, hipStream_t s) {
    return launch_batch_search_as<LifeNext>(W, R, nsoups, sp, s);
}

}  // namespace golhip
