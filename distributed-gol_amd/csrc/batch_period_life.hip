// batch_period_life.hip -- gol_batch_period for B3/S23 (LifeNext, gol_batch's rule step): every board
// shape, plain and with history.
#include "batch_period.hpp"

namespace golhip {

hipError_t launch_batch_period_life(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s) {
    return launch_batch_period_as<LifeNext>(K, W, R, nboards, pp, s);
}

}  // namespace golhip
