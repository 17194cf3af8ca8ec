// batch_period_daynight.hip -- gol_batch_period constant-folded for Day & Night (B3678/S34678): every board shape, plain and with history.
#include "batch_period.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_PERIOD_CONST(0x1C8, 0x1D8)
}  // namespace golhip
