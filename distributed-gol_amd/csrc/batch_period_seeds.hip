// batch_period_seeds.hip -- gol_batch_period constant-folded for Seeds (B2/S): every board shape, plain and with history.
#include "batch_period.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_PERIOD_CONST(0x004, 0x000)
}  // namespace golhip
