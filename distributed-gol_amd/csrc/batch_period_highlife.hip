// batch_period_highlife.hip -- gol_batch_period constant-folded for HighLife (B36/S23): every board shape, plain and with history.
#include "batch_period.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_PERIOD_CONST(0x048, 0x00C)
}  // namespace golhip
