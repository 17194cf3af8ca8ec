// batch_period_replicator.hip -- gol_batch_period constant-folded for Replicator (B1357/S1357): every board shape, plain and with history.
#include "batch_period.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_PERIOD_CONST(0x0AA, 0x0AA)
}  // namespace golhip
