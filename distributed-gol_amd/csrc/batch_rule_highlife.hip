// batch_rule_highlife.hip -- gol_batch_rule constant-folded for HighLife (B36/S23): every board shape and mode.
#include "batch_rule.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_RULE_CONST(0x048, 0x00C)
}  // namespace golhip
