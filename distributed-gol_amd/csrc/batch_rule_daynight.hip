// batch_rule_daynight.hip -- gol_batch_rule constant-folded for Day & Night (B3678/S34678): every board shape and mode.
#include "batch_rule.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_RULE_CONST(0x1C8, 0x1D8)
}  // namespace golhip
