// batch_rule_seeds.hip -- gol_batch_rule constant-folded for Seeds (B2/S): every board shape and mode.
#include "batch_rule.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_RULE_CONST(0x004, 0x000)
}  // namespace golhip
