// batch_rule_replicator.hip -- gol_batch_rule constant-folded for Replicator (B1357/S1357): every board shape and mode.
#include "batch_rule.hpp"

namespace golhip {
GOLHIP_DEFINE_BATCH_RULE_CONST(0x0AA, 0x0AA)
}  // namespace golhip
