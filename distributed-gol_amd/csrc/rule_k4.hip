// rule_k4.hip -- the 4-generation life-like rule stencil launcher (gol_rule), one TU per launch depth.
#include "golhip_rule.hpp"

namespace golhip {
GOLHIP_DEFINE_RULE_K(4)
}  // namespace golhip
