// rule_k1.hip -- the 1-generation life-like rule stencil launcher (gol_rule), one TU per launch depth.
#include "golhip_rule.hpp"

namespace golhip {
GOLHIP_DEFINE_RULE_K(1)
}  // namespace golhip
