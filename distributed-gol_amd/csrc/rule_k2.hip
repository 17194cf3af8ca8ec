// rule_k2.hip -- the 2-generation life-like rule stencil launcher (gol_rule), one TU per launch depth.
#include "golhip_rule.hpp"

namespace golhip {
GOLHIP_DEFINE_RULE_K(2)
}  // namespace golhip
