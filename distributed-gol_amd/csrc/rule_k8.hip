// rule_k8.hip -- the 8-generation life-like rule stencil launcher (gol_rule), one TU per launch depth.
#include "golhip_rule.hpp"

namespace golhip {
GOLHIP_DEFINE_RULE_K(8)
}  // namespace golhip
