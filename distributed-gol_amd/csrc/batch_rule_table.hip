// batch_rule_table.hip -- gol_batch_rule in the table form (RuleTable: any rule, uniform or one
// per board) for every board shape and mode, and launch_batch_rule: the dispatch of a batch rule
// launch to its functor's translation unit (batch_rule_*.hip).
#include "batch_rule.hpp"

namespace golhip {

hipError_t launch_batch_rule(int K, int W, int R, int nboards, const BatchRuleParams &rp, hipStream_t s) {
    const BatchParams &p = rp.b;
    if (K < 1 || K > kBoardMaxK || nboards < 1 || p.board_pitch != (int64_t)4 * W * R * p.wd ||
        (p.wd != 4 && p.wd != 8 && p.wd != 16) || (p.prev && !p.last_diff))
        return hipErrorInvalidValue;
    if (rp.rules)  // per-board rules: always the table form
        return launch_batch_rule_as<RuleTable>(K, W, R, nboards, rp, s);
    if ((rp.rule.birth | rp.rule.survive) & ~kRuleMaskBits) return hipErrorInvalidValue;
#define GOLHIP_X(B, S) \
    if (rp.rule.birth == (B) && rp.rule.survive == (S)) return launch_batch_rule_##B##_##S(K, W, R, nboards, rp, s);
    GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
    return launch_batch_rule_as<RuleTable>(K, W, R, nboards, rp, s);
}

}  // namespace golhip
