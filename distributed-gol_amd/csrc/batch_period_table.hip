// batch_period_table.hip -- gol_batch_period in the table form (RuleTable: any rule, uniform or one
// per board) for every board shape, plain and with history, and launch_batch_period: the dispatch of
// a period-tracking launch to its functor's translation unit (batch_period_*.hip).
#include "batch_period.hpp"

namespace golhip {

hipError_t launch_batch_period(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s) {
    const BatchParams &p = pp.b;
    if (K < 1 || K > kBoardMaxK || nboards < 1 || p.board_pitch != (int64_t)4 * W * R * p.wd ||
        (p.wd != 4 && p.wd != 8 && p.wd != 16) || p.prev || p.last_diff || !pp.snap || !pp.repeat_turn)
        return hipErrorInvalidValue;
    if (pp.rules)  // per-board rules: always the table form
        return launch_batch_period_as<RuleTable>(K, W, R, nboards, pp, s);
    if ((pp.rule.birth | pp.rule.survive) & ~kRuleMaskBits) return hipErrorInvalidValue;
    if (pp.rule.birth == kLifeBirth && pp.rule.survive == kLifeSurvive)
        return launch_batch_period_life(K, W, R, nboards, pp, s);
#define GOLHIP_X(B, S) \
    if (pp.rule.birth == (B) && pp.rule.survive == (S)) return launch_batch_period_##B##_##S(K, W, R, nboards, pp, s);
    GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
    return launch_batch_period_as<RuleTable>(K, W, R, nboards, pp, s);
}

}  // namespace golhip
