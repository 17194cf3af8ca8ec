// batch_search_table.hip -- gol_batch_search in the table form (RuleTable: any rule, uniform or one
// per soup) for every board shape, and launch_batch_search: the dispatch of a search launch to its
// functor's translation unit (batch_search_*.hip).
#include "batch_search.hpp"

namespace golhip {

hipError_t launch_batch_search(int W, int R, int nsoups, const BatchSearchParams &sp, hipStream_t s) {
    if (sp.max_turns < 1 || sp.max_turns > kSearchMaxTurns || nsoups < 1 || !sp.out ||
        (sp.wd != 4 && sp.wd != 8 && sp.wd != 16) || sp.width < 64 || sp.width % 64 != 0 || sp.width > 32 * sp.wd)
        return hipErrorInvalidValue;
    if (sp.rules)  // per-soup rules: always the table form
        return launch_batch_search_as<RuleTable>(W, R, nsoups, sp, s);
    if ((sp.rule.birth | sp.rule.survive) & ~kRuleMaskBits) return hipErrorInvalidValue;
    if (sp.rule.birth == kLifeBirth && sp.rule.survive == kLifeSurvive)
        return launch_batch_search_life(W, R, nsoups, sp, s);
#define GOLHIP_X(B, S) \
    if (sp.rule.birth == (B) && sp.rule.survive == (S)) return launch_batch_search_##B##_##S(W, R, nsoups, sp, s);
    GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
    return launch_batch_search_as<RuleTable>(W, R, nsoups, sp, s);
}

}  // namespace golhip
