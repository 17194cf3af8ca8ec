// batch_plane_table.hip -- the plane kernels in the table form (RuleTable: any rule, uniform or one per
// board or soup): gol_plane_rule for every board shape and mode, gol_plane_period plain and with
// history, gol_plane_search; and launch_plane_rule, launch_plane_period and launch_plane_search: the
// dispatch of a plane launch (or a boxed search launch) to its functor.
#include "batch_plane.hpp"

namespace golhip {

hipError_t launch_plane_rule(int K, int W, int R, int nboards, const BatchRuleParams &rp, hipStream_t s) {
    const BatchParams &p = rp.b;
    if (K < 1 || K > kBoardMaxK || nboards < 1 || p.board_pitch != (int64_t)4 * W * R * p.wd ||
        (p.wd != 4 && p.wd != 8 && p.wd != 16) || (p.prev && !p.last_diff) || p.width < 1 ||
        p.width > 32 * p.wd || (p.width & (p.width - 1)) != 0)
        return hipErrorInvalidValue;
    if (!rp.rules && ((rp.rule.birth | rp.rule.survive) & ~kRuleMaskBits)) return hipErrorInvalidValue;
    if (plane_is_life(rp.rule, rp.rules)) return launch_plane_rule_life(K, W, R, nboards, rp, s);
    return launch_plane_rule_as<RuleTable>(K, W, R, nboards, rp, s);
}

hipError_t launch_plane_period(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s) {
    const BatchParams &p = pp.b;
    if (K < 1 || K > kBoardMaxK || nboards < 1 || p.board_pitch != (int64_t)4 * W * R * p.wd ||
        (p.wd != 4 && p.wd != 8 && p.wd != 16) || p.prev || p.last_diff || !pp.snap || !pp.repeat_turn ||
        p.width < 1 || p.width > 32 * p.wd || (p.width & (p.width - 1)) != 0)
        return hipErrorInvalidValue;
    if (!pp.rules && ((pp.rule.birth | pp.rule.survive) & ~kRuleMaskBits)) return hipErrorInvalidValue;
    if (plane_is_life(pp.rule, pp.rules)) return launch_plane_period_life(K, W, R, nboards, pp, s);
    return launch_plane_period_as<RuleTable>(K, W, R, nboards, pp, s);
}

hipError_t launch_plane_search(int W, int R, int nsoups, const BatchBoxSearchParams &bp, hipStream_t s) {
    const BatchSearchParams &sp = bp.s;
    const SoupBox &bx = bp.box;
    if (sp.max_turns < 1 || sp.max_turns > kSearchMaxTurns || nsoups < 1 || !sp.out ||
        (sp.wd != 4 && sp.wd != 8 && sp.wd != 16) || sp.width < 64 || sp.width % 64 != 0 || sp.width > 32 * sp.wd ||
        (sp.width & (sp.width - 1)) != 0)
        return hipErrorInvalidValue;
    if (bx.w < 1 || bx.h < 1 || bx.x0 < 0 || bx.y0 < 0 || bx.x0 + bx.w > sp.width || bx.y0 + bx.h > 4 * W * R)
        return hipErrorInvalidValue;
    if (!sp.rules && ((sp.rule.birth | sp.rule.survive) & ~kRuleMaskBits)) return hipErrorInvalidValue;
    if (plane_is_life(sp.rule, sp.rules)) return launch_plane_search_life(W, R, nsoups, bp, s);
    return launch_plane_search_as<RuleTable>(W, R, nsoups, bp, s);
}

}  // namespace golhip
