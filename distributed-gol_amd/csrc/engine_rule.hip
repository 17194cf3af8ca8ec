// engine_rule.hip -- life-like rules: the B.../S... parser, the handle's rule, and the dispatch of
// a rule launch to its depth's translation unit (rule_k<K>.hip, gol_rule in golhip_rule.hpp).
//
// The reference hard-codes Conway's rule (calculateNextState, server/server.go:21-52: alive next iff
// 3 neighbours, or 2 and alive); here it is the default of a handle whose rule can be any
// outer-totalistic rule on the same 8-cell neighbourhood.  B3/S23 keeps the production kernels and
// their planner; any other rule runs gol_rule on every launch (engine: rule_path()).
#include <cctype>
#include <cstdio>

#include "golhip_engine.hpp"

namespace golhip {

hipError_t launch_rule(int K, RuleMasks rm, const uint32_t *in_row0, uint32_t *out_row0,
                       const StencilParams &p, unsigned long long *slots, hipStream_t s) {
    switch (K) {
#define GOLHIP_X(KK) \
    case KK: return launch_rule_k##KK(rm, in_row0, out_row0, p, slots, s);
        GOLHIP_RULE_DEPTHS(GOLHIP_X)
#undef GOLHIP_X
        default: return hipErrorInvalidValue;  // a missing kernel is an error, never another kernel
    }
}

int rule_waves_per_cu(int K, RuleMasks rm, bool counting) {
    const void *fn = nullptr;
    switch (K) {
#define GOLHIP_X(KK) \
    case KK: fn = rule_fn_k##KK(rm, counting); break;
        GOLHIP_RULE_DEPTHS(GOLHIP_X)
#undef GOLHIP_X
        default: break;
    }
    int blocks = 0;
    if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 256, 0) != hipSuccess || blocks < 1)
        return 4;
    return blocks * 4;  // 256-thread blocks = 4 waves
}

namespace {

// "B<digits>/S<digits>", case-insensitive, digits 0-8 without repeats, either list may be empty.
// On failure `why` says what is wrong with the text.
bool parse_rule_text(const char *rule, uint32_t *birth, uint32_t *survive, std::string *why) {
    auto bad = [&](const char *what) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "rule \"%.80s\": %s (expected B<digits 0-8>/S<digits 0-8>, e.g. B36/S23)",
                      rule ? rule : "(null)", what);
        *why = buf;
        return false;
    };
    if (!rule) return bad("no text");
    const char *c = rule;
    uint32_t m[2] = {0, 0};
    for (int part = 0; part < 2; ++part) {
        if (std::toupper((unsigned char)*c) != (part == 0 ? 'B' : 'S'))
            return bad(part == 0 ? "does not start with B" : "no S part after the '/'");
        ++c;
        for (; *c >= '0' && *c <= '9'; ++c) {
            const int d = *c - '0';
            if (d > 8) return bad("a cell has at most 8 neighbours");
            if (m[part] & (1u << d)) return bad("a digit is repeated");
            m[part] |= 1u << d;
        }
        if (part == 0) {
            if (*c != '/') return bad("no '/' after the B part");
            ++c;
        }
    }
    if (*c != '\0') return bad("text after the S part");
    *birth = m[0];
    *survive = m[1];
    return true;
}

}  // namespace
}  // namespace golhip

using namespace golhip;

extern "C" {

int golhip_parse_rule(const char *rule, uint32_t *birth, uint32_t *survive) {
    uint32_t b = 0, s = 0;
    std::string why;
    if (!birth || !survive) {
        g_create_error = "golhip_parse_rule: null output";
        return GOLHIP_ERR_ARG;
    }
    if (!parse_rule_text(rule, &b, &s, &why)) {
        g_create_error = why;  // golhip_last_error(NULL)
        return GOLHIP_ERR_ARG;
    }
    *birth = b;
    *survive = s;
    return GOLHIP_OK;
}

int golhip_set_rule_masks(golhip_t h, uint32_t birth, uint32_t survive) {
    if (!h) return GOLHIP_ERR_ARG;
    if ((birth | survive) & ~kRuleMaskBits)
        return fail(h, GOLHIP_ERR_ARG, "rule masks birth=0x%x survive=0x%x: bits above 8 (a cell has 8 neighbours)",
                    birth, survive);
    if (birth == h->rule.birth && survive == h->rule.survive) return GOLHIP_OK;
    // everything cached per launch shape goes: captured graphs bake a kernel in (graph_for's key has
    // no rule), the stable-slab flags describe launches of the old rule
    int rc = sync_all(h);
    if (rc) return rc;
    for (auto &g : h->graphs) (void)hipGraphExecDestroy(g.exec);
    h->graphs.clear();
    h->act_valid = false;
    for (auto &w : h->rule_wpc) w[0] = w[1] = 0;  // the occupancy cache is per rule kernel
    h->rule.birth = birth;
    h->rule.survive = survive;
    return GOLHIP_OK;
}

int golhip_set_rule(golhip_t h, const char *rule) {
    if (!h) return GOLHIP_ERR_ARG;
    uint32_t b = 0, s = 0;
    std::string why;
    if (!parse_rule_text(rule, &b, &s, &why)) return fail(h, GOLHIP_ERR_ARG, "%s", why.c_str());
    return golhip_set_rule_masks(h, b, s);
}

int golhip_get_rule(golhip_t h, uint32_t *birth, uint32_t *survive) {
    if (!h || !birth || !survive) return GOLHIP_ERR_ARG;
    *birth = h->rule.birth;
    *survive = h->rule.survive;
    return GOLHIP_OK;
}

}  // extern "C"
