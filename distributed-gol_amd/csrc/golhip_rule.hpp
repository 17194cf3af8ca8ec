// golhip_rule.hpp -- gol_rule<K, COUNT, LD, Rule>: the rule-generic streaming stencil for life-like
// (outer-totalistic, Moore neighbourhood) rules B.../S..., shared by the per-depth translation
// units rule_k*.hip.  gol_stencil and the other B3/S23 kernels are untouched: B3/S23 never runs this.
//
// Same mapping and the same StencilParams contract as gol_stencil's drifting 62-word geometry
// (golhip_stencil.hpp): one lane = one 32-bit word, lanes 1..62 of a wave store whole words, K
// chained levels with drifting row sums (one DPP + 2 v_alignbit + 2 v_bitop3 per row), the level-K
// row realigned before its store, per-generation counts of owned cells into `slots`, the last
// generation's flips to p.diff.  Input rows come by plain global loads prefetched in VGPRs; every
// wait is the compiler's (no LDS-DMA ring, no hand-counted vmcnt).
//
// The rule.  With o, k the full adder of the three rows' sum bits and p, q that of their carries
// (as in life_next), the 9-cell sum including the centre is S9 = o + 2 T, T = k + p + 2 q in 0..4,
// so S9's bits are b0 = o, b1 = k ^ p, b2 = (k & p) ^ q, b3 = k & p & q (b1..b3 = the bits of T).
// The next state is G[S9][mc]: G[s][0] = birth bit s, G[s][1] = survive bit s - 1 (a live centre
// is part of S9); G[0][1] and G[9][0] cannot occur and are taken as 0.
//   RuleConst<B, S>: for each of the four (o, mc) pairs the next state is a function of (k, p, q)
//     alone, i.e. one v_bitop3 whose truth table is derived constexpr from the masks
//     (rule_tt<B, S>(o, mc)); three selects (mc, mc, o) pick among them: 7 v_bitop3 after o, k, p, q
//     (life_next: 3), fewer where the compiler folds equal or constant tables.
//   RuleTable: the 18 rule bits arrive as kernel arguments and are expanded to 0 / ~0 words once per
//     wave; a select tree evaluates them: mc (10 selects: g[s] = mc ? S[s-1] : B[s]), o (5:
//     e[T] = o ? g[2T+1] : g[2T]), then b1, b1, b2, b3 (4) with b1..b3 computed by 3 ops: 22
//     v_bitop3 after o, k, p, q.  The same kernel template with another functor.
#pragma once
#include "golhip_stencil.hpp"

namespace golhip {
namespace {

constexpr uint8_t kSelect = GOL_TT((a & b) | (~a & c));  // a ? b : c
static_assert(kSelect == 0xCA, "bitop3 select table");

// G[s][mc] of the rule (birth, survive), s = 9-cell sum including the centre.
constexpr uint32_t rule_next_bit(uint32_t birth, uint32_t survive, int s, int mc) {
    if (mc) return s >= 1 && s <= 9 ? (survive >> (s - 1)) & 1u : 0u;
    return s <= 8 ? (birth >> s) & 1u : 0u;
}
// Truth table over (k, p, q) -- index (k << 2) | (p << 1) | q, v_bitop3's order -- of the next
// state for fixed o and mc: S9 = o + 2 (k + p + 2 q).
template <uint32_t B, uint32_t S>
constexpr uint8_t rule_tt(int o, int mc) {
    uint32_t tt = 0;
    for (int i = 0; i < 8; ++i) {
        const int k = (i >> 2) & 1, p = (i >> 1) & 1, q = i & 1;
        tt |= rule_next_bit(B, S, o + 2 * (k + p + 2 * q), mc) << i;
    }
    return (uint8_t)tt;
}

template <uint32_t B, uint32_t S>
struct RuleConst {
    static constexpr bool kConst = true;
    __device__ __forceinline__ explicit RuleConst(RuleMasks) {}
    __device__ __forceinline__ uint32_t next(uint32_t o, uint32_t k, uint32_t p, uint32_t q,
                                             uint32_t mc) const {
        const uint32_t a00 = GOL_BOP3(k, p, q, (rule_tt<B, S>(0, 0)));
        const uint32_t a01 = GOL_BOP3(k, p, q, (rule_tt<B, S>(0, 1)));
        const uint32_t a10 = GOL_BOP3(k, p, q, (rule_tt<B, S>(1, 0)));
        const uint32_t a11 = GOL_BOP3(k, p, q, (rule_tt<B, S>(1, 1)));
        const uint32_t even = GOL_BOP3(mc, a01, a00, kSelect);
        const uint32_t odd = GOL_BOP3(mc, a11, a10, kSelect);
        return GOL_BOP3(o, odd, even, kSelect);
    }
};

struct RuleTable {
    static constexpr bool kConst = false;
    uint32_t b[10], s[10];  // b[n] / s[n]: 0 or ~0, G[n][0] / G[n][1] for S9 = n
    __device__ __forceinline__ explicit RuleTable(RuleMasks rm) {
#pragma unroll
        for (int n = 0; n < 10; ++n) {
            b[n] = (n <= 8 && ((rm.birth >> n) & 1u)) ? ~0u : 0u;
            s[n] = (n >= 1 && ((rm.survive >> (n - 1)) & 1u)) ? ~0u : 0u;
        }
    }
    __device__ __forceinline__ uint32_t next(uint32_t o, uint32_t k, uint32_t p, uint32_t q,
                                             uint32_t mc) const {
        uint32_t e[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const uint32_t g0 = GOL_BOP3(mc, s[2 * t], b[2 * t], kSelect);          // S9 = 2t
            const uint32_t g1 = GOL_BOP3(mc, s[2 * t + 1], b[2 * t + 1], kSelect);  // S9 = 2t + 1
            e[t] = GOL_BOP3(o, g1, g0, kSelect);
        }
        const uint32_t b1 = k ^ p;
        const uint32_t b2 = GOL_BOP3(k, p, q, GOL_TT((a & b) ^ c));
        const uint32_t b3 = GOL_BOP3(k, p, q, GOL_TT(a & b & c));
        const uint32_t f01 = GOL_BOP3(b1, e[1], e[0], kSelect);
        const uint32_t f23 = GOL_BOP3(b1, e[3], e[2], kSelect);
        const uint32_t f = GOL_BOP3(b2, f23, f01, kSelect);
        return GOL_BOP3(b3, e[4], f, kSelect);  // T = 4: b1 = b2 = 0
    }
};

// One level update under `rule` (level_update's drift form): `in` is the new row, `above` / `mid`
// the level's two previous rows; returns the next generation of `mid`, stores `in`'s state into
// `above` (now free).
template <class Rule>
__device__ __forceinline__ uint32_t rule_level(const Rule &rule, RowState<1> &above,
                                               const RowState<1> &mid, uint32_t in) {
    uint32_t ns, ncy, nctr;
    row_sum3_drift<NoNb>(in, ns, ncy, nctr);
    const uint32_t o = GOL_BOP3(above.s.w[0], mid.s.w[0], ns, kXor3);
    const uint32_t k = GOL_BOP3(above.s.w[0], mid.s.w[0], ns, kMaj);
    const uint32_t p = GOL_BOP3(above.cy.w[0], mid.cy.w[0], ncy, kXor3);
    const uint32_t q = GOL_BOP3(above.cy.w[0], mid.cy.w[0], ncy, kMaj);
    const uint32_t nx = rule.next(o, k, p, q, mid.c.w[0]);
    above.s.w[0] = ns;
    above.cy.w[0] = ncy;
    above.c.w[0] = nctr;
    return nx;
}

// K = generations per launch (levels chained: level j + 1 consumes the row level j produced in the
// same step; level j's rows sit j + 1 bits east in the lane frame); COUNT: per-generation counts;
// LD: the last generation's flips to p.diff beside the output.
template <int K, bool COUNT, bool LD, class Rule>
__global__ __launch_bounds__(256) void gol_rule(const uint32_t *__restrict__ in,
                                                uint32_t *__restrict__ out, StencilParams p,
                                                unsigned long long *__restrict__ slots, RuleMasks rm) {
    static_assert(K >= 1 && K <= 32, "drift with 62-word chunks: 2 K <= 64 stale bits");
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t chunk = wave % p.nchunks;
    const int64_t bandi = wave / p.nchunks;
    if (bandi >= p.nbands) return;  // wave-uniform
    if (p.prio) __builtin_amdgcn_s_setprio(3);
    int ya, yb;
    band_rows(p, bandi, ya, yb);
    const int colraw = (int)chunk * kRuleChunkWords + (lane - 1);
    const int col = (colraw + p.wd) % p.wd;
    RowStream rows(p, ya - K);
    auto load_next = [&]() -> uint32_t {
        const uint32_t v = in[(int64_t)rows.ly * p.pitch + col];
        rows.advance();
        return v;
    };
    // output (and flips) through one raw-buffer descriptor over the band's rows: see gol_stencil
    const int rowbytes = (int)(p.pitch * 4);
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
        out + (int64_t)ya * p.pitch, 0, (yb - ya) * rowbytes, kBufferRsrcWord3);
    __amdgpu_buffer_rsrc_t drsrc = orsrc;
    if constexpr (LD)
        drsrc = __builtin_amdgcn_make_buffer_rsrc(p.diff + (int64_t)ya * p.pitch, 0,
                                                  (yb - ya) * rowbytes, kBufferRsrcWord3);
    const LaneStore ls = lane_store<false>(lane, colraw, col, p.wd);
    // count window of the drifting 62-word geometry (gol_stencil): every lane counts whole words,
    // the lanes outside [2, the lane with colraw == wd] drop their sums at the flush
    const bool count_lane = lane >= 2 && colraw <= p.wd;
    const Rule rule(rm);

    RowState<1> X[K], Y[K];
    uint32_t acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        X[j].s.w[0] = X[j].cy.w[0] = X[j].c.w[0] = 0;
        Y[j].s.w[0] = Y[j].cy.w[0] = Y[j].c.w[0] = 0;
        acc[j] = 0;
    }
    const int nrows = yb - ya;
    constexpr int lag = 2 * K;  // steps before the first stored row
    const int nsteps = nrows + lag;

    // One step: a new level-0 row enters, every level emits one row (level j's is row
    // ya - K + st - (j + 1), valid from step 2 j + 2 on; the rows of the pipeline fill are computed
    // and dropped), the level-K row is stored.  PAR 0: above = X, mid = Y; PAR 1: the other way.
    auto step = [&](auto par, uint32_t vin, int st) {
        constexpr int PAR = decltype(par)::value;
        uint32_t nc = vin;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            RowState<1> &above = PAR == 0 ? X[j] : Y[j];
            const RowState<1> &mid = PAR == 0 ? Y[j] : X[j];
            const uint32_t prev = mid.c.w[0];  // generation j of the output row, same frame
            uint32_t nx = rule_level(rule, above, mid, nc);
            if (COUNT) {
                const int r = st - K - (j + 1);
                if (r >= 0 && r < nrows) acc[j] += __builtin_popcount(nx);
            }
            if (j == K - 1) {
                const int r = st - lag;  // stored row - ya
                const int rowoff = (r >= 0 && r < nrows) ? r * rowbytes : kOutOfRange;
                Words<1> v, dv;
                v.w[0] = realign_drift<K>(nx);  // back to the board frame: K bits west
                store_row<1, false>(orsrc, ls, v, rowoff);
                if constexpr (LD) {
                    dv.w[0] = realign_drift<K>(nx ^ prev);
                    store_row<1, false>(drsrc, ls, dv, rowoff);
                }
            } else {
                nc = nx;
            }
        }
    };
    using Par0 = std::integral_constant<int, 0>;
    using Par1 = std::integral_constant<int, 1>;
    // Register prefetch ring: loads run P steps ahead of their use (deeper for small K, whose steps
    // are short).  The steps run in blocks of P: up to P - 1 extra steps past the band's end load
    // wrapped / clamped rows (RowStream) and store nothing.
    constexpr int P = K >= 4 ? 4 : (K == 2 ? 8 : 16);
    uint32_t buf[P];
#pragma unroll
    for (int u = 0; u < P; ++u) buf[u] = load_next();
    for (int s = 0; s < nsteps; s += P) {
#pragma unroll
        for (int u = 0; u < P; ++u) {
            const uint32_t vin = buf[u];
            buf[u] = load_next();
            if (u & 1)
                step(Par1{}, vin, s + u);
            else
                step(Par0{}, vin, s + u);
        }
    }
    if (COUNT) {
        if (!count_lane) {
#pragma unroll
            for (int j = 0; j < K; ++j) acc[j] = 0;
        }
        flush_counts<K>(acc, 0, lane, wave, slots);
    }
}

template <int K, class Rule>
hipError_t launch_rule_as(RuleMasks rm, const uint32_t *in, uint32_t *out, const StencilParams &p,
                          unsigned long long *slots, hipStream_t s) {
    const int64_t waves = p.nbands * (int64_t)p.nchunks;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, (waves + 3) / 4);
    if (p.diff && slots)
        hipLaunchKernelGGL((gol_rule<K, true, true, Rule>), dim3(blocks), dim3(256), 0, s, in, out, p, slots, rm);
    else if (p.diff)
        hipLaunchKernelGGL((gol_rule<K, false, true, Rule>), dim3(blocks), dim3(256), 0, s, in, out, p, slots, rm);
    else if (slots)
        hipLaunchKernelGGL((gol_rule<K, true, false, Rule>), dim3(blocks), dim3(256), 0, s, in, out, p, slots, rm);
    else
        hipLaunchKernelGGL((gol_rule<K, false, false, Rule>), dim3(blocks), dim3(256), 0, s, in, out, p, slots, rm);
    return hipGetLastError();
}

// A catalogue rule runs its constant-folded kernel, every other rule the table form.
template <int K>
hipError_t launch_rule_k(RuleMasks rm, const uint32_t *in, uint32_t *out, const StencilParams &p,
                         unsigned long long *slots, hipStream_t s) {
#define GOLHIP_X(B, S) \
    if (rm.birth == (B) && rm.survive == (S)) return launch_rule_as<K, RuleConst<(B), (S)>>(rm, in, out, p, slots, s);
    GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
    return launch_rule_as<K, RuleTable>(rm, in, out, p, slots, s);
}

// The kernel launch_rule_k<K> runs for this rule (without flips), for the occupancy query that sizes
// the grid: the functors and the counting kernels differ in VGPRs, hence in resident waves.
template <int K>
const void *rule_fn_k(RuleMasks rm, bool counting) {
#define GOLHIP_X(B, S)                                                                        \
    if (rm.birth == (B) && rm.survive == (S))                                                 \
        return counting ? (const void *)gol_rule<K, true, false, RuleConst<(B), (S)>>         \
                        : (const void *)gol_rule<K, false, false, RuleConst<(B), (S)>>;
    GOLHIP_RULE_CATALOGUE(GOLHIP_X)
#undef GOLHIP_X
    return counting ? (const void *)gol_rule<K, true, false, RuleTable>
                    : (const void *)gol_rule<K, false, false, RuleTable>;
}

}  // namespace

// Defines the rule launcher of depth K (launch_rule_k<K> / rule_fn_k<K>, declared in
// golhip_internal.hpp) in the TU that includes this header for one depth.
#define GOLHIP_DEFINE_RULE_K(K)                                                                  \
    hipError_t launch_rule_k##K(RuleMasks rm, const uint32_t *in, uint32_t *out,                \
                                const StencilParams &p, unsigned long long *slots, hipStream_t s) { \
        return launch_rule_k<K>(rm, in, out, p, slots, s);                                      \
    }                                                                                            \
    const void *rule_fn_k##K(RuleMasks rm, bool counting) { return rule_fn_k<K>(rm, counting); }

}  // namespace golhip
