// batch_rule.hpp -- gol_batch_rule<W, R, HIST, SETTLE, Rule>: gol_batch (batch_board.hip) for
// life-like rules B.../S..., shared by the per-functor translation units batch_rule_*.hip.
// B3/S23 never runs this.
//
// The generation step is sums16 and board_common.hpp's board_gen, as in gol_board and gol_batch.  The
// body around it -- loads, prev, HIST partials through cnt[2][4][16] flushed by wave 0 one group
// later, SETTLE through prev / last_diff, groups of 4 generations plus the 0..3 remainder,
// unrotate16 on the way out -- is gol_batch's, kept as a second copy (batch_board.hip says why) and
// described there.  None of it depends on the rule; the settle argument needs a deterministic rule
// only (once board(t) == board(t - 2) it holds for every later t), so it holds for any fixed rule,
// B0 rules and their period-2 strobing included.
//
// The one difference: where gol_batch's rule step is life_om, rule_om forms the sum bits o, k, p, q of a
// few rows op-major (four v_bitop3 per row, as life_om does) and hands each row to the functor of
// golhip_rule.hpp -- RuleConst<B, S> (7 v_bitop3, truth tables as immediates) for a catalogue rule,
// RuleTable (22 v_bitop3, the 18 rule bits expanded to 0 / ~0 words once per wave) for every other
// rule.  Same convention as gol_rule: the 9-cell sum includes the centre.
//
// Rule source: BatchRuleParams::rules == null: one rule for the launch (BatchRuleParams::rule).
// Otherwise board blockIdx.x reads its own (birth, survive) pair from rules[2 i], rules[2 i + 1]:
// the address is wave-uniform, so it is a scalar load and the expanded table lives in SGPRs.
// Per-board rules always run RuleTable, whatever the rules are.
//
// Interleave width (kRuleInterleave): life_om advances all NI = R - 2 interior rows of a segment
// op-major.  RuleConst keeps four partial results per row and does the same (64 VGPRs at (16, 8)
// plain: two workgroups per CU, as gol_batch).  RuleTable keeps five e[t] per row beside o, k, p,
// q: six rows wide is 73 VGPRs at (16, 8) plain, three 67, two 65, one row at a time 62 -- the only
// width that keeps the second 16-wave workgroup on a CU (<= 64), so that is what it runs; the 4 to
// 8 waves per SIMD cover the latency of the single chain.  No instantiation uses scratch.
#pragma once
#include "board_common.hpp"
#include "golhip_rule.hpp"

namespace golhip {
namespace {

template <class Rule>
constexpr int kRuleInterleave = Rule::kConst ? 6 : 1;

// The next generation of N rows under `rule`, IW rows at a time: their sum bits op-major, then the
// functor row by row.
template <int N, int IW, class Rule>
__device__ __forceinline__ void rule_om(const Rule &rule, const uint32_t (&as)[N], const uint32_t (&acy)[N],
                                        const uint32_t (&ms)[N], const uint32_t (&mcy)[N],
                                        const uint32_t (&mc)[N], const uint32_t (&bs)[N],
                                        const uint32_t (&bcy)[N], uint32_t (&out)[N]) {
#pragma unroll
    for (int i0 = 0; i0 < N; i0 += IW) {
        uint32_t o[IW], k[IW], pp[IW], q[IW];
#pragma unroll
        for (int i = 0; i < IW; ++i)
            if (i0 + i < N) o[i] = GOL_BOP3(as[i0 + i], ms[i0 + i], bs[i0 + i], kXor3);
#pragma unroll
        for (int i = 0; i < IW; ++i)
            if (i0 + i < N) k[i] = GOL_BOP3(as[i0 + i], ms[i0 + i], bs[i0 + i], kMaj);
#pragma unroll
        for (int i = 0; i < IW; ++i)
            if (i0 + i < N) pp[i] = GOL_BOP3(acy[i0 + i], mcy[i0 + i], bcy[i0 + i], kXor3);
#pragma unroll
        for (int i = 0; i < IW; ++i)
            if (i0 + i < N) q[i] = GOL_BOP3(acy[i0 + i], mcy[i0 + i], bcy[i0 + i], kMaj);
#pragma unroll
        for (int i = 0; i < IW; ++i)
            if (i0 + i < N) out[i0 + i] = rule.next(o[i], k[i], pp[i], q[i], mc[i0 + i]);
    }
}

// `rule` as board_gen's rule step.
template <class Rule>
struct RuleNext {
    Rule rule;
    template <int N>
    __device__ __forceinline__ void operator()(const uint32_t (&as)[N], const uint32_t (&acy)[N],
                                               const uint32_t (&ms)[N], const uint32_t (&mcy)[N],
                                               const uint32_t (&mc)[N], const uint32_t (&bs)[N],
                                               const uint32_t (&bcy)[N], uint32_t (&out)[N]) const {
        rule_om<N, kRuleInterleave<Rule>>(rule, as, acy, ms, mcy, mc, bs, bcy, out);
    }
};

template <int W, int R, bool HIST, bool SETTLE, class Rule>
__global__ __launch_bounds__(64 * W) void gol_batch_rule(BatchRuleParams rp, int K) {
    constexpr int NSEG = 4 * W;
    const BatchParams &p = rp.b;
    __shared__ uint32_t ex[2][NSEG][4][16];
    __shared__ uint32_t cnt[2][4][16];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c16 = lane & 15;
    const int sg = 4 * w + (lane >> 4);
    const int wd = p.wd;
    const bool own = c16 < wd;  // one copy of the replicated row is stored
    // HIST counts one copy of the BOARD's row, as gol_batch does
    const int cw = (p.width + 31) >> 5;
    const uint32_t cmask = c16 >= cw ? 0u : (c16 == cw - 1 && (p.width & 31)) ? (1u << (p.width & 31)) - 1u : ~0u;
    const int64_t boff = (int64_t)blockIdx.x * p.board_pitch;
    uint32_t *__restrict__ board = p.boards + boff;
    // the board's rule: its own pair (a scalar load: blockIdx.x is wave-uniform) or the launch's
    RuleMasks rm = rp.rule;
    if (rp.rules) {
        rm.birth = rp.rules[2 * (int64_t)blockIdx.x];
        rm.survive = rp.rules[2 * (int64_t)blockIdx.x + 1];
    }
    const RuleNext<Rule> next{Rule(rm)};
    uint32_t c[R];
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = board[(sg * R + r) * wd + (c16 & (wd - 1))];
    // SETTLE: board(t - 1) in board(t)'s frame; at t0 == 0 there is none
    uint32_t old[SETTLE ? R : 1];
    uint32_t last = 0;  // 1 + the last generation of this launch whose result differed (0: none)
    const int gmin = p.t0 > 0 ? 0 : 1;
    if constexpr (SETTLE) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            old[r] = gmin == 0 ? p.prev[boff + (sg * R + r) * wd + (c16 & (wd - 1))] : 0u;
        }
    }
    const int up = (sg + NSEG - 1) % NSEG, dn = (sg + 1) % NSEG;
    // generation g (exchange buffer par): the rows advance in place; returns this lane's alive
    // cells of the new generation (HIST)
    auto gen = [&](int g, int par) -> uint32_t {
        uint32_t s[R], cy[R], ctr[R], nx[R];
        sums16<R>(c, s, cy, ctr);
        board_gen<R>(s, cy, ctr, ex, par, sg, up, dn, c16, next, nx);
        uint32_t a = 0;
        if constexpr (HIST)
#pragma unroll
            for (int r = 0; r < R; ++r) a += (uint32_t)__builtin_popcount(nx[r] & cmask);
        if constexpr (SETTLE) {
            uint32_t wl[R], e1[R], acc = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) wl[r] = west16(old[r]);
#pragma unroll
            for (int r = 0; r < R; ++r) e1[r] = __builtin_amdgcn_alignbit(old[r], wl[r], 31);  // one more bit east
#pragma unroll
            for (int r = 0; r < R; ++r) acc = GOL_BOP3(acc, nx[r], e1[r], GOL_TT(a | (b ^ c)));
            if (acc != 0 && g >= gmin) last = (uint32_t)g + 1;
            // pin the compare to its generation (see gol_batch)
            asm volatile("" : "+v"(last));
#pragma unroll
            for (int r = 0; r < R; ++r) old[r] = ctr[r];  // board(t) in board(t + 1)'s frame, from sums16
        }
#pragma unroll
        for (int r = 0; r < R; ++r) c[r] = nx[r];
        return a;
    };
    // HIST: wave 0 sums the W partials of the n generations from g0 that lie in cnt[buf]
    auto flush = [&](int buf, int g0, int n) {
        if (w == 0) {
            const int u = lane >> 4;
            uint32_t v = c16 < W ? cnt[buf][u][c16] : 0u;
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
            if (c16 == 15 && u < n) p.hist[(int64_t)blockIdx.x * K + g0 + u] = v;
        }
    };
    int g = 0, grp = 0;
#pragma clang loop unroll(disable)
    for (; g + 4 <= K; g += 4, ++grp) {
        uint32_t a[4];
        a[0] = gen(g, 0);
        a[1] = gen(g + 1, 1);
        a[2] = gen(g + 2, 0);
        a[3] = gen(g + 3, 1);
        if constexpr (HIST) {
            wave_sum_dpp_n<4>(a);
            if (grp > 0) flush((grp - 1) & 1, g - 4, 4);
            if (lane == 63)
#pragma unroll
                for (int u = 0; u < 4; ++u) cnt[grp & 1][u][w] = a[u];
        }
    }
    const int rem = K - g;  // 0..3 generations left: one more, partial, group
    if (rem > 0) {
        uint32_t a[4] = {0, 0, 0, 0};
        a[0] = gen(g, 0);
        if (rem > 1) a[1] = gen(g + 1, 1);
        if (rem > 2) a[2] = gen(g + 2, 0);
        if constexpr (HIST) {
            wave_sum_dpp_n<4>(a);
            if (grp > 0) flush((grp - 1) & 1, g - 4, 4);
            if (lane == 63)
#pragma unroll
                for (int u = 0; u < 4; ++u) cnt[grp & 1][u][w] = a[u];
        }
        ++grp;
    }
    if constexpr (HIST) {  // the last group's partials: one more barrier orders them
        lds_barrier();
        flush((grp - 1) & 1, (grp - 1) * 4, rem > 0 ? rem : 4);
    }
    // the rows back in the board frame (K bits west around the torus), one copy stored
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t v = unrotate16(c[r], lane, K);
        if (own) board[(sg * R + r) * wd + c16] = v;
        if constexpr (SETTLE) {
            const uint32_t o = unrotate16(old[r], lane, K);
            if (own) p.prev[boff + (sg * R + r) * wd + c16] = o;
        }
    }
    if constexpr (SETTLE) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) last = max(last, (uint32_t)__shfl_xor((int)last, off, 64));
        if (lane == 0 && last)
            atomicMax(&p.last_diff[blockIdx.x], (unsigned long long)p.t0 + (unsigned long long)last);
    }
}

template <int W, int R, class Rule>
hipError_t launch_batch_rule_wr(int K, int nboards, const BatchRuleParams &rp, hipStream_t s) {
    const bool hist = rp.b.hist != nullptr, settle = rp.b.prev != nullptr;
    const dim3 grid((unsigned)nboards), block(64 * W);
    if (hist && settle)
        hipLaunchKernelGGL((gol_batch_rule<W, R, true, true, Rule>), grid, block, 0, s, rp, K);
    else if (hist)
        hipLaunchKernelGGL((gol_batch_rule<W, R, true, false, Rule>), grid, block, 0, s, rp, K);
    else if (settle)
        hipLaunchKernelGGL((gol_batch_rule<W, R, false, true, Rule>), grid, block, 0, s, rp, K);
    else
        hipLaunchKernelGGL((gol_batch_rule<W, R, false, false, Rule>), grid, block, 0, s, rp, K);
    return hipGetLastError();
}

// Every shape of the table under one functor.
template <class Rule>
hipError_t launch_batch_rule_as(int K, int W, int R, int nboards, const BatchRuleParams &rp, hipStream_t s) {
#define GOLHIP_X(WW, RR) \
    if (W == WW && R == RR) return launch_batch_rule_wr<WW, RR, Rule>(K, nboards, rp, s);
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

}  // namespace

// One functor per translation unit (the build compiles them side by side): the constant-folded
// kernels of catalogue rule (B, S), declared in golhip_internal.hpp as launch_batch_rule_<B>_<S>.
#define GOLHIP_DEFINE_BATCH_RULE_CONST(B, S)                                                              \
    hipError_t launch_batch_rule_##B##_##S(int K, int W, int R, int nboards, const BatchRuleParams &rp, \
                                           hipStream_t s) {                                              \
        return launch_batch_rule_as<RuleConst<(B), (S)>>(K, W, R, nboards, rp, s);                      \
    }

}  // namespace golhip
