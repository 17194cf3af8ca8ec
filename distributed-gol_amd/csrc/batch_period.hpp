// batch_period.hpp -- gol_batch_period<W, R, HIST, Rule>: gol_batch / gol_batch_rule with per-board
// cycle detection (Brent, snapshots at turns 2^j - 1), shared by the per-functor translation units
// batch_period_*.hip.  A batch without period tracking never runs this.
//
// The definition.  For t >= 1 let s(t) = 2^floor(log2 t) - 1 (0 for t = 1, 1 for t = 2..3, 3 for
// t = 4..7, ...).  A board repeats at turn t when board(t) == board(s(t)) over the whole torus;
// repeat_turn[board] is the smallest such t that has been run, -1 before.  The rule is
// deterministic, so repeat_turn - s(repeat_turn) is exactly the period of the cycle the board has
// entered (offsets inside a window only run up to the window's length, so the first match is one
// period after the snapshot); the host derives it.
//
// The generation step is sums16 and board_common.hpp's board_gen, as in gol_board, gol_batch and
// gol_batch_rule, with the rule as its functor: LifeNext (B3/S23), RuleNext<RuleConst<B, S>> (a
// catalogue rule), RuleNext<RuleTable> (any rule; with BatchPeriodParams::rules != null board i reads its
// own pair, a scalar load, as gol_batch_rule does).  Loads, HIST partials through cnt flushed by
// wave 0 one group later, groups of 4 generations plus the 0..3 remainder and unrotate16 on the way
// out are gol_batch's, a third copy of that body (batch_board.hip says why the bodies are not
// folded).
//
// Snapshot rows: each lane keeps the snapshot of its R rows in R more VGPRs, loaded from `snap` at
// launch start (at t0 == 0 the snapshot IS the loaded board) and stored back un-rotated at the end,
// as SETTLE does with prev.  The frame drifts one bit east per generation, so the snapshot moves one
// bit east per generation (one DPP + one v_alignbit per row) and one v_bitop3 per row ORs its XOR
// with the new row into an accumulator: 3 VALU per word per generation, SETTLE's price.  After the
// generation that completes a turn 2^j - 1 the snapshot becomes the new rows (workgroup-uniform, R
// moves).
//
// Match mask: a repeat needs every lane of every wave to match at the SAME generation, so unlike
// SETTLE the lanes cannot just keep a maximum.  They do not vote per generation either: a lane sets
// bit (g mod 32) of a mask when all its rows matched at generation g; once per 32 generations and at
// the end of the launch the mask is AND-reduced over the wave (6 DPP steps) and lane 63 puts it
// into LDS, pm[block parity][w].  The next group's barriers order those stores before wave 0 reads
// them at that group's end (as HIST's cnt; one more barrier at the very end for the last block),
// ANDs the W masks and takes the lowest set bit: turn t0 + 32 block + bit + 1.  Wave 0 reads
// repeat_turn[board] once at launch start and stores once, if it was -1: a plain store -- one
// workgroup owns a board and launches are stream-ordered.  The buffer parity is safe as cnt's is:
// block k + 2 overwrites pm[k & 1] 64 barriers after wave 0 read it.
#pragma once
#include <type_traits>

#include "batch_rule.hpp"

namespace golhip {
namespace {

// board_gen's rule step for functor class Rule: LifeNext itself, or RuleNext<Rule> over the masks.
template <class Rule>
__device__ __forceinline__ auto period_next(RuleMasks rm) {
    if constexpr (std::is_same_v<Rule, LifeNext>)
        return LifeNext{};
    else
        return RuleNext<Rule>{Rule(rm)};
}

// AND of v over the wave, valid in lane 63 (wave_sum_dpp's steps with AND; lanes a step does not
// write keep ~0 or their own value, which only ever holds fewer terms).
__device__ __forceinline__ uint32_t wave_and_dpp(uint32_t v) {
    v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x112, 0xf, 0xf, false);
    v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x114, 0xf, 0xf, false);
    v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x118, 0xf, 0xf, false);
    v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return v;
}

template <int W, int R, bool HIST, class Rule>
__global__ __launch_bounds__(64 * W) void gol_batch_period(BatchPeriodParams pp, int K) {
    constexpr int NSEG = 4 * W;
    const BatchParams &p = pp.b;
    __shared__ uint32_t ex[2][NSEG][4][16];
    __shared__ uint32_t cnt[2][4][16];
    __shared__ uint32_t pm[2][16];
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
    uint32_t *__restrict__ snapb = pp.snap + boff;
    RuleMasks rm = pp.rule;
    if constexpr (!std::is_same_v<Rule, LifeNext>) {
        if (pp.rules) {  // the board's own pair (a scalar load: blockIdx.x is wave-uniform)
            rm.birth = pp.rules[2 * (int64_t)blockIdx.x];
            rm.survive = pp.rules[2 * (int64_t)blockIdx.x + 1];
        }
    }
    const auto next = period_next<Rule>(rm);
    // a repeat found by an earlier launch stands
    bool found = pp.repeat_turn[blockIdx.x] >= 0;
    uint32_t c[R], sn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = board[(sg * R + r) * wd + (c16 & (wd - 1))];
    // the snapshot board(s(t0 + 1)) in board(t0)'s frame; at t0 == 0 it is board(0)
    if (p.t0 > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) sn[r] = snapb[(sg * R + r) * wd + (c16 & (wd - 1))];
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) sn[r] = c[r];
    }
    uint32_t m = 0;  // bit g % 32: every row of this lane matched the snapshot at generation g
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
        uint32_t wl[R], acc = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) wl[r] = west16(sn[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) sn[r] = __builtin_amdgcn_alignbit(sn[r], wl[r], 31);  // one bit east
#pragma unroll
        for (int r = 0; r < R; ++r) acc = GOL_BOP3(acc, nx[r], sn[r], GOL_TT(a | (b ^ c)));
        if (acc == 0) m |= 1u << (g & 31);
        // pin the compare to its generation (see gol_batch)
        asm volatile("" : "+v"(m));
        // the turn this generation completes is t0 + g + 1; after turn 2^j - 1 the snapshot is
        // the new board (workgroup-uniform)
        const uint64_t t1 = (uint64_t)p.t0 + (uint64_t)g + 2;  // the turn + 1
        if ((t1 & (t1 - 1)) == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) sn[r] = nx[r];
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
    // the wave's match mask of block blk (generations [32 blk, 32 blk + 32) of the launch) to LDS
    auto put_mask = [&](int blk) {
        const uint32_t v = wave_and_dpp(m);
        if (lane == 63) pm[blk & 1][w] = v;
        m = 0;
    };
    // wave 0: the W masks of block blk, ordered by a barrier since put_mask; the first repeat
    auto take_mask = [&](int blk) {
        if (w == 0) {
            uint32_t v = pm[blk & 1][c16 & (W - 1)];
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x112, 0xf, 0xf, false);
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x114, 0xf, 0xf, false);
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x118, 0xf, 0xf, false);
            // lane 15 holds the AND of the row's 16 lanes: every wave's mask, W | 16
            if (lane == 15 && v != 0 && !found)
                pp.repeat_turn[blockIdx.x] = p.t0 + 32 * (int64_t)blk + (int64_t)__builtin_ctz(v) + 1;
            found = found || __builtin_amdgcn_readlane((int)v, 15) != 0;
        }
    };
    int g = 0, grp = 0;
    int pend = -1;  // the block whose masks lie in LDS, not yet taken by wave 0
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
        if (pend >= 0) {
            take_mask(pend);
            pend = -1;
        }
        if ((grp & 7) == 7) {
            pend = grp >> 3;
            put_mask(pend);
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
        if (pend >= 0) {
            take_mask(pend);
            pend = -1;
        }
        ++grp;
    }
    // the last block if it is a partial one (bits of generations not run stay 0; a full block
    // before it was taken by the group that followed it), then one more barrier orders the last
    // masks and HIST's last partials
    if ((K & 31) != 0) {
        pend = (K - 1) >> 5;
        put_mask(pend);
    }
    lds_barrier();
    if (pend >= 0) take_mask(pend);
    if constexpr (HIST) flush((grp - 1) & 1, (grp - 1) * 4, rem > 0 ? rem : 4);
    // the rows back in the board frame (K bits west around the torus), one copy stored
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t v = unrotate16(c[r], lane, K);
        if (own) board[(sg * R + r) * wd + c16] = v;
        const uint32_t o = unrotate16(sn[r], lane, K);
        if (own) snapb[(sg * R + r) * wd + c16] = o;
    }
}

template <int W, int R, class Rule>
hipError_t launch_batch_period_wr(int K, int nboards, const BatchPeriodParams &pp, hipStream_t s) {
    const dim3 grid((unsigned)nboards), block(64 * W);
    if (pp.b.hist)
        hipLaunchKernelGGL((gol_batch_period<W, R, true, Rule>), grid, block, 0, s, pp, K);
    else
        hipLaunchKernelGGL((gol_batch_period<W, R, false, Rule>), grid, block, 0, s, pp, K);
    return hipGetLastError();
}

// Every shape of the table under one functor.
template <class Rule>
hipError_t launch_batch_period_as(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s) {
#define GOLHIP_X(WW, RR) \
    if (W == WW && R == RR) return launch_batch_period_wr<WW, RR, Rule>(K, nboards, pp, s);
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

}  // namespace

// One functor per translation unit (the build compiles them side by side): the constant-folded
// kernels of catalogue rule (B, S), declared in golhip_internal.hpp as launch_batch_period_<B>_<S>.
#define GOLHIP_DEFINE_BATCH_PERIOD_CONST(B, S)                                                                \
    hipError_t launch_batch_period_##B##_##S(int K, int W, int R, int nboards, const BatchPeriodParams &pp, \
                                             hipStream_t s) {                                                \
        return launch_batch_period_as<RuleConst<(B), (S)>>(K, W, R, nboards, pp, s);                        \
    }

}  // namespace golhip
