// batch_plane.hpp -- the batch kernels on a bounded plane: gol_plane_rule<W, R, HIST, SETTLE, Rule>,
// gol_plane_period<W, R, HIST, Rule> and gol_plane_search<W, R, Rule>, shared by the translation
// units batch_plane_*.hip.  A plane of width x height is the torus's cells with every neighbour
// outside the rectangle dead (Golly's :P where the torus is :T).  A torus batch never runs these:
// the torus kernels (batch_board.hip, batch_rule.hpp, batch_period.hpp, batch_search.hpp) and
// board_common.hpp are untouched, so their code objects are the ones they were.  The one
// exception is a BOXED search on the torus (golhip_batch_set_soup_box), which runs gol_plane_search
// with its plane switch off: the seam mask is all ones and the segments wrap, at no cost per
// generation.
//
// Geometry: board_common.hpp's.  The rows still drift one bit east per generation around the
// replicated 512-bit ring of a 16-lane row, and a row narrower than 512 cells is still replicated:
// position P = 32 lane + bit of a row with drift d holds column (P - d) mod width.  Two seams:
//
// Vertical.  Segment 0 has no row above it and segment NSEG - 1 none below.  The exchange array gets
// one more slot, ex[2][NSEG + 1][4][16], which nobody writes after it has been zeroed before the
// first barrier; segment 0 reads its upper neighbour's edge sums there (up = NSEG) and the last
// segment its lower neighbour's (dn = NSEG): sums of a dead row.  board_gen deduces the array's extent
// and indexes it by sg, up and dn only, so it runs as it is: no instruction per generation.
//
// Horizontal.  sums16 adds, for the centre ctr (the row moved one bit east, position P holding the
// cell that was at P - 1), its west neighbour w2 (from P - 2) and its east neighbour x (from P).
// On a plane w2 must vanish where the centre is column 0 and x where the centre is column
// width - 1.  With Z the word of a mask whose bit at position P is 0 where (P - d) mod width == 0
// and 1 elsewhere: x's bit at P is the east neighbour of the cell of column (P - 1 - d), which is
// width - 1 exactly where Z is 0, so xe = x & Z; and Z moved one bit east (Zn: 0 where
// (P - 1 - d) mod width == 0, the centre in column 0) masks w2.  Zn is also the Z of the next
// generation's frame, drift d + 1.  ctr stays unmasked: SETTLE and the snapshot compare need the
// true old rows.  Z is periodic with period `width` like the rows (all zeros for width 1), so the
// replicated copies stay identical and HIST's one-copy count holds.  Every launch starts with
// drift 0 (the stores unrotate16 the boards), so Z starts as plane_z0.  Cost: one DPP and one
// v_alignbit for Z and two v_and per row, 2 R + 2 VALU per generation.
//
// The bodies around the step -- loads, HIST through cnt, SETTLE through prev / last_diff, the Brent
// snapshot and match masks, the search's retirement -- are the torus kernels', copied (batch_board.hip
// says why the bodies are not folded) and described in batch_rule.hpp, batch_period.hpp and
// batch_search.hpp.  Functors: LifeNext for a uniform B3/S23, RuleNext<RuleTable> for every other
// rule and for per-board rules; the plane has no constant-folded catalogue kernels.
//
// The soup box (SoupBox): box_word_mask gives, for word `col` of row y, the bits whose cell lies in
// the box.  gol_plane_search ANDs it into the words it seeds; batch_clip_box (batch_plane_box.hip)
// ANDs it into the boards batch_init_random wrote; the mask lives in golhip_internal.hpp beside
// init_random_word.
#pragma once
#include "batch_search.hpp"

namespace golhip {
namespace {

// Z at drift 0 for lane column c16: 0 at every position whose column is 0.
__device__ __forceinline__ uint32_t plane_z0(int width, int c16) {
    if (width >= 32) return ((32 * c16) & (width - 1)) == 0 ? ~1u : ~0u;
    return ~(0xffffffffu / ((1u << width) - 1u));  // one 0 every `width` bits; width 1: all zeros
}

// sums16 on a plane: Z is this generation's seam mask and leaves as the next one's.
template <int N>
__device__ __forceinline__ void sums16_plane(const uint32_t (&x)[N], uint32_t &Z, uint32_t (&s)[N],
                                             uint32_t (&cy)[N], uint32_t (&ctr)[N]) {
    uint32_t wl[N], w2[N], xe[N];
    const uint32_t Zn = __builtin_amdgcn_alignbit(Z, west16(Z), 31);  // one bit east, as the rows
#pragma unroll
    for (int i = 0; i < N; ++i) wl[i] = west16(x[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) ctr[i] = __builtin_amdgcn_alignbit(x[i], wl[i], 31);  // cell x-1 onto x
#pragma unroll
    for (int i = 0; i < N; ++i) w2[i] = __builtin_amdgcn_alignbit(x[i], wl[i], 30) & Zn;  // cell x-2, none west of column 0
#pragma unroll
    for (int i = 0; i < N; ++i) xe[i] = x[i] & Z;  // none east of column width - 1
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = GOL_BOP3(w2[i], ctr[i], xe[i], kXor3);
#pragma unroll
    for (int i = 0; i < N; ++i) cy[i] = GOL_BOP3(w2[i], ctr[i], xe[i], kMaj);
    Z = Zn;
}

// The dead row beyond the top and the bottom: slot NSEG of both exchange buffers, zeroed once.  The
// first generation's barrier orders the stores before any read.
template <int NSEG>
__device__ __forceinline__ void plane_zero_slot(uint32_t (&ex)[2][NSEG + 1][4][16]) {
    if (threadIdx.x < 64) {
        (&ex[0][NSEG][0][0])[threadIdx.x] = 0u;
        (&ex[1][NSEG][0][0])[threadIdx.x] = 0u;
    }
}

template <int W, int R, bool HIST, bool SETTLE, class Rule>
__global__ __launch_bounds__(64 * W) void gol_plane_rule(BatchRuleParams rp, int K) {
    constexpr int NSEG = 4 * W;
    const BatchParams &p = rp.b;
    __shared__ uint32_t ex[2][NSEG + 1][4][16];
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
    RuleMasks rm = rp.rule;
    if constexpr (!std::is_same_v<Rule, LifeNext>) {
        if (rp.rules) {  // the board's own pair (a scalar load: blockIdx.x is wave-uniform)
            rm.birth = rp.rules[2 * (int64_t)blockIdx.x];
            rm.survive = rp.rules[2 * (int64_t)blockIdx.x + 1];
        }
    }
    const auto next = period_next<Rule>(rm);
    plane_zero_slot<NSEG>(ex);
    uint32_t Z = plane_z0(p.width, c16);
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
    // the dead row's slot beyond the first and the last segment
    const int up = sg == 0 ? NSEG : sg - 1, dn = sg == NSEG - 1 ? NSEG : sg + 1;
    // generation g (exchange buffer par): the rows advance in place; returns this lane's alive
    // cells of the new generation (HIST)
    auto gen = [&](int g, int par) -> uint32_t {
        uint32_t s[R], cy[R], ctr[R], nx[R];
        sums16_plane<R>(c, Z, s, cy, ctr);
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
            for (int r = 0; r < R; ++r) old[r] = ctr[r];  // board(t) in board(t + 1)'s frame, unmasked
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
    // the rows back in the board frame (K bits west around the ring), one copy stored
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

template <int W, int R, bool HIST, class Rule>
__global__ __launch_bounds__(64 * W) void gol_plane_period(BatchPeriodParams pp, int K) {
    constexpr int NSEG = 4 * W;
    const BatchParams &p = pp.b;
    __shared__ uint32_t ex[2][NSEG + 1][4][16];
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
    plane_zero_slot<NSEG>(ex);
    uint32_t Z = plane_z0(p.width, c16);
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
    // the dead row's slot beyond the first and the last segment
    const int up = sg == 0 ? NSEG : sg - 1, dn = sg == NSEG - 1 ? NSEG : sg + 1;
    // generation g (exchange buffer par): the rows advance in place; returns this lane's alive
    // cells of the new generation (HIST)
    auto gen = [&](int g, int par) -> uint32_t {
        uint32_t s[R], cy[R], ctr[R], nx[R];
        sums16_plane<R>(c, Z, s, cy, ctr);
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
    // the last block if it is a partial one, then one more barrier orders the last masks and
    // HIST's last partials (gol_batch_period)
    if ((K & 31) != 0) {
        pend = (K - 1) >> 5;
        put_mask(pend);
    }
    lds_barrier();
    if (pend >= 0) take_mask(pend);
    if constexpr (HIST) flush((grp - 1) & 1, (grp - 1) * 4, rem > 0 ? rem : 4);
    // the rows back in the board frame (K bits west around the ring), one copy stored
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t v = unrotate16(c[r], lane, K);
        if (own) board[(sg * R + r) * wd + c16] = v;
        const uint32_t o = unrotate16(sn[r], lane, K);
        if (own) snapb[(sg * R + r) * wd + c16] = o;
    }
}

template <int W, int R, class Rule>
__global__ __launch_bounds__(64 * W) void gol_plane_search(BatchBoxSearchParams bp) {
    constexpr int NSEG = 4 * W;
    const BatchSearchParams &sp = bp.s;
    __shared__ uint32_t ex[2][NSEG + 1][4][16];
    __shared__ uint32_t pm[2][16];
    __shared__ uint32_t pop[16];
    __shared__ uint32_t stop;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c16 = lane & 15;
    const int sg = 4 * w + (lane >> 4);
    const int wd = sp.wd;
    const int K = sp.max_turns;
    // one copy of the BOARD's row, as gol_batch's HIST counts it
    const int cw = (sp.width + 31) >> 5;
    const uint32_t cmask = c16 >= cw ? 0u : (c16 == cw - 1 && (sp.width & 31)) ? (1u << (sp.width & 31)) - 1u : ~0u;
    RuleMasks rm = sp.rule;
    if constexpr (!std::is_same_v<Rule, LifeNext>) {
        if (sp.rules) {  // the soup's own pair (a scalar load: blockIdx.x is wave-uniform)
            rm.birth = sp.rules[2 * (int64_t)blockIdx.x];
            rm.survive = sp.rules[2 * (int64_t)blockIdx.x + 1];
        }
    }
    const auto next = period_next<Rule>(rm);
    const uint64_t seed = sp.seeds ? sp.seeds[blockIdx.x] : sp.seed0 + (uint64_t)blockIdx.x;
    if (threadIdx.x == 0) stop = 0;
    plane_zero_slot<NSEG>(ex);
    // a boxed search on the torus: no seam mask, and the segments wrap
    const bool plane = bp.plane != 0;
    uint32_t Z = plane ? plane_z0(sp.width, c16) : ~0u;
    uint32_t c[R], sn[R];
    // the soup of the seed with every cell outside the box cleared
#pragma unroll
    for (int r = 0; r < R; ++r)
        c[r] = init_random_word(seed, sg * R + r, c16 & (wd - 1), sp.width, sp.density) &
               box_word_mask(sg * R + r, c16 & (wd - 1), sp.width, bp.box);
#pragma unroll
    for (int r = 0; r < R; ++r) sn[r] = c[r];  // board(0) is the first snapshot
    uint32_t m = 0;  // bit g % 32: every row of this lane matched the snapshot at generation g
    int rep = -1;    // wave 0: the first repeat turn
    const int up = sg == 0 ? (plane ? NSEG : NSEG - 1) : sg - 1;
    const int dn = sg == NSEG - 1 ? (plane ? NSEG : 0) : sg + 1;
    // generation g (exchange buffer par): the rows advance in place
    auto gen = [&](int g, int par) {
        uint32_t s[R], cy[R], ctr[R], nx[R];
        sums16_plane<R>(c, Z, s, cy, ctr);
        board_gen<R>(s, cy, ctr, ex, par, sg, up, dn, c16, next, nx);
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
        // this generation completes turn g + 1; after turn 2^j - 1 the snapshot is the new board
        const uint32_t t1 = (uint32_t)g + 2;  // the turn + 1
        if ((t1 & (t1 - 1)) == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) sn[r] = nx[r];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) c[r] = nx[r];
    };
    // the wave's match mask of block blk (generations [32 blk, 32 blk + 32)) to LDS
    auto put_mask = [&](int blk) {
        const uint32_t v = wave_and_dpp(m);
        if (lane == 63) pm[blk & 1][w] = v;
        m = 0;
    };
    // wave 0: the W masks of block blk, ordered by a barrier since put_mask; the first repeat
    // retires the soup
    auto take_mask = [&](int blk) {
        if (w == 0) {
            uint32_t v = pm[blk & 1][c16 & (W - 1)];
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x112, 0xf, 0xf, false);
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x114, 0xf, 0xf, false);
            v &= (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)v, 0x118, 0xf, 0xf, false);
            // lane 15 holds the AND of the row's 16 lanes: every wave's mask, W | 16
            const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
            if (all != 0 && rep < 0) {
                rep = 32 * blk + __builtin_ctz(all) + 1;
                if (lane == 0) stop = 1;
            }
        }
    };
    int g = 0, grp = 0;
    int pend = -1;  // the block whose masks lie in LDS, not yet taken by wave 0
    bool retired = false;
#pragma clang loop unroll(disable)
    while (g + 4 <= K) {
        gen(g, 0);
        gen(g + 1, 1);
        gen(g + 2, 0);
        gen(g + 3, 1);
        g += 4;
        if (pend >= 0) {
            take_mask(pend);
            pend = -1;
        }
        if ((grp & 7) == 7) {
            pend = grp >> 3;
            put_mask(pend);
        }
        // the one exit: the same group in every wave, the same value in every wave
        // (batch_search.hpp has the argument; nothing in it depends on the topology)
        if ((grp & 7) == 1 && __builtin_amdgcn_readfirstlane((int)stop) != 0) {
            retired = true;
            break;
        }
        ++grp;
    }
    if (!retired) {
        const int rem = K - g;  // 0..3 generations left: one more, partial, group
        if (rem > 0) {
            gen(g, 0);
            if (rem > 1) gen(g + 1, 1);
            if (rem > 2) gen(g + 2, 0);
            g = K;
            if (pend >= 0) {
                take_mask(pend);
                pend = -1;
            }
        }
        // the last block if it is a partial one
        if ((K & 31) != 0) {
            pend = (K - 1) >> 5;
            put_mask(pend);
        }
    }
    // the alive cells of board(g); one more barrier orders the waves' sums and the last masks
    uint32_t a = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) a += (uint32_t)__builtin_popcount(c[r] & cmask);
    a = wave_sum_dpp(a);
    if (lane == 63) pop[w] = a;
    lds_barrier();
    if (pend >= 0) take_mask(pend);
    if (w == 0) {
        uint32_t v = lane < W ? pop[lane] : 0u;
        v = wave_sum_dpp(v);
        if (lane == 63) {
            SoupRecord rec;
            rec.repeat_turn = rep;
            // t - s(t), s(t) = 2^floor(log2 t) - 1: the snapshot turn of the window t lies in
            rec.period = rep > 0 ? rep - ((1 << (31 - __builtin_clz((uint32_t)rep))) - 1) : -1;
            rec.stop_turn = g;
            rec.population = v;
            rec.reserved = 0;
            sp.out[blockIdx.x] = rec;
        }
    }
}

template <int W, int R, class Rule>
hipError_t launch_plane_rule_wr(int K, int nboards, const BatchRuleParams &rp, hipStream_t s) {
    const bool hist = rp.b.hist != nullptr, settle = rp.b.prev != nullptr;
    const dim3 grid((unsigned)nboards), block(64 * W);
    if (hist && settle)
        hipLaunchKernelGGL((gol_plane_rule<W, R, true, true, Rule>), grid, block, 0, s, rp, K);
    else if (hist)
        hipLaunchKernelGGL((gol_plane_rule<W, R, true, false, Rule>), grid, block, 0, s, rp, K);
    else if (settle)
        hipLaunchKernelGGL((gol_plane_rule<W, R, false, true, Rule>), grid, block, 0, s, rp, K);
    else
        hipLaunchKernelGGL((gol_plane_rule<W, R, false, false, Rule>), grid, block, 0, s, rp, K);
    return hipGetLastError();
}

// Every shape of the table under one functor.
template <class Rule>
hipError_t launch_plane_rule_as(int K, int W, int R, int nboards, const BatchRuleParams &rp, hipStream_t s) {
#define GOLHIP_X(WW, RR) \
    if (W == WW && R == RR) return launch_plane_rule_wr<WW, RR, Rule>(K, nboards, rp, s);
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

template <class Rule>
hipError_t launch_plane_period_as(int K, int W, int R, int nboards, const BatchPeriodParams &pp, hipStream_t s) {
#define GOLHIP_X(WW, RR)                                                                                          \
    if (W == WW && R == RR) {                                                                                     \
        const dim3 grid((unsigned)nboards), block(64 * WW);                                                      \
        if (pp.b.hist)                                                                                            \
            hipLaunchKernelGGL((gol_plane_period<WW, RR, true, Rule>), grid, block, 0, s, pp, K);               \
        else                                                                                                      \
            hipLaunchKernelGGL((gol_plane_period<WW, RR, false, Rule>), grid, block, 0, s, pp, K);              \
        return hipGetLastError();                                                                                 \
    }
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

template <class Rule>
hipError_t launch_plane_search_as(int W, int R, int nsoups, const BatchBoxSearchParams &bp, hipStream_t s) {
#define GOLHIP_X(WW, RR)                                                                                        \
    if (W == WW && R == RR) {                                                                                   \
        hipLaunchKernelGGL((gol_plane_search<WW, RR, Rule>), dim3((unsigned)nsoups), dim3(64 * WW), 0, s, bp); \
        return hipGetLastError();                                                                               \
    }
    GOLHIP_BOARD_SHAPES(GOLHIP_X)
#undef GOLHIP_X
    return hipErrorInvalidValue;
}

inline bool plane_is_life(const RuleMasks &rule, const uint32_t *rules) {
    return !rules && rule.birth == kLifeBirth && rule.survive == kLifeSurvive;
}

}  // namespace
}  // namespace golhip
